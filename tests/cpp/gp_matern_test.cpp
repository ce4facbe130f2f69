// gp_matern_test.cpp — the Matern kernels through the C++ host API on the device:
// GaussianProcess<double> with Sum(Matern52, Gaussian) (Initialize, Predict, GetCredibleInterval
// against a dense host solve of the same system), a Save / Load round trip that gives the same
// predictions, and GaussianLogLikelihood's gradient against central differences of its value.
// Prints one line per case; exit status = #failures.  Built by `make cpptests`; driven by
// tests/test_gpu_matern_host.py (-m gpu).
#include <cmath>
#include <cstdio>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gpr/GaussianProcess.h"
#include "gpr/Kernel.h"
#include "gpr/Likelihood.h"

using namespace gpr;

typedef GaussianProcess<double> G;
typedef Kernel<double>::Pointer KP;

static int g_fail = 0;
static void run(const char* name, const std::function<void()>& f) {
    try {
        f();
        std::printf("PASS %s\n", name);
    } catch (const std::string& s) {
        std::printf("FAIL %s: %s\n", name, s.c_str());
        g_fail++;
    }
    std::fflush(stdout);
}
static void check(bool ok, const std::string& what) {
    if (!ok) throw what;
}
static std::string num(double v) {
    std::ostringstream s;
    s << v;
    return s.str();
}

static double unit(unsigned long long i) {
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static G::VectorType point(unsigned long long i) {
    G::VectorType x(2);
    x(0) = 2 * unit(2 * i) - 1;
    x(1) = 2 * unit(2 * i + 1) - 1;
    return x;
}
static KP tree() {
    return std::make_shared<SumKernel<double>>(std::make_shared<Matern52Kernel<double>>(0.8, 1.1),
                                               std::make_shared<GaussianKernel<double>>(1.5, 0.6));
}
static std::shared_ptr<G> make_gp(KP k, unsigned n, double sigma) {
    auto gp = std::make_shared<G>(k);
    gp->SetSigma(sigma);
    for (unsigned i = 0; i < n; i++) {
        G::VectorType x = point(i), y(1);
        y(0) = std::sin(3 * x(0)) + std::cos(2 * x(1));
        gp->AddSample(x, y);
    }
    return gp;
}

// in-place Cholesky solve of the dense system on the host (n = 150)
static std::vector<double> chol(std::vector<double> A, unsigned n) {
    for (unsigned j = 0; j < n; j++) {
        for (unsigned k = 0; k < j; k++)
            for (unsigned i = j; i < n; i++) A[i * n + j] -= A[i * n + k] * A[j * n + k];
        const double dj = std::sqrt(A[j * n + j]);
        for (unsigned i = j; i < n; i++) A[i * n + j] /= dj;
    }
    return A;
}
static std::vector<double> solve(const std::vector<double>& L, std::vector<double> b, unsigned n) {
    for (unsigned i = 0; i < n; i++) {
        for (unsigned k = 0; k < i; k++) b[i] -= L[i * n + k] * b[k];
        b[i] /= L[i * n + i];
    }
    for (unsigned ii = n; ii-- > 0;) {
        for (unsigned k = ii + 1; k < n; k++) b[ii] -= L[k * n + ii] * b[k];
        b[ii] /= L[ii * n + ii];
    }
    return b;
}

static void fit_predict_interval() {
    const unsigned n = 150;
    const double sigma = 0.4;
    KP k = tree();
    auto gp = make_gp(k, n, sigma);
    gp->Initialize();
    std::vector<double> A(n * n), y(n);
    for (unsigned i = 0; i < n; i++) {
        const G::VectorType xi = point(i);
        y[i] = std::sin(3 * xi(0)) + std::cos(2 * xi(1));
        for (unsigned j = 0; j < n; j++) A[i * n + j] = (*k)(xi, point(j)) + (i == j ? sigma * sigma : 0.0);
    }
    const std::vector<double> L = chol(A, n), alpha = solve(L, y, n);
    double dp = 0, sp = 0, dc = 0, sc = 0;
    for (unsigned q = 0; q < 16; q++) {
        const G::VectorType x = point(100000 + q);
        std::vector<double> kx(n);
        double mean = 0;
        for (unsigned j = 0; j < n; j++) {
            kx[j] = (*k)(x, point(j));
            mean += kx[j] * alpha[j];
        }
        const std::vector<double> w = solve(L, kx, n);
        double var = (*k)(x, x);
        for (unsigned j = 0; j < n; j++) var -= kx[j] * w[j];
        const double pm = gp->Predict(x)(0), ci = gp->GetCredibleInterval(x);
        dp = std::max(dp, std::fabs(pm - mean));
        sp = std::max(sp, std::fabs(mean));
        dc = std::max(dc, std::fabs(ci - 2 * std::sqrt(var)));
        sc = std::max(sc, 2 * std::sqrt(var));
    }
    check(dp <= 1e-9 * sp, "Predict differs from the host solve by " + num(dp / sp));
    check(dc <= 1e-7 * sc, "GetCredibleInterval differs from the host solve by " + num(dc / sc));
}

static void save_load_round_trip() {
    auto gp = make_gp(tree(), 150, 0.4);
    gp->Initialize();
    gp->Save("/tmp/gpr_amd_matern_test-");
    auto rd = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(1));
    rd->Load("/tmp/gpr_amd_matern_test-");
    check(*gp == *rd, "the loaded process compares equal");
    for (unsigned q = 0; q < 16; q++) {
        const G::VectorType x = point(100000 + q);
        const double a = gp->Predict(x)(0), b = rd->Predict(x)(0);
        check(std::fabs(a - b) <= 1e-12 * std::max(1.0, std::fabs(a)), "prediction after Load " + num(a) + " vs " + num(b));
        const double ca = gp->GetCredibleInterval(x), cb = rd->GetCredibleInterval(x);
        check(std::fabs(ca - cb) <= 1e-9 * std::max(1.0, ca), "credible interval after Load");
    }
}

static void likelihood_gradient() {
    KP k = tree();
    auto gp = make_gp(k, 150, 0.4);
    GaussianLogLikelihood<double> lik;
    auto vg = lik.GetValueAndParameterDerivatives(gp);
    check(std::isfinite(vg.first(0)), "likelihood not finite");
    check(vg.second.size() == 4, "four parameter derivatives");
    auto p = k->GetParameters();
    for (std::size_t i = 0; i < p.size(); i++) {
        const double h = 1e-5;
        auto pp = p, pm = p;
        pp[i] += h;
        pm[i] -= h;
        k->SetParameters(pp);
        gp->SetKernel(k);
        const double vp = lik(gp)(0);
        k->SetParameters(pm);
        gp->SetKernel(k);
        const double vm = lik(gp)(0);
        const double fd = (vp - vm) / (2 * h);
        check(std::fabs(fd - vg.second(i)) <= 1e-4 * std::max(1.0, std::fabs(fd)),
              "grad[" + num((double)i) + "] " + num(vg.second(i)) + " vs fd " + num(fd));
    }
}

int main() {
    run("FitPredictInterval", fit_predict_interval);
    run("SaveLoadRoundTrip", save_load_round_trip);
    run("LikelihoodGradient", likelihood_gradient);
    return g_fail;
}
