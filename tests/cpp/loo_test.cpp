// loo_test.cpp — leave-one-out cross-validation through the C++ host API:
// GaussianProcess<T>::LeaveOneOut and LeaveOneOutLogLikelihood<T> (gprx_model_loo) against the
// values of the numpy restatement (tests/loo_ref.py), which tests/test_gpu_loo_host.py writes
// into the file given as the first argument, and GaussianProcessInference::Optimize maximising
// the leave-one-out value.  `--no-device`: only that the class throws when no GPU is visible.
// Prints one line per case; exit status = #failures.  Built by `make cpptests`.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gpr/GaussianProcess.h"
#include "gpr/GaussianProcessInference.h"
#include "gpr/Kernel.h"
#include "gpr/Likelihood.h"

using namespace gpr;

typedef GaussianProcess<double> G;
typedef LeaveOneOutLogLikelihood<double> LooType;

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
    s.precision(17);
    s << v;
    return s.str();
}

// the file: n d sigma kernel_sigma kernel_scale / value / g0 g1 / n rows of x_0 .. x_{d-1} y mu s2
struct Expected {
    unsigned n = 0, d = 0;
    double sigma = 0, ksigma = 0, kscale = 0, value = 0, g[2] = {0, 0};
    std::vector<double> x, y, mu, s2;
};
static Expected read_expected(const std::string& path) {
    std::ifstream f(path.c_str());
    Expected e;
    if (!(f >> e.n >> e.d >> e.sigma >> e.ksigma >> e.kscale >> e.value >> e.g[0] >> e.g[1]))
        throw std::string("cannot read " + path);
    e.x.resize((size_t)e.n * e.d);
    e.y.resize(e.n);
    e.mu.resize(e.n);
    e.s2.resize(e.n);
    for (unsigned i = 0; i < e.n; i++) {
        for (unsigned k = 0; k < e.d; k++) f >> e.x[(size_t)i * e.d + k];
        f >> e.y[i] >> e.mu[i] >> e.s2[i];
    }
    if (!f) throw std::string("truncated " + path);
    return e;
}
static std::shared_ptr<G> make_gp(const Expected& e) {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(e.ksigma, e.kscale));
    gp->SetSigma(e.sigma);
    for (unsigned i = 0; i < e.n; i++) {
        G::VectorType x(e.d), y(1);
        for (unsigned k = 0; k < e.d; k++) x(k) = e.x[(size_t)i * e.d + k];
        y(0) = e.y[i];
        gp->AddSample(x, y);
    }
    return gp;
}
// normwise relative error of a against b
template <class A>
static double relerr(const A& a, const std::vector<double>& b) {
    double d = 0, s = 0;
    for (size_t i = 0; i < b.size(); i++) {
        d = std::max(d, std::fabs((double)a[i] - b[i]));
        s = std::max(s, std::fabs(b[i]));
    }
    return d / s;
}

static void means_and_variances(const Expected& e) {
    auto gp = make_gp(e);
    gp->Initialize();
    G::MatrixType mean;
    G::VectorType var;
    const double v = gp->LeaveOneOut(mean, var);
    check(mean.rows() == e.n && mean.cols() == 1 && var.size() == e.n, "shapes");
    std::vector<double> mu(e.n);
    for (unsigned i = 0; i < e.n; i++) mu[i] = mean(i, 0);
    check(relerr(mu, e.mu) <= 1e-6, "means differ by " + num(relerr(mu, e.mu)));
    check(relerr(var, e.s2) <= 1e-6, "variances differ by " + num(relerr(var, e.s2)));
    check(std::fabs(v - e.value) <= 1e-6 * std::max(1.0, std::fabs(e.value)), "value " + num(v) + " vs " + num(e.value));
    // the call read the fitted model: predictions are the same before and after
    G::VectorType x(e.d);
    for (unsigned k = 0; k < e.d; k++) x(k) = 0.1 * (k + 1);
    const double p0 = gp->Predict(x)(0);
    gp->LeaveOneOut(mean, var);
    check(gp->Predict(x)(0) == p0, "Predict changed after LeaveOneOut");
}

static void likelihood(const Expected& e) {
    auto gp = make_gp(e);
    auto lh = std::make_shared<LooType>();
    const double v = (*lh)(gp)[0];
    check(std::fabs(v - e.value) <= 1e-6 * std::max(1.0, std::fabs(e.value)), "value " + num(v) + " vs " + num(e.value));
    auto vd = lh->GetValueAndParameterDerivatives(gp);
    // (with the gradient diag(C) is read from C, without it summed from V: not the same bits)
    check(std::fabs(vd.first[0] - e.value) <= 1e-6 * std::max(1.0, std::fabs(e.value)),
          "value with the gradient " + num(vd.first[0]) + " vs " + num(e.value));
    check(vd.second.size() == 2, "gradient size");
    const std::vector<double> g = {e.g[0], e.g[1]};
    check(relerr(vd.second, g) <= 1e-6, "gradient differs by " + num(relerr(vd.second, g)));
    auto g2 = lh->GetParameterDerivatives(gp);
    check(g2[0] == vd.second[0] && g2[1] == vd.second[1], "GetParameterDerivatives differs");
    check(lh->ToString() == "LeaveOneOutLogLikelihood", "ToString");
}

// deterministic samples (as tests/cpp/gp_remove_test.cpp): x_i in [-1, 1]^2, y = sin(3 x0) + cos(2 x1)
static double unit(unsigned long long i) {
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// two Optimize steps (step width 0.01: in numpy the value goes -30.700 -> -30.607 -> -30.539)
static void optimize() {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(0.7, 1.3));
    gp->SetSigma(0.5);
    for (unsigned i = 0; i < 100; i++) {
        G::VectorType x(2), y(1);
        x(0) = 2 * unit(2 * i) - 1;
        x(1) = 2 * unit(2 * i + 1) - 1;
        y(0) = std::sin(3 * x(0)) + std::cos(2 * x(1));
        gp->AddSample(x, y);
    }
    Likelihood<double>::Pointer lh = std::make_shared<LooType>();
    GaussianProcessInference<double> gpi(lh, gp, 0.01, 1);
    double v = (*lh)(gp)[0];
    check(std::fabs(v - -30.700283886660333) <= 1e-6 * 30.7, "start value " + num(v));
    for (int step = 0; step < 2; step++) {
        gpi.Optimize(false);
        gp->GetKernel()->SetParameters(gpi.GetParameters());
        const double v1 = (*lh)(gp)[0];
        check(v1 >= v, "step " + num(step) + " decreased the value: " + num(v) + " -> " + num(v1));
        v = v1;
    }
    check(v > -30.6, "two steps reached only " + num(v));
}

static void no_device() {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(1.0));
    G::VectorType x(1), y(1);
    x(0) = 1;
    y(0) = 2;
    gp->AddSample(x, y);
    bool threw = false;
    try {
        LooType lh;
        lh(gp);
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "LeaveOneOutLogLikelihood without a GPU must throw");
    threw = false;
    try {
        G::MatrixType mean;
        G::VectorType var;
        gp->LeaveOneOut(mean, var);
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "LeaveOneOut without a GPU must throw");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--no-device") {
        run("NoDeviceFailsLoudly", no_device);
        return g_fail;
    }
    if (argc < 2) {
        std::printf("usage: loo_test <expected values file> | --no-device\n");
        return 2;
    }
    Expected e;
    run("ReadExpected", [&] { e = read_expected(argv[1]); });
    if (g_fail) return g_fail;
    run("LeaveOneOut", [&] { means_and_variances(e); });
    run("LeaveOneOutLogLikelihood", [&] { likelihood(e); });
    run("OptimizeLeaveOneOut", optimize);
    return g_fail;
}
