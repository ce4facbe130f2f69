// sample_test.cpp — the joint posterior and posterior sampling through the C++ host API:
// GaussianProcess<T>::GetPosterior and ::Sample (gprx_model_posterior, gprx_model_sample) against
// the values of the numpy restatement (tests/sample_ref.py), which tests/test_gpu_sample_host.py
// writes into the file given as the first argument.  `--no-device`: only that the class throws
// when no GPU is visible.  Prints one line per case; exit status = #failures.  Built by
// `make cpptests`.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gpr/GaussianProcess.h"
#include "gpr/Kernel.h"

using namespace gpr;

typedef GaussianProcess<double> G;

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

// the file: n d q nsamp seed sigma kernel_sigma kernel_scale / n rows of x_0 .. x_{d-1} y /
// q rows of xq_0 .. xq_{d-1} mean / q rows of Sigma (without the noise) / nsamp rows of a draw with
// the noise (q values)
struct Expected {
    unsigned n = 0, d = 0, q = 0, nsamp = 0;
    unsigned long long seed = 0;
    double sigma = 0, ksigma = 0, kscale = 0;
    std::vector<double> x, y, xq, mean, cov, draws;
};
static Expected read_expected(const std::string& path) {
    std::ifstream f(path.c_str());
    Expected e;
    if (!(f >> e.n >> e.d >> e.q >> e.nsamp >> e.seed >> e.sigma >> e.ksigma >> e.kscale))
        throw std::string("cannot read " + path);
    e.x.resize((size_t)e.n * e.d);
    e.y.resize(e.n);
    e.xq.resize((size_t)e.q * e.d);
    e.mean.resize(e.q);
    e.cov.resize((size_t)e.q * e.q);
    e.draws.resize((size_t)e.nsamp * e.q);
    for (unsigned i = 0; i < e.n; i++) {
        for (unsigned k = 0; k < e.d; k++) f >> e.x[(size_t)i * e.d + k];
        f >> e.y[i];
    }
    for (unsigned p = 0; p < e.q; p++) {
        for (unsigned k = 0; k < e.d; k++) f >> e.xq[(size_t)p * e.d + k];
        f >> e.mean[p];
    }
    for (double& v : e.cov) f >> v;
    for (double& v : e.draws) f >> v;
    if (!f) throw std::string("truncated " + path);
    return e;
}
static void add_sample(G& gp, const Expected& e, unsigned i) {
    G::VectorType x(e.d), y(1);
    for (unsigned k = 0; k < e.d; k++) x(k) = e.x[(size_t)i * e.d + k];
    y(0) = e.y[i];
    gp.AddSample(x, y);
}
static std::shared_ptr<G> make_gp(const Expected& e, unsigned n) {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(e.ksigma, e.kscale));
    gp->SetSigma(e.sigma);
    for (unsigned i = 0; i < n; i++) add_sample(*gp, e, i);
    return gp;
}
static std::vector<G::VectorType> queries(const Expected& e) {
    std::vector<G::VectorType> xs;
    for (unsigned p = 0; p < e.q; p++) {
        G::VectorType x(e.d);
        for (unsigned k = 0; k < e.d; k++) x(k) = e.xq[(size_t)p * e.d + k];
        xs.push_back(x);
    }
    return xs;
}
// normwise relative error of the first b.size() values at a against b
static double relerr(const double* a, const std::vector<double>& b) {
    double d = 0, s = 0;
    for (size_t i = 0; i < b.size(); i++) {
        d = std::max(d, std::fabs(a[i] - b[i]));
        s = std::max(s, std::fabs(b[i]));
    }
    return d / s;
}

static void check_posterior(G& gp, const Expected& e) {
    const std::vector<G::VectorType> xs = queries(e);
    G::MatrixType mean, cov, noisy;
    gp.GetPosterior(xs, mean, cov);
    check(mean.rows() == e.q && mean.cols() == 1 && cov.rows() == e.q && cov.cols() == e.q, "shapes");
    check(relerr(mean.data(), e.mean) <= 1e-6, "means differ by " + num(relerr(mean.data(), e.mean)));
    check(relerr(cov.data(), e.cov) <= 1e-6, "covariance differs by " + num(relerr(cov.data(), e.cov)));
    for (unsigned a = 0; a < e.q; a++)
        for (unsigned b = 0; b < a; b++) check(cov(a, b) == cov(b, a), "covariance is not symmetric");
    gp.GetPosterior(xs, mean, noisy, true);
    std::vector<double> want = e.cov;
    for (unsigned a = 0; a < e.q; a++) want[(size_t)a * e.q + a] += e.sigma * e.sigma;
    check(relerr(noisy.data(), want) <= 1e-6, "noisy covariance differs by " + num(relerr(noisy.data(), want)));
}

static void posterior(const Expected& e) {
    auto gp = make_gp(e, e.n);
    check_posterior(*gp, e);
    // the call read the fitted model: predictions are the same before and after
    const std::vector<G::VectorType> xs = queries(e);
    const double p0 = gp->Predict(xs[0])(0);
    G::MatrixType mean, cov;
    gp->GetPosterior(xs, mean, cov);
    gp->Sample(xs, 2, 1);
    check(gp->Predict(xs[0])(0) == p0, "Predict changed after GetPosterior and Sample");
}

static void sample(const Expected& e) {
    auto gp = make_gp(e, e.n);
    const std::vector<G::VectorType> xs = queries(e);
    const std::vector<G::MatrixType> draws = gp->Sample(xs, e.nsamp, e.seed, true);
    check(draws.size() == e.nsamp, "number of draws");
    std::vector<double> flat;
    for (const auto& m : draws) {
        check(m.rows() == e.q && m.cols() == 1, "shape of a draw");
        flat.insert(flat.end(), m.data(), m.data() + e.q);
    }
    check(relerr(flat.data(), e.draws) <= 1e-6, "draws differ by " + num(relerr(flat.data(), e.draws)));
    const std::vector<G::MatrixType> two = gp->Sample(xs, 2, e.seed, true);
    for (unsigned i = 0; i < 2 && i < e.nsamp; i++)
        for (unsigned p = 0; p < e.q; p++) check(two[i](p, 0) == draws[i](p, 0), "a draw depends on the number of draws");
    const std::vector<G::MatrixType> other = gp->Sample(xs, 2, e.seed + 1, true);
    check(other[0](0, 0) != draws[0](0, 0), "another seed gave the same draw");
    check(gp->Sample(xs, 0, e.seed).empty(), "zero draws");
}

// a sample added after the fit is part of the posterior (as LeaveOneOut: Initialize refits)
static void queued_sample(const Expected& e) {
    auto gp = make_gp(e, e.n - 1);
    gp->Initialize();
    add_sample(*gp, e, e.n - 1);
    check_posterior(*gp, e);
}

static void no_device() {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(1.0));
    G::VectorType x(1), y(1);
    x(0) = 1;
    y(0) = 2;
    gp->AddSample(x, y);
    const std::vector<G::VectorType> xs(1, x);
    bool threw = false;
    try {
        G::MatrixType mean, cov;
        gp->GetPosterior(xs, mean, cov);
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "GetPosterior without a GPU must throw");
    threw = false;
    try {
        gp->Sample(xs, 1, 0);
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "Sample without a GPU must throw");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--no-device") {
        run("NoDeviceFailsLoudly", no_device);
        return g_fail;
    }
    if (argc < 2) {
        std::printf("usage: sample_test <expected values file> | --no-device\n");
        return 2;
    }
    Expected e;
    run("ReadExpected", [&] { e = read_expected(argv[1]); });
    if (g_fail) return g_fail;
    run("GetPosterior", [&] { posterior(e); });
    run("Sample", [&] { sample(e); });
    run("QueuedSample", [&] { queued_sample(e); });
    return g_fail;
}
