// sparse_reuse_test.cpp — two SparseGaussianProcess<double> one after the other in one process.
// Both run on DefaultContext(), so the second meets the sparse state the first left in it: here
// fewer inducing points on the same 128-padded layout (140, then 130), where the streamed block
// still holds the first one's rows.  Each is checked for Predict at its query points and for
// operator() at its pairs against the oracle's values, which tests/test_gpu_sparse_reuse_host.py
// writes into the file given as the first argument.
// Prints one line per case; exit status = #failures.  Built by `make cpptests`.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gpr/Kernel.h"
#include "gpr/SparseGaussianProcess.h"

using namespace gpr;

typedef SparseGaussianProcess<double> S;

static int g_fail = 0;
static void run(const std::string& name, const std::function<void()>& f) {
    try {
        f();
        std::printf("PASS %s\n", name.c_str());
    } catch (const std::string& s) {
        std::printf("FAIL %s: %s\n", name.c_str(), s.c_str());
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

// the file: the number of processes, then per process
//   n d M q sigma jitter kernel_sigma kernel_scale
//   n rows of x_0 .. x_{d-1} y, M rows of the same for the inducing points,
//   q rows of a_0 .. a_{d-1} b_0 .. b_{d-1} mean(a) cov(a, b)
struct Expected {
    unsigned n = 0, d = 0, M = 0, q = 0;
    double sigma = 0, jitter = 0, ksigma = 0, kscale = 0;
    std::vector<double> x, y, xm, ym, a, b, mean, cov;
};
static void read_rows(std::ifstream& f, unsigned rows, unsigned d, std::vector<double>& x, std::vector<double>& y) {
    x.resize((size_t)rows * d);
    y.resize(rows);
    for (unsigned i = 0; i < rows; i++) {
        for (unsigned k = 0; k < d; k++) f >> x[(size_t)i * d + k];
        f >> y[i];
    }
}
static std::vector<Expected> read_expected(const std::string& path) {
    std::ifstream f(path.c_str());
    unsigned count = 0;
    if (!(f >> count) || count == 0 || count > 16) throw std::string("cannot read " + path);
    std::vector<Expected> out(count);
    for (Expected& e : out) {
        if (!(f >> e.n >> e.d >> e.M >> e.q >> e.sigma >> e.jitter >> e.ksigma >> e.kscale))
            throw std::string("cannot read a header of " + path);
        read_rows(f, e.n, e.d, e.x, e.y);
        read_rows(f, e.M, e.d, e.xm, e.ym);
        e.a.resize((size_t)e.q * e.d);
        e.b.resize((size_t)e.q * e.d);
        e.mean.resize(e.q);
        e.cov.resize(e.q);
        for (unsigned i = 0; i < e.q; i++) {
            for (unsigned k = 0; k < e.d; k++) f >> e.a[(size_t)i * e.d + k];
            for (unsigned k = 0; k < e.d; k++) f >> e.b[(size_t)i * e.d + k];
            f >> e.mean[i] >> e.cov[i];
        }
        if (!f) throw std::string("truncated " + path);
    }
    return out;
}
static S::VectorType row(const std::vector<double>& x, unsigned i, unsigned d) {
    S::VectorType v(d);
    for (unsigned k = 0; k < d; k++) v(k) = x[(size_t)i * d + k];
    return v;
}
// normwise error of a against b, relative to max(floor, |b|)
static double relerr(const std::vector<double>& a, const std::vector<double>& b, double floor) {
    double d = 0, s = floor;
    for (size_t i = 0; i < b.size(); i++) {
        d = std::max(d, std::fabs(a[i] - b[i]));
        s = std::max(s, std::fabs(b[i]));
    }
    return d / s;
}

static void sparse_process(const Expected& e) {
    S gp(std::make_shared<GaussianKernel<double>>(e.ksigma, e.kscale), e.jitter);
    gp.SetSigma(e.sigma);
    S::VectorType y(1);
    for (unsigned i = 0; i < e.n; i++) {
        y(0) = e.y[i];
        gp.AddSample(row(e.x, i, e.d), y);
    }
    for (unsigned i = 0; i < e.M; i++) {
        y(0) = e.ym[i];
        gp.AddInducingSample(row(e.xm, i, e.d), y);
    }
    check(gp.GetNumberOfInducingSamples() == e.M, "inducing samples");
    gp.Initialize();
    std::vector<double> mean(e.q), cov(e.q);
    for (unsigned i = 0; i < e.q; i++) {
        mean[i] = gp.Predict(row(e.a, i, e.d))(0);
        cov[i] = gp(row(e.a, i, e.d), row(e.b, i, e.d));
    }
    check(relerr(mean, e.mean, 1e-300) <= 1e-6, "predictions differ by " + num(relerr(mean, e.mean, 1e-300)));
    // (the prior variance is kscale^2 >= 1: the posterior covariances are measured against it)
    check(relerr(cov, e.cov, 1.0) <= 1e-6, "operator() differs by " + num(relerr(cov, e.cov, 1.0)));
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: sparse_reuse_test <expected values file>\n");
        return 2;
    }
    std::vector<Expected> all;
    run("ReadExpected", [&] { all = read_expected(argv[1]); });
    if (g_fail) return g_fail;
    for (const Expected& e : all) run("Sparse" + std::to_string(e.M), [&] { sparse_process(e); });
    return g_fail;
}
