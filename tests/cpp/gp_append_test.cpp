// gp_append_test.cpp — GaussianProcess<T>::Update(): a GP that only grew since its last device
// fit extends that fit's Cholesky factor (gprx_model_append) instead of refitting.  Every case
// compares with a second GaussianProcess given all the samples and a plain Initialize().
// Prints one line per case; exit status = #failures.  Built by `make cpptests`; driven by
// tests/test_gpu_append_host.py (-m gpu).
#include <cmath>
#include <cstdio>
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
    s << v;
    return s.str();
}

// deterministic samples: x_i in [-1, 1]^2 from a 64-bit mixer, y = sin(3 x0) + cos(2 x1)
static double unit(unsigned long long i) {
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static void sample(unsigned i, G::VectorType& x, G::VectorType& y) {
    x = G::VectorType(2);
    y = G::VectorType(1);
    x(0) = 2 * unit(2 * i) - 1;
    x(1) = 2 * unit(2 * i + 1) - 1;
    y(0) = std::sin(3 * x(0)) + std::cos(2 * x(1));
}
static void add(G& gp, unsigned i0, unsigned i1) {
    for (unsigned i = i0; i < i1; i++) {
        G::VectorType x, y;
        sample(i, x, y);
        gp.AddSample(x, y);
    }
}
static std::shared_ptr<G> fresh(double sigma, double scale, unsigned n) {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(0.7, scale));
    gp->SetSigma(sigma);
    add(*gp, 0, n);
    gp->Initialize();
    return gp;
}
// predictions and credible intervals of a and b at 16 queries agree to 1e-6 relative
static void same(G& a, G& b, const std::string& what) {
    check(a.GetNumberOfSamples() == b.GetNumberOfSamples(), what + ": sample counts differ");
    double dp = 0, sp = 0, dc = 0, sc = 0;
    for (unsigned q = 0; q < 16; q++) {
        G::VectorType x(2);
        x(0) = 2 * unit(100000 + 2 * q) - 1;
        x(1) = 2 * unit(100001 + 2 * q) - 1;
        const double pa = a.Predict(x)(0), pb = b.Predict(x)(0);
        const double ca = a.GetCredibleInterval(x), cb = b.GetCredibleInterval(x);
        dp = std::max(dp, std::fabs(pa - pb));
        sp = std::max(sp, std::fabs(pb));
        dc = std::max(dc, std::fabs(ca - cb));
        sc = std::max(sc, std::fabs(cb));
    }
    check(dp <= 1e-6 * sp, what + ": predictions differ by " + num(dp / sp));
    check(dc <= 1e-6 * sc, what + ": credible intervals differ by " + num(dc / sc));
}

// 200 samples and Initialize(), then 10 x (AddSample; Update(); Predict)
static void append_matches_refit() {
    auto gp = fresh(0.5, 1.3, 200);
    for (unsigned step = 0; step < 10; step++) {
        add(*gp, 200 + step, 201 + step);
        gp->Update();
        auto ref = fresh(0.5, 1.3, 201 + step);
        same(*gp, *ref, "step " + num(step));
    }
}

// several samples between two updates, across the 256 block boundary
static void append_several() {
    auto gp = fresh(0.5, 1.3, 250);
    add(*gp, 250, 270);
    gp->Update();
    auto ref = fresh(0.5, 1.3, 270);
    same(*gp, *ref, "20 samples");
}

static void update_after_set_sigma() {
    auto gp = fresh(0.5, 1.3, 200);
    add(*gp, 200, 203);
    gp->SetSigma(0.3);
    gp->Update();
    auto ref = fresh(0.3, 1.3, 203);
    same(*gp, *ref, "SetSigma");
}

static void update_after_set_kernel() {
    auto gp = fresh(0.5, 1.3, 200);
    add(*gp, 200, 203);
    gp->SetKernel(std::make_shared<GaussianKernel<double>>(0.7, 0.9));
    gp->Update();
    auto ref = fresh(0.5, 0.9, 203);
    same(*gp, *ref, "SetKernel");
    // and the factor made by that refit is extended again
    add(*gp, 203, 205);
    gp->Update();
    auto ref2 = fresh(0.5, 0.9, 205);
    same(*gp, *ref2, "SetKernel, then append");
}

static void update_before_initialize() {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(0.7, 1.3));
    gp->SetSigma(0.5);
    add(*gp, 0, 150);
    gp->Update();
    auto ref = fresh(0.5, 1.3, 150);
    same(*gp, *ref, "first Update");
}

// a plain Initialize() after AddSample still sees all the data, also after an Update()
static void initialize_after_add_sample() {
    auto gp = fresh(0.5, 1.3, 200);
    add(*gp, 200, 204);
    gp->Initialize();
    auto ref = fresh(0.5, 1.3, 204);
    same(*gp, *ref, "Initialize after AddSample");
    add(*gp, 204, 205);
    gp->Update();
    add(*gp, 205, 207);
    gp->Initialize();
    auto ref2 = fresh(0.5, 1.3, 207);
    same(*gp, *ref2, "Initialize after Update");
}

int main() {
    run("UpdateMatchesRefit", append_matches_refit);
    run("UpdateSeveralSamples", append_several);
    run("UpdateAfterSetSigma", update_after_set_sigma);
    run("UpdateAfterSetKernel", update_after_set_kernel);
    run("UpdateBeforeInitialize", update_before_initialize);
    run("InitializeAfterAddSample", initialize_after_add_sample);
    return g_fail;
}
