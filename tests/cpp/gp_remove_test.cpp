// gp_remove_test.cpp — GaussianProcess<T>::RemoveSample() + Update(): a GP whose samples were
// removed and added since its last device fit updates that fit's Cholesky factor
// (gprx_model_remove, then gprx_model_append) instead of refitting.  Every case compares with a
// second GaussianProcess given the remaining samples and a plain Initialize().
// Prints one line per case; exit status = #failures.  Built by `make cpptests`; driven by
// tests/test_gpu_remove_host.py (-m gpu).
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

// deterministic samples (as tests/cpp/gp_append_test.cpp): x_i in [-1, 1]^2, y = sin(3 x0) + cos(2 x1)
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
static void add(G& gp, unsigned i) {
    G::VectorType x, y;
    sample(i, x, y);
    gp.AddSample(x, y);
}
static std::vector<unsigned> range(unsigned i0, unsigned i1) {
    std::vector<unsigned> v;
    for (unsigned i = i0; i < i1; i++) v.push_back(i);
    return v;
}
// a GP of the samples `ids`, Initialize()d
static std::shared_ptr<G> fresh(double sigma, double scale, const std::vector<unsigned>& ids) {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(0.7, scale));
    gp->SetSigma(sigma);
    for (unsigned i : ids) add(*gp, i);
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

// 200 samples and Initialize(), then 6 x (RemoveSample(0); AddSample; Update(); Predict)
static void sliding_window() {
    std::vector<unsigned> ids = range(0, 200);
    auto gp = fresh(0.5, 1.3, ids);
    for (unsigned step = 0; step < 6; step++) {
        gp->RemoveSample(0);
        ids.erase(ids.begin());
        add(*gp, 200 + step);
        ids.push_back(200 + step);
        gp->Update();
        auto ref = fresh(0.5, 1.3, ids);
        same(*gp, *ref, "step " + num(step));
    }
}

// removals only, in the middle and at the end, several between two updates
static void remove_only() {
    std::vector<unsigned> ids = range(0, 260);
    auto gp = fresh(0.5, 1.3, ids);
    for (unsigned at : {50u, 257u, 130u}) {
        gp->RemoveSample(at);
        ids.erase(ids.begin() + at);
    }
    gp->Update();
    auto ref = fresh(0.5, 1.3, ids);
    same(*gp, *ref, "three removals");
}

// a sample that never reached the device is only erased from the lists
static void remove_not_yet_uploaded() {
    std::vector<unsigned> ids = range(0, 200);
    auto gp = fresh(0.5, 1.3, ids);
    for (unsigned i = 200; i < 203; i++) {
        add(*gp, i);
        ids.push_back(i);
    }
    gp->RemoveSample(201);
    ids.erase(ids.begin() + 201);
    gp->RemoveSample(7);  // (and one that did)
    ids.erase(ids.begin() + 7);
    gp->Update();
    auto ref = fresh(0.5, 1.3, ids);
    same(*gp, *ref, "removed before upload");
    bool threw = false;
    try {
        gp->RemoveSample(ids.size());
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "RemoveSample past the end did not throw");
}

// a kernel change in between: the factor's provenance no longer holds, Update() reinitialises
static void remove_after_set_kernel() {
    std::vector<unsigned> ids = range(0, 200);
    auto gp = fresh(0.5, 1.3, ids);
    gp->RemoveSample(0);
    ids.erase(ids.begin());
    gp->SetKernel(std::make_shared<GaussianKernel<double>>(0.7, 0.9));
    gp->Update();
    auto ref = fresh(0.5, 0.9, ids);
    same(*gp, *ref, "SetKernel");
    // and the factor made by that refit is updated again
    gp->RemoveSample(10);
    ids.erase(ids.begin() + 10);
    gp->Update();
    auto ref2 = fresh(0.5, 0.9, ids);
    same(*gp, *ref2, "SetKernel, then remove");
}

// a plain Initialize() after RemoveSample + AddSample (the sample count is the device's again)
static void initialize_after_remove() {
    std::vector<unsigned> ids = range(0, 200);
    auto gp = fresh(0.5, 1.3, ids);
    gp->RemoveSample(3);
    ids.erase(ids.begin() + 3);
    add(*gp, 200);
    ids.push_back(200);
    gp->Initialize();
    auto ref = fresh(0.5, 1.3, ids);
    same(*gp, *ref, "Initialize after RemoveSample");
    gp->RemoveSample(0);
    ids.erase(ids.begin());
    gp->Update();
    auto ref2 = fresh(0.5, 1.3, ids);
    same(*gp, *ref2, "Update after that");
}

int main() {
    run("SlidingWindow", sliding_window);
    run("RemoveOnly", remove_only);
    run("RemoveNotYetUploaded", remove_not_yet_uploaded);
    run("RemoveAfterSetKernel", remove_after_set_kernel);
    run("InitializeAfterRemove", initialize_after_remove);
    return g_fail;
}
