// ard_test.cpp — per-dimension length scales through the C++ host API:
// GaussianProcess<T>::SetLengthScales / GetLengthScales and
// GaussianLogLikelihood<T>::GetLengthScaleDerivatives (gprx_model_set_length_scales,
// gprx_model_lml_scale_grad) against what the Python binding returned for the same model, which
// tests/test_gpu_ard_host.py writes into the file given as the first argument.
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
#include "gpr/Kernel.h"
#include "gpr/Likelihood.h"

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

// the file: n d q sigma kernel_sigma kernel_scale / ell (d) / grad_ell (d) / n rows of x y /
// q rows of xq mean
struct Expected {
    unsigned n = 0, d = 0, q = 0;
    double sigma = 0, ksigma = 0, kscale = 0;
    std::vector<double> ell, grad, x, y, xq, mean;
};
static Expected read_expected(const std::string& path) {
    std::ifstream f(path.c_str());
    Expected e;
    if (!(f >> e.n >> e.d >> e.q >> e.sigma >> e.ksigma >> e.kscale)) throw std::string("cannot read " + path);
    e.ell.resize(e.d);
    e.grad.resize(e.d);
    for (auto& v : e.ell) f >> v;
    for (auto& v : e.grad) f >> v;
    e.x.resize((size_t)e.n * e.d);
    e.y.resize(e.n);
    for (unsigned i = 0; i < e.n; i++) {
        for (unsigned k = 0; k < e.d; k++) f >> e.x[(size_t)i * e.d + k];
        f >> e.y[i];
    }
    e.xq.resize((size_t)e.q * e.d);
    e.mean.resize(e.q);
    for (unsigned i = 0; i < e.q; i++) {
        for (unsigned k = 0; k < e.d; k++) f >> e.xq[(size_t)i * e.d + k];
        f >> e.mean[i];
    }
    if (!f) throw std::string("truncated " + path);
    return e;
}
static std::shared_ptr<G> make_gp(const Expected& e, bool scales) {
    auto gp = std::make_shared<G>(std::make_shared<GaussianKernel<double>>(e.ksigma, e.kscale));
    gp->SetSigma(e.sigma);
    for (unsigned i = 0; i < e.n; i++) {
        G::VectorType x(e.d), y(1);
        for (unsigned k = 0; k < e.d; k++) x(k) = e.x[(size_t)i * e.d + k];
        y(0) = e.y[i];
        gp->AddSample(x, y);
    }
    if (scales) {
        G::VectorType ell(e.d);
        for (unsigned k = 0; k < e.d; k++) ell(k) = e.ell[k];
        gp->SetLengthScales(ell);
    }
    return gp;
}
template <class A>
static double relerr(const A& a, const std::vector<double>& b) {
    double d = 0, s = 0;
    for (size_t i = 0; i < b.size(); i++) {
        d = std::max(d, std::fabs((double)a[i] - b[i]));
        s = std::max(s, std::fabs(b[i]));
    }
    return d / s;
}
static std::vector<double> predict_all(G& gp, const Expected& e) {
    std::vector<double> out(e.q);
    for (unsigned i = 0; i < e.q; i++) {
        G::VectorType x(e.d);
        for (unsigned k = 0; k < e.d; k++) x(k) = e.xq[(size_t)i * e.d + k];
        out[i] = gp.Predict(x)(0);
    }
    return out;
}

static void set_get_predict(const Expected& e) {
    auto gp = make_gp(e, true);
    check(gp->GetLengthScales().size() == e.d, "GetLengthScales size");
    for (unsigned k = 0; k < e.d; k++) check(gp->GetLengthScales()[k] == e.ell[k], "GetLengthScales value");
    gp->Initialize();
    // the same library, data and arithmetic as the Python model; one query per call here, all at once there
    const std::vector<double> p = predict_all(*gp, e);
    check(relerr(p, e.mean) <= 1e-10, "Predict differs from the Python model's by " + num(relerr(p, e.mean)));
    // cleared: another model
    gp->SetLengthScales(G::VectorType(0));
    check(gp->GetLengthScales().size() == 0, "cleared scales");
    gp->Initialize();
    const std::vector<double> p0 = predict_all(*gp, e);
    check(relerr(p0, e.mean) > 1e-3, "clearing the length scales did not change the predictions");
    auto plain = make_gp(e, false);
    plain->Initialize();
    const std::vector<double> p1 = predict_all(*plain, e);
    for (unsigned i = 0; i < e.q; i++) check(p0[i] == p1[i], "cleared scales differ from a GP that never had any");
}

static void derivatives(const Expected& e) {
    auto gp = make_gp(e, true);
    GaussianLogLikelihood<double> lh;
    auto g = lh.GetLengthScaleDerivatives(gp);
    check(g.size() == e.d, "gradient size");
    // (fitted by this call with the inverse riding along; the Python model formed it from the factor)
    check(relerr(g, e.grad) <= 1e-9, "gradient differs from lml_scale_grad by " + num(relerr(g, e.grad)));
    // the likelihood's own value and parameter gradient still work on the same gp
    check(lh.GetValueAndParameterDerivatives(gp).second.size() == 2, "parameter gradient size");
    bool threw = false;
    try {
        lh.GetLengthScaleDerivatives(make_gp(e, false));
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "GetLengthScaleDerivatives without length scales must throw");
}

static void refusals(const Expected& e) {
    auto gp = make_gp(e, true);
    gp->Initialize();
    bool threw = false;
    try {
        gp->Save("/nonexistent-directory/ard");
    } catch (const std::string& s) {
        threw = s.find("length scales") != std::string::npos;
    }
    check(threw, "Save must refuse a GP with length scales");
    G::VectorType bad(e.d + 1);
    for (unsigned k = 0; k < e.d + 1; k++) bad(k) = 1.0;
    gp->SetLengthScales(bad);
    threw = false;
    try {
        gp->Initialize();
    } catch (const std::string&) {
        threw = true;
    }
    check(threw, "a wrong number of length scales must throw");
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: ard_test <expected values file>\n");
        return 2;
    }
    Expected e;
    run("ReadExpected", [&] { e = read_expected(argv[1]); });
    if (g_fail) return g_fail;
    run("SetGetPredict", [&] { set_get_predict(e); });
    run("LengthScaleDerivatives", [&] { derivatives(e); });
    run("Refusals", [&] { refusals(e); });
    return g_fail;
}
