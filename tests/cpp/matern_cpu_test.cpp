// matern_cpu_test.cpp — Matern32Kernel / Matern52Kernel of the host API on the CPU alone (no
// device): the KernelFactory round trip of a composite tree holding both, operator() against
// the closed form, GetDerivative against central differences at r = 0, small r and large r,
// and the parameter-count and zero-parameter errors.
// Prints one line per case; exit status = #failures.  Built by `make cpptests`; driven by
// tests/test_matern_cpu.py.
#include <cmath>
#include <cstdio>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "gpr/Kernel.h"

using namespace gpr;

typedef Kernel<double> K;
typedef K::VectorType V;

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
static V vec3(double a, double b, double c) {
    V v(3);
    v(0) = a;
    v(1) = b;
    v(2) = c;
    return v;
}
static bool throws(const std::function<void()>& f, const std::string& msg) {
    try {
        f();
    } catch (const std::string& e) {
        return e == msg;
    }
    return false;
}

static double closed(int nu2, double l, double s, double r) {
    const double a = std::sqrt((double)nu2) * r / std::fabs(l);
    return s * s * (nu2 == 3 ? 1 + a : 1 + a + a * a / 3) * std::exp(-a);
}

static void factory_round_trip() {
    K::Pointer k = std::make_shared<SumKernel<double>>(
        std::make_shared<ProductKernel<double>>(std::make_shared<Matern52Kernel<double>>(0.9, 1.1),
                                                std::make_shared<PeriodicKernel<double>>(0.8, 2.5, 0.7)),
        std::make_shared<Matern32Kernel<double>>(0.6, 1.2));
    const std::string str = k->ToString();
    check(str.find("Matern52Kernel(") != std::string::npos && str.find("Matern32Kernel(") != std::string::npos,
          "ToString " + str);
    std::string s = str;
    K::Pointer r = KernelFactory<double>::GetKernel(s);
    check(r->ToString() == str, "round trip " + r->ToString());
    check(*r == *k, "operator==");
    check(r->GetNumberOfParameters() == 7, "parameter count");
    const std::vector<double> want = {0.9, 1.1, 0.8, 2.5, 0.7, 0.6, 1.2};
    check(r->GetParameters() == want, "parameter order");
    const V x = vec3(0.1, -0.4, 0.7), y = vec3(-0.3, 0.2, 0.5);
    check((*r)(x, y) == (*k)(x, y), "value after the round trip");
    std::vector<gprx_knode> prog;
    r->Describe(prog);
    check(prog.size() == 5 && prog[0].op == GPRX_K_MATERN52 && prog[1].op == GPRX_K_PERIODIC &&
              prog[2].op == GPRX_K_PRODUCT && prog[3].op == GPRX_K_MATERN32 && prog[4].op == GPRX_K_SUM,
          "Describe program");
    check(prog[0].p[0] == 0.9 && prog[0].p[1] == 1.1 && prog[3].p[0] == 0.6 && prog[3].p[1] == 1.2, "Describe parameters");
    std::string one = "Matern32Kernel(0.5,)";
    check(throws([&] { KernelFactory<double>::GetKernel(one); }, "Matern32Kernel::Load: wrong number of kernel parameters."),
          "Load with one parameter");
    Matern52Kernel<double> fromstr("0.75", "1.5");
    check(fromstr.GetParameters() == std::vector<double>({0.75, 1.5}), "string constructor");
    check(Matern32Kernel<double>(0.5).GetParameters() == std::vector<double>({0.5, 1.0}), "default scale");
}

// (the two evaluations round a differently, sqrt(nu2 r^2) / |l| against sqrt(nu2) r / |l|: up to
// ~4 ulp in a, times |a k'(a)| <= 0.6 s^2, plus the roundings of the polynomial and the product:
// below 16 ulp = 4e-15 of s^2)
static void value_closed_form() {
    const V x = vec3(0.1, -0.4, 0.7);
    const double ls[] = {0.6, -0.6, 2.5}, ss[] = {1.2, -0.7};
    const double dirs[] = {0.0, 1e-9, 1e-3, 0.3, 2.0, 40.0};
    for (double l : ls)
        for (double s : ss)
            for (double t : dirs) {
                const V y = vec3(0.1 + t * 2.0 / 3, -0.4 - t / 3, 0.7 + t * 2.0 / 3);  // |x - y| = t
                const double r = (x - y).norm();
                const double v3 = Matern32Kernel<double>(l, s)(x, y), v5 = Matern52Kernel<double>(l, s)(x, y);
                check(std::fabs(v3 - closed(3, l, s, r)) <= 4e-15 * s * s, "3/2 value at r = " + num(r));
                check(std::fabs(v5 - closed(5, l, s, r)) <= 4e-15 * s * s, "5/2 value at r = " + num(r));
                if (t == 0.0) check(v3 == s * s && v5 == s * s, "k(x, x) = s^2");
            }
    check(Matern32Kernel<double>(0.6, 1.2)(x, x) == Matern32Kernel<double>(-0.6, 1.2)(x, x), "|sigma|");
}

// d/dsigma and d/dscale against central differences of operator() (h = 1e-6: truncation
// ~h^2 k''' / 6 and rounding ~1e-16 / h are both below 1e-9 at these O(1) parameters)
template <class KT>
static void derivative_case(double l, double s, double t) {
    const V x = vec3(0.1, -0.4, 0.7), y = vec3(0.1 + t * 2.0 / 3, -0.4 - t / 3, 0.7 + t * 2.0 / 3);
    const V D = KT(l, s).GetDerivative(x, y);
    check(D.size() == 2, "two derivatives");
    const double h = 1e-6;
    const double fl = (KT(l + h, s)(x, y) - KT(l - h, s)(x, y)) / (2 * h);
    const double fs = (KT(l, s + h)(x, y) - KT(l, s - h)(x, y)) / (2 * h);
    const double tol = 1e-8 * std::max(1.0, s * s);
    check(std::isfinite(D[0]) && std::isfinite(D[1]), "finite at r = " + num(t));
    check(std::fabs(D[0] - fl) <= tol, "d/dsigma " + num(D[0]) + " vs " + num(fl) + " at r = " + num(t));
    check(std::fabs(D[1] - fs) <= tol, "d/dscale " + num(D[1]) + " vs " + num(fs) + " at r = " + num(t));
    if (t == 0.0) check(D[0] == 0.0 && D[1] == 2 * s, "derivatives at r = 0");
}
static void derivative_central_differences() {
    const double ts[] = {0.0, 1e-7, 1e-3, 0.4, 3.0, 25.0};
    for (double t : ts) {
        derivative_case<Matern32Kernel<double>>(0.6, 1.2, t);
        derivative_case<Matern52Kernel<double>>(0.6, 1.2, t);
        derivative_case<Matern32Kernel<double>>(-0.8, 0.7, t);  // the sigma-derivative carries sigma's sign
        derivative_case<Matern52Kernel<double>>(-0.8, 0.7, t);
    }
    // composite: [k1 params, k2 params], the product rule
    auto a = std::make_shared<Matern32Kernel<double>>(0.6, 1.2);
    auto b = std::make_shared<GaussianKernel<double>>(0.9, 0.8);
    ProductKernel<double> p(a, b);
    const V x = vec3(0.1, -0.4, 0.7), y = vec3(-0.3, 0.2, 0.5);
    const V D = p.GetDerivative(x, y), Da = a->GetDerivative(x, y), Db = b->GetDerivative(x, y);
    check(D.size() == 4 && D[0] == Da[0] * (*b)(x, y) && D[3] == Db[1] * (*a)(x, y), "product rule");
}

static void parameter_errors() {
    Matern32Kernel<double> k3(0.6, 1.2);
    Matern52Kernel<double> k5(0.6, 1.2);
    check(k3.GetNumberOfParameters() == 2 && k5.GetNumberOfParameters() == 2, "two parameters");
    check(throws([&] { k3.SetParameters({1.0}); }, "Matern32Kernel::SetParameters: wrong number of parameters."),
          "3/2 SetParameters with one");
    check(throws([&] { k5.SetParameters({1.0, 2.0, 3.0}); }, "Matern52Kernel::SetParameters: wrong number of parameters."),
          "5/2 SetParameters with three");
    k3.SetParameters({0.7, 1.3});
    check(k3.GetParameters() == std::vector<double>({0.7, 1.3}), "SetParameters");
    check(k3.ToString() == "Matern32Kernel(0.7,1.3,)", "ToString " + k3.ToString());
    check(throws([] { Matern32Kernel<double> z(0.0, 1.0); }, "Matern32Kernel: sigma has to be positive"), "zero sigma");
    check(throws([] { Matern52Kernel<double> z(1.0, 0.0); }, "Matern52Kernel: scale has to be positive"), "zero scale");
    std::string s = "Matern52Kernel(0,1,)";
    check(throws([&] { KernelFactory<double>::GetKernel(s); }, "Matern52Kernel: sigma has to be positive"),
          "zero sigma through the factory");
}

int main() {
    run("FactoryRoundTrip", factory_round_trip);
    run("ValueClosedForm", value_closed_form);
    run("DerivativeCentralDifferences", derivative_central_differences);
    run("ParameterErrors", parameter_errors);
    return g_fail;
}
