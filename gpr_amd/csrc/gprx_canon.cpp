// gprx_canon.cpp — the canonical kernel form: a caller's post-order kernel tree lowered to the
// leaves, product terms and parameter layout the device kernels read (KCanon<T>).
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "gprx_internal.h"

namespace gprx {

static int leaf_nparams(int op) {
    switch (op) {
        case GPRX_K_GAUSSIAN:
        case GPRX_K_GAUSSIAN_EXP:
        case GPRX_K_MATERN32:
        case GPRX_K_MATERN52:
            return 2;
        case GPRX_K_WHITE:
            return 1;
        case GPRX_K_RATIONAL_QUADRATIC:
        case GPRX_K_PERIODIC:
            return 3;
    }
    return 0;
}

template <typename T>
std::string canonicalize(const gprx_kernel_desc& desc, KCanon<T>& K) {
    std::memset(&K, 0, sizeof(K));
    if (desc.n_nodes <= 0 || desc.n_nodes > GPRX_MAX_KNODES) return "kernel descriptor: bad node count";
    std::vector<std::vector<unsigned>> st;
    int nleaf = 0, nparams = 0, nper = 0;
    bool r2 = false;
    for (int i = 0; i < desc.n_nodes; i++) {
        const gprx_knode& nd = desc.node[i];
        const int op = nd.op;
        if (op == GPRX_K_SUM || op == GPRX_K_PRODUCT) {
            if (st.size() < 2) return "kernel descriptor: malformed post-order program";
            std::vector<unsigned> b = st.back();
            st.pop_back();
            std::vector<unsigned> a = st.back();
            st.pop_back();
            std::vector<unsigned> r;
            if (op == GPRX_K_SUM) {
                r = a;
                r.insert(r.end(), b.begin(), b.end());
            } else {
                for (unsigned ta : a)
                    for (unsigned tb : b) r.push_back(ta | tb);
            }
            if ((int)r.size() > MAX_TERM) return "kernel descriptor: too many product terms for the device form";
            st.push_back(r);
            continue;
        }
        const int np = leaf_nparams(op);
        if (np == 0) return "kernel descriptor: unknown node op";
        if (nleaf >= MAX_LEAF) return "kernel descriptor: too many leaf kernels for the device form";
        KLeaf<T>& L = K.leaf[nleaf];
        const T p0 = (T)nd.p[0], p1 = (T)nd.p[1], p2 = (T)nd.p[2];
        L.p[0] = p0;
        L.p[1] = p1;
        L.p[2] = p2;
        switch (op) {
            case GPRX_K_GAUSSIAN:  // include/Kernel.h:529-537
                if (p0 == T(0)) return "GaussianKernel: sigma has to be positive";
                if (p1 == T(0)) return "GaussianKernel: scale has to be positive";
                L.type = L_GAUSS;
                L.c0 = p1 * p1;
                L.c1 = T(-0.5) / (p0 * p0);
                r2 = true;
                break;
            case GPRX_K_GAUSSIAN_EXP: {
                const T es = std::exp(p1), eg = std::exp(p0);
                L.type = L_GAUSS_EXP;
                L.c0 = es * es;
                L.c1 = T(-0.5) / (eg * eg);
                r2 = true;
                break;
            }
            case GPRX_K_WHITE:
                L.type = L_WHITE;
                L.c0 = p0 * p0;
                r2 = true;
                break;
            case GPRX_K_RATIONAL_QUADRATIC:
                L.type = L_RQ;
                L.c0 = p0 * p0;
                L.c1 = T(0.5) / (p1 * p1 * p2);
                L.c2 = p2;
                r2 = true;
                break;
            case GPRX_K_PERIODIC:  // include/Kernel.h:1003-1005
                if (p0 == T(0)) return "PeriodicKernel: scale parameter has to be positive.";
                if (p1 == T(0)) return "PeriodicKernel: period length parameter has to be positive.";
                if (p2 == T(0)) return "PeriodicKernel: sigma parameter has to be positive.";
                if (nper >= MAX_PER) return "kernel descriptor: at most 2 periodic leaves on the device";
                L.type = L_PERIODIC;
                L.pslot = nper;
                K.b[nper] = p1;
                nper++;
                L.c0 = p0 * p0;
                L.c1 = T(-0.5) / (p2 * p2);
                break;
            case GPRX_K_MATERN32:  // c0 (1 + a) exp(-a), a = sqrt(c1 r2)
                if (p0 == T(0)) return "Matern32Kernel: sigma has to be positive";
                if (p1 == T(0)) return "Matern32Kernel: scale has to be positive";
                L.type = L_MATERN32;
                L.c0 = p1 * p1;
                L.c1 = T(3) / (p0 * p0);
                r2 = true;
                break;
            case GPRX_K_MATERN52:  // c0 (1 + a + a^2/3) exp(-a)
                if (p0 == T(0)) return "Matern52Kernel: sigma has to be positive";
                if (p1 == T(0)) return "Matern52Kernel: scale has to be positive";
                L.type = L_MATERN52;
                L.c0 = p1 * p1;
                L.c1 = T(5) / (p0 * p0);
                L.c2 = L.c0 / T(3);
                r2 = true;
                break;
        }
        // the folded exp constants (fexp_fold: f64 predict epilogue only)
        L.fold = 0;
        L.f1 = L.f0 = T(0);
        if (std::is_same<T, double>::value && (L.type == L_GAUSS || L.type == L_GAUSS_EXP || L.type == L_PERIODIC) &&
            L.c0 > T(0) && std::isfinite(std::log((double)L.c0))) {
            constexpr double kS = 92.33248261689366;  // 64 / ln 2
            L.f1 = (T)((double)L.c1 * kS);
            L.f0 = (T)(std::log((double)L.c0) * kS);
            L.fold = 1;
        }
        K.param_base[nleaf] = nparams;
        nparams += np;
        st.push_back(std::vector<unsigned>{1u << nleaf});
        nleaf++;
    }
    if (st.size() != 1) return "kernel descriptor: malformed post-order program";
    K.nleaf = nleaf;
    K.nterm = (int)st[0].size();
    K.sum_leaves = 1;
    for (int t = 0; t < K.nterm; t++) {
        K.term_mask[t] = st[0][t];
        if (st[0][t] != (1u << t)) K.sum_leaves = 0;
    }
    K.nper = nper;
    K.need_r2 = r2 ? 1 : 0;
    K.nparams = nparams;
    if (nparams > GPRX_MAX_KPARAMS) return "kernel descriptor: too many parameters";
    return "";
}
template std::string canonicalize<float>(const gprx_kernel_desc&, KCanon<float>&);
template std::string canonicalize<double>(const gprx_kernel_desc&, KCanon<double>&);

}  // namespace gprx
