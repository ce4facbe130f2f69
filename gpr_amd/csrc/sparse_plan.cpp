// sparse_plan.cpp — the clearing plan of the sparse GP's streamed block (sparse_plan.h).
#include "sparse_plan.h"

#include <algorithm>

namespace gprx {

int sparse_clear_plan(SparseBlock& st, int64_t id, int64_t ld, int64_t cols, int64_t Mp, int64_t M, int64_t nc,
                      ClearRect* out) {
    int k = 0;
    const int64_t ncp = (nc + 15) / 16 * 16;
    if (st.id != id || st.ld != ld || st.cols != cols || st.Mp != Mp) {  // a new block layout: zero it whole
        out[k++] = ClearRect{0, ld, 0, cols};
        st.id = id;
        st.ld = ld;
        st.cols = cols;
        st.Mp = Mp;
        st.zero = 0;
        st.rows = 0;
    }
    // columns [nc, cols) must be zero for this chunk's products (the split-K slices overhang the
    // data): zero what an earlier, longer chunk left there; this chunk dirties [0, ncp)
    if (st.zero > nc) {
        out[k++] = ClearRect{0, ld, nc, st.zero - nc};
        st.zero = nc;
    }
    // rows [M, Mp) must be zero too (the products read whole tiles of rows): zero what an earlier
    // call with more inducing points left there, over the columns that can still hold anything
    if (st.rows > M) {
        if (st.zero > 0) out[k++] = ClearRect{M, st.rows - M, 0, st.zero};
        st.rows = M;
    }
    st.rows = std::max(st.rows, M);
    st.zero = std::max(st.zero, ncp);
    return k;
}

}  // namespace gprx
