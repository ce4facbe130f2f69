// sparse_plan.h — the clearing plan of the sparse GP's streamed block (sparse_plan.cpp): which
// rectangles of the block must be zeroed before a chunk is built into it.
//
// Plain host C++ with standard headers only: state in, rectangles out, no HIP call.
// sparse_normal_eq (gprx_sparse.cpp) issues the memsets it returns; gprx_dev_sparse_clear_plan
// (include/gprx_dev.h) exports it, so the rule is replayed on a host without a GPU
// (tests/test_sparse_reuse_cpu.py).
#pragma once

#include <cstdint>

namespace gprx {

// What is known about the streamed block (column-major, ld x cols; rows [0, Mp) the Kmn rows of
// the inducing points, rows [Mp, ld) the label rows) between calls.  Everything outside
//   rows [0, rows) x columns [0, zero)   and   rows [Mp, ld) x columns [0, zero)
// holds zeros.  A chunk's build stores rows [0, M) x columns [0, nc) and nothing else; its label
// rows (when it has any) store rows [Mp, ld) x columns [0, round_up(nc, 16)) whole.
struct SparseBlock {
    int64_t id = 0;    // the allocation (its address): a new one holds anything
    int64_t ld = 0, cols = 0, Mp = 0;
    int64_t zero = 0;  // columns from here on hold zeros in every row
    int64_t rows = 0;  // rows [rows, Mp) hold zeros in every column
};

struct ClearRect {  // rows [row0, row0 + nrows) x columns [col0, col0 + ncols)
    int64_t row0, nrows, col0, ncols;
};

constexpr int SPARSE_CLEAR_MAX = 3;

// The rectangles to zero before the chunk of nc dense rows (of a call with M inducing points on
// the block id, ld x cols, Mp) is built, at most SPARSE_CLEAR_MAX into out; st becomes the state
// after the chunk's stores.  Afterwards every element of the block that this chunk does not store
// is zero in rows [M, Mp) (all columns) and in columns [nc, cols) (all rows) -- what the rank-k
// accumulation reads beside the chunk's own stores.  Returns the count.
int sparse_clear_plan(SparseBlock& st, int64_t id, int64_t ld, int64_t cols, int64_t Mp, int64_t M, int64_t nc,
                      ClearRect* out);

}  // namespace gprx
