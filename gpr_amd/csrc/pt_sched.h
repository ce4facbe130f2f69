// pt_sched.h — the tile factorisation's schedule planner (pt_sched.cpp): the ticket lists the
// persistent kernel of k_ptiles.hip claims, on one GPU and sharded over ranks, and the constants
// the planner and the kernel must agree on (task types, build variants).
//
// Plain host C++: standard headers, <hip/hip_vector_types.h> for int4 and the error type.  It
// compiles with a host compiler alone (-D__HIP_PLATFORM_AMD__), so the planner can be tested,
// sanitized and stepped through without the HIP runtime (tests/cpp/pt_sched_test.cpp).
#pragma once

#include <hip/hip_vector_types.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "gprx_error.h"

namespace gprx {

namespace mm {
// T_UPD2 (round 6): the update of two vertically adjacent tiles (i, j), (i + 1, j) over the same
// panels as one 256 x 128 product (tile_mma_tall): the single-GPU factorisation's paired chunks
enum { T_DIAGX = 0, T_TRSM = 1, T_UPD = 2, T_BUILD = 3, T_TPART = 4, T_UPD2 = 5 };
}  // namespace mm

namespace pt {

// TPART workgroups per split diagonal step: f64 eight -- part p = C + 4 h takes the column
// groups C, 7 - C of T's rows 64 h .. 64 h + 63 and the S quarter of tile-rows C, 7 - C over T's
// columns 64 h .. 64 h + 63 (tpart_run8: half the four-part form's MFMAs per wave in both phases,
// DESIGN 4.1.1a "Eight parts") -- f32 four (tpart_run).
constexpr int tp_parts(bool f64) { return f64 ? 8 : 4; }
// The diagonal factor by precision: f64 the blocked factor with look-ahead on an LDS image
// (diag_factor_la), which the split step's parts feed through the S buffer; f32 the rank-8
// register image, its block read from memory.
template <typename T>
constexpr bool diag_la = std::is_same<T, double>::value;

struct Cost {  // per-task durations (us, one CU), calibrated from GPRX_PT_TRACE timelines
    double k128 = 17.1;  // per 128-deep slice of a full tile update
    double ovh = 6.5;    // per update task: ticket, waits, fences, C read-modify-write
    double trsm = 16.0;  // TRSM tile (r01i trace: 15.9)
    double diagx = 70.0;   // DIAGX(k > 0): trsm + syrk tile + 128x128 factor/inverse (r02f trace, f64)
    double diag0 = 40.0;   // DIAGX(0): factor/inverse only
    double early = 31.0;   // DIAGX(k) publishes L_{k,k-1} after its trsm and syrk phases
    double diagf = 0.97;   // diagonal-tile update relative to a full one (2 of 8 waves idle)
    double build = 28.0;   // BUILD tile (pair statistics + kernel values + stores)
    // the split diagonal step (f64): TPART(k, c) takes tpart + tpart_c (c + 1); DIAGX(k) then
    // sums the products and factors (diagx_s), publishing L_{k,k-1} early_s into it
    // (r03w trace, N = 4096: the parts publish S ~12 us after Linv_{k-1}, DIAGX copies it in
    // 2 us and factors; step 54.4 us)
    double tpart = 11.5, tpart_c = 0.0;
    double diagx_s = 44.0, early_s = 2.0;
    int np = 4;         // TPART tasks per split step (tp_parts; set by the callers)
    // a paired update (T_UPD2) per panel, relative to two single-tile panels (the 256 x 128
    // mainloop's probe rate against the 128 x 128 tile's: 0.877 / 0.901)
    double tall = 0.975;
    // which chunks pair (make_schedule pair > 0): at least pair_nbmin panels wide, in the columns
    // before the last pair_tail (GPRX_PT_PAIR_NBMIN / GPRX_PT_PAIR_TAIL)
    int pair_nbmin = 1, pair_tail = 0;
    // per 128-deep slice of a narrow label-row update (make_schedule narrow; GPRX_PT_KLAB_US);
    // < 0: priced as a full tile's (k128).  C3 fit traces: 4.3-4.5 us per panel against 15.7 for a
    // full tile (profiles/label_rows_pt_trace_fit16384_narrow*.json); priced so, C3's launch
    // 24.28-24.30 -> 24.22-24.23 ms, same box, three rounds (profiles/label_rows_ab.txt)
    double klab = 4.3;
};

struct Schedule {
    std::vector<int4> list;  // the tickets in claim order: {type | nb << 8, i, j, b0}
    double est_us = 0;
    int64_t ntasks = 0;
    // identity rows paired (make_schedule): an odd identity row block 2s + 1 starts its updates at
    // panel 2s with its partner -- its counters start there and its tile at column 2s is zeroed
    bool ident_even = false;
};

// The planner's parameters.  Every environment variable the planner honours is read here, once
// per process (params()).
struct Params {
    // r01i sweep (scripts/sched_sweep.sh): at N = 16384 W = 64 with no single-panel tail is
    // 1.6-2.0% faster than W = 32, near = 1; at N = 4096 (chain-bound) near = 1 stays 6% faster
    int W = 64, near = -1;  // near < 0: by size (near_for)
    int ratio = -1;         // chunk-width rule of tile_chunks: < 0 picked per shape by the simulation
    int split = 1;          // f64: the split diagonal step (TPART tasks); GPRX_PT_SPLIT=0 turns it off
    int tail = 0;           // > 0: the capped chunk rule only in the last `tail` column blocks
    int pair = -1;          // paired updates (make_schedule): < 0 the precision's default (default_pair),
                            // 0 off, n > 0 pairs from row j + n (GPRX_PT_PAIR)
    int label = 1;          // the narrow label row (make_schedule narrow, tile_gemm_rows16) where a fit has
                            // at most LAB_NARROW labels; GPRX_PT_LABEL=0: the full tile and its pairing (A/B)
    // identity rows in pairs (make_schedule ident_even; GPRX_PT_IDPAIR=0: single, A/B), in the last
    // pair_tail columns too (the tail rule spares the factor's chain-bound last columns; the
    // identity rows' updates there are bulk work): LML N = 8192 73.66 -> 73.05 ms with both
    // (profiles/r06z_idpair_ab.txt); GPRX_PT_IDTAIL=0 restricts them
    bool id_pair = true, id_tail = true;
    Cost cm;
    // GPRX_PT_PAIR_NBMIN / GPRX_PT_PAIR_TAIL were given: cm's values replace default_pair's
    bool pair_nbmin_set = false, pair_tail_set = false;
    // the sharded schedule's timed nodes: a push is one tile's stores over xGMI plus the flag
    // (measured on one GPU as a same-device copy), a release one flag (GPRX_DIST_PUSH_US / _REL_US)
    double push_us = 4.0, rel_us = 2.0;
    int near_for(int nc) const { return near >= 0 ? near : (nc <= 64 ? 1 : 0); }
    Params();
    // the cost model for a precision
    Cost cost(bool f64) const {
        Cost c = cm;
        c.np = tp_parts(f64);
        return c;
    }
};
const Params& params();

// the single-GPU schedule with the shortest simulated makespan among the chunk rules
Schedule best_schedule(int nc, int nr, const Params& pr, int P, bool build, int ni, bool split, bool f64,
                       bool narrow = false);
// the split diagonal step is on for this precision and P workgroups (the parts of a step wait for
// each other: at least tp_parts workgroups)
bool split_for(bool f64, int P);

}  // namespace pt

// The simulated schedule of a distributed factorisation: per-rank ticket lists (in start
// order of one list-schedule simulation of all ranks, window flow control included), the
// window-reading chunks per (rank, panel), and the predicted makespan.  ni > 0: nc identity
// row blocks ride along (U = L^{-T}) plus the lower C = U U^T tiles (LML mode).
struct DistSched {
    std::vector<std::vector<int4>> lists;
    std::vector<int> need;            // [g * nc]
    std::vector<unsigned char> cons;  // [g * nr]: rank q reads row block j through its window
    double est_us = 0;
    int W = 0;              // update chunk width used
};
DistSched potrf_dist_schedule(int nc, int g, int gb, int ww, int P, bool build, bool inv, int ratio = 0, bool f64 = true,
                              int tail = 0);
bool potrf_split_for(bool f64, int P);  // the split diagonal step is on (this precision, P workgroups)
// Host-only schedule statistics (no device work): tasks, predicted makespan, the ticket list, and a
// check that every task's producers come earlier in the ticket order (it throws otherwise).
int64_t potrf_tiles_schedule_stats(int nc, int nr, int P, bool build, double* est_us, int ni = 0, int ratio = -1,
                                   int32_t* list_out = nullptr, int64_t list_max = 0, int pair = -1,
                                   bool narrow = false, bool f64 = true);

}  // namespace gprx
