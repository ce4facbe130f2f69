// k_pt_ops.h — the tile products of the tile-dataflow factorisation (k_ptiles.hip): one task's
// 128 x 128 (or 16 x 128, 256 x 128) output from the staged MFMA mainloops of k_mma.h, stored
// write-through (sc1) so that the task loop can publish it without a release fence.  All inline:
// they are the task loop's hot bodies.  Also the names every k_pt_*.h header uses (mm::, ho::).
#pragma once
#include "k_handoff.h"
#include "k_mma.h"

namespace gprx {
namespace pt {

using namespace mm;
// the hand-off helpers (k_handoff.h) by name: this file keeps its own control-word layout (mm::C_*)
using ho::ld_agent;
using ho::ld_sys;
using ho::ld_uni;
using ho::local_sync;
using ho::publish;
using ho::publish2;
using ho::st_agent;
using ho::st_sys;
using ho::wait_until;
using ho::wave_id;

// ------------------------------------------------------------------------------------------
// One 128x128 tile:  C = A B^T (UPDATE = false)  or  C -= A B^T (UPDATE = true), K deep.
// A: 128 rows x K (column-major, lda), B: 128 rows x K (ldb).  lower: diagonal tile, only
// row >= col is stored and the waves wholly above the diagonal skip their MFMAs.  tri: B is
// lower triangular (K = 128, a diagonal-block inverse): output columns 32 wc .. 32 wc + 31
// need only k < 32 wc + 32, the waves skip the MFMAs of the zero part.
// ------------------------------------------------------------------------------------------
// Bpan: B by 128-column panels (tile_mma): the distributed factorisation's window tiles.
// MAP: the wave -> output-block map (k_mma.h wave_block): 1 for triangular B, 2 for lower.
template <typename T, bool UPDATE, int MAP = 0>
__device__ __forceinline__ void tile_gemm(T* __restrict__ C, int64_t ldc, const T* __restrict__ A, int64_t lda,
                                          const T* __restrict__ B, int64_t ldb, int K, bool lower, T* smem,
                                          const int t, bool tri = false, const uint64_t* Bpan = nullptr) {
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    const int lane = t & 63, w = t >> 6;
    int wr, wc;
    wave_block<MAP>(w, wr, wc);
    const int lr = lane & 15, lk = lane >> 4;
    const bool active = !(lower && wr == 0 && wc >= 2);
    // UPDATE: the whole C tile is fetched into registers up front (its latency hides under the
    // mainloop; loading it unconditionally, all before any store, avoids hipcc's per-element
    // branches and vmcnt(0) waits)
    T cv[2][4][4];
    if (UPDATE && active) {
#pragma unroll
        for (int x = 0; x < 2; x++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int jl = wc * 32 + x * 16 + Tr::orow(lk, reg);
                const T* ccol = C + (int64_t)jl * ldc;
#pragma unroll
                for (int y = 0; y < 4; y++) cv[x][y][reg] = ccol[wr * 64 + y * 16 + lr];
            }
    }
    acc_t acc[2][4];
    tile_mma<T, MAP>(acc, A, lda, B, ldb, K, !active ? 0 : (tri ? 32 * (wc + 1) : K), smem, t, Bpan);
    if (!active) return;
#pragma unroll
    for (int x = 0; x < 2; x++) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int jl = wc * 32 + x * 16 + Tr::orow(lk, reg);
            T* ccol = C + (int64_t)jl * ldc;
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const int il = wr * 64 + y * 16 + lr;
                // stores are unconditional (a branch per element makes hipcc wait for every
                // previous store); above the diagonal of a diagonal tile the old value goes back.
                // sc1 (write-through) stores: the hand-off needs no L2 write-back fence
                if (UPDATE)
                    st_sc1(ccol + il, (lower && il < jl) ? cv[x][y][reg] : cv[x][y][reg] - acc[x][y][reg]);
                else if (!lower || il >= jl)
                    st_sc1(ccol + il, acc[x][y][reg]);
            }
        }
    }
}

// TRSM task: C = A B^T for the lower-triangular B = Linv_k, each wave 16 rows x 128 columns
// (k_mma.h tile_mma_trirows: every stage's triangle split evenly over the waves); C may be A.
// C3 fit trace: TRSM 15.7 -> 13.0 us per task; launch 24.75 -> 24.62 ms same box, C2 within
// noise, C4 unchanged (profiles/r06t_trsm_rows_ab.txt; out of line: 24.78 ms, not kept).
// (The MAP 1 form through tile_gemm was removed; commit 15ef139 still has it.)
template <typename T>
__device__ __forceinline__ void tile_trsm(T* C, int64_t ldc, const T* A, int64_t lda,
                                          const T* __restrict__ B, int64_t ldb, T* smem, const int t) {
    typedef Mfma<T> Tr;
    const int lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    typename Tr::acc_t acc[2][4];
    mm::tile_mma_trirows<T>(acc, A, lda, B, ldb, smem, t);
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int y = 0; y < 4; y++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
                st_sc1(C + (int64_t)(16 * (4 * x + y) + Tr::orow(lk, reg)) * ldc + 16 * w + lr, acc[x][y][reg]);
}

// Narrow label-row update: C -= A B^T for rows 0..15 of the tile only (k_mma.h tile_mma_rows16) --
// the label row block of a fit with at most 16 labels, whose other rows are stored zeros that the
// full tile would multiply (0 - 0 B^T) for nothing.  Wave w: the 16 rows x columns 16 w .. 16 w +
// 15; C - acc goes out in sc1 stores as tile_gemm<T, true> does it, the same MFMA steps in the
// same k order before the same subtraction, so the live rows keep their bits.  Rows 16..127 of
// the tile are neither read nor written.
template <typename T>
__device__ __forceinline__ void tile_gemm_rows16(T* __restrict__ C, int64_t ldc, const T* __restrict__ A, int64_t lda,
                                                 const T* __restrict__ B, int64_t ldb, int K, T* smem, const int t) {
    typedef Mfma<T> Tr;
    const int lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    T cv[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) cv[reg] = C[(int64_t)(16 * w + Tr::orow(lk, reg)) * ldc + lr];
    typename Tr::acc_t acc;
    mm::tile_mma_rows16<T>(acc, A, lda, B, ldb, K, smem, t);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) st_sc1(C + (int64_t)(16 * w + Tr::orow(lk, reg)) * ldc + lr, cv[reg] - acc[reg]);
}

// ------------------------------------------------------------------------------------------
// Paired update (T_UPD2): C -= A B^T on a 256 x 128 tile -- tiles (i, j) and (i + 1, j), which
// are adjacent rows of the column-major factor (C and A are 256 rows at one ld) -- over K panels
// of the same B (L_j).  The 8 waves take 64 x 64 blocks (tile_mma_tall: 16 MFMAs per 8 fragment
// reads, 384 DMA'd rows per stage for twice the 128 x 128 tile's flops; probe 0.901 of the f64
// MFMA bound against 0.877, f32 0.857 against 0.818, profiles/r05u).  Its 128 accumulator
// registers fit the task loop because the C tile is not prefetched into registers beside them,
// as tile_gemm does: C comes in four column chunks during the first stages and is subtracted
// from the accumulators (tile_mma_tall Csub), and -acc = C - A B^T is stored.  (Starting the
// accumulators from -C held the first MFMA for the whole 256 KB read: C3's launch lost 0.4 ms.)
// Off-diagonal tiles only.
// ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void tile_gemm_tall(T* __restrict__ C, int64_t ldc, const T* __restrict__ A, int64_t lda,
                                               const T* __restrict__ B, int64_t ldb, int K, T* smem, const int t) {
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    const int lane = t & 63, w = t >> 6;
    const int wr = w & 3, wc = w >> 2, lr = lane & 15, lk = lane >> 4;
    acc_t acc[4][4];
    mm::tile_mma_tall<T, 1>(acc, A, lda, B, ldb, K, smem, t, C, ldc);
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            T* ccol = C + (int64_t)(64 * wc + 16 * x + Tr::orow(lk, reg)) * ldc;
#pragma unroll
            for (int y = 0; y < 4; y++) st_sc1(ccol + 64 * wr + 16 * y + lr, -acc[x][y][reg]);
        }
}

}  // namespace pt
}  // namespace gprx
