// k_pt_split.h — the critical diagonal step of the tile-dataflow factorisation (k_ptiles.hip)
// before its factor: T = L_{k,k-1} = A_{k,k-1} Linv_{k-1}^T and S = A_kk - T T^T.  Either inside
// DIAGX(k) (diagx_ts, f64: S left in the look-ahead factor's LDS image), or split over TPART(k, p)
// tasks on other workgroups (tpart_run8 f64, tpart_run f32; tpart_task picks), after which
// DIAGX(k) only fetches S (diagx_split f64) or waits for it in place (diagx_split_wait f32).
// Measurements and the forms that were tried and removed: DESIGN 4.1.1a.
#pragma once
#include "k_pt_diag.h"
#include "k_pt_dist.h"

namespace gprx {
namespace pt {

// DIAGX(k > 0)'s two products before the diagonal factor, with the result left in the
// factor's LDS image (f64, diag_factor_la):
//   T = A_{k,k-1} Linv_{k-1}^T  on the staging ring (triangular B, MAP 1), stored to HBM as
//       L_{k,k-1} AND into the LDS image as an operand;
//   A_kk - T T^T  with both fragments read from that image (no second HBM round trip, no
//       ring fill), the diagonal tile's lower 16 x 16 tiles only (MAP 2), accumulated onto
//       A_kk itself (loaded while T is stored); the result overwrites the image (lower part).
// Publishes L_{k,k-1} (lcnt[k] = k) after S (the two-call form published between the two).
// (The distributed form pushes L_{k,k-1} to the other ranks after the diagonal factor.)
template <typename T>
__device__ __forceinline__ long long diagx_ts(T* __restrict__ Akm, T* __restrict__ Akk, int64_t ld,
                                              const T* __restrict__ Lp, int* lflag, int k, T* smem, const int t,
                                              bool mark) {
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    const int lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    int sr, sc;
    wave_block<2>(w, sr, sc);
    // the S accumulators start from A_kk: its loads are in flight during T's mainloop
    // (MAP 2 layout; every element, the upper ones unused)
    acc_t sacc[2][4];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const T* ccol = Akk + (int64_t)(sc * 32 + x * 16 + Tr::orow(lk, reg)) * ld;
#pragma unroll
            for (int y = 0; y < 4; y++) sacc[x][y][reg] = ccol[sr * 64 + y * 16 + lr];
        }
    // ---- T on the ring ---------------------------------------------------------------------
    {
        int tr_, tc_;
        wave_block<1>(w, tr_, tc_);
        acc_t acc[2][4];
        tile_mma<T, 1>(acc, Akm, ld, Lp, DB, GT, 32 * (tc_ + 1), smem, t);
        __syncthreads();  // every wave done with the ring before the image overwrites it
#pragma unroll
        for (int x = 0; x < 2; x++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int jl = tc_ * 32 + x * 16 + Tr::orow(lk, reg);
#pragma unroll
                for (int y = 0; y < 4; y++) {
                    const int il = tr_ * 64 + y * 16 + lr;
                    st_sc1(Akm + il + (int64_t)jl * ld, acc[x][y][reg]);
                    smem[il + jl * SIL] = acc[x][y][reg];
                }
            }
    }
    __syncthreads();  // the image holds T
    const long long tm = mark ? wall_clock64() : 0;  // (GPRX_PT_TRACE: end of the T phase)
    // ---- A_kk - T T^T from the image ----------------------------------------------------------
    // fragments of step kq + 1 are read while the MFMAs of step kq run (as tile_mma)
    T fb[2][2], fa[2][4];
    auto frag = [&](int kq, int r) {
        const int kc = kq * 4 + lk;
#pragma unroll
        for (int x = 0; x < 2; x++) fb[r][x] = smem[(sc * 32 + x * 16 + lr) + kc * SIL];
#pragma unroll
        for (int y = 0; y < 4; y++) fa[r][y] = smem[(sr * 64 + y * 16 + lr) + kc * SIL];
    };
    frag(0, 0);
#pragma unroll 2
    for (int kq = 0; kq < GT / 4; kq++) {
        if (kq + 1 < GT / 4) frag(kq + 1, (kq + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int x = 0; x < 2; x++)
#pragma unroll
            for (int y = 0; y < 4; y++)
                if (4 * sr + y >= 2 * sc + x) sacc[x][y] = Tr::mma(-fb[kq & 1][x], fa[kq & 1][y], sacc[x][y]);
    }
    // L_{k,k-1} final: unblocks the updates of column k.  Published after S so the HBM stores'
    // latency hides under S; its barrier is also "every read of T done" for the image below.
    publish(lflag, k, false);
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int jl = sc * 32 + x * 16 + Tr::orow(lk, reg);
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const int il = sr * 64 + y * 16 + lr;
                if (4 * sr + y >= 2 * sc + x) smem[il + jl * SIL] = sacc[x][y][reg];
            }
        }
    __syncthreads();
    return tm;
}

// ---- the split diagonal step (f64) ---------------------------------------------------------
// DIAGX(k)'s two products before the factor (T = A_{k,k-1} Linv_{k-1}^T, A_kk - T T^T: 2432
// MFMAs, 31 us on the one CU of the chain) spread over four more workgroups, in two phases
// (tpart_run):
//   1. TPART(k, p), p = 0..3: the 16-column groups p and 7 - p of T = L_{k,k-1}, stored in
//      place.  A part's stores overwrite A columns the other parts read: each part raises
//      "A read" (tflag 1) once its operand is in registers, stores only after all four have,
//      then raises "T stored" (tflag 2);
//   2. once all of T is stored and A_kk is final, part p forms the S = A_kk - T T^T quarter of
//      tile-rows p and 7 - p (T staged in LDS) into pbuf (f64: DIAGX copies the quarters
//      into its LDS image, diagx_split) or in place into A_kk (f32), and raises tflag 3.
// Tickets: TPART(k, np-1) .. (k, 0) in that order (order_tparts; np = tp_parts), after DIAGX(k-1)
// and before DIAGX(k), and no other k's parts between them (test_schedule.py checks this).
// Nothing but DIAGX(k) depends on the parts, so every ticket between them completes; a part
// waits only on its siblings, so at most np - 1 workgroups wait at once and with P >= np one
// is always free to claim the next sibling (split_for: fewer workers keep the whole step
// inside DIAGX).
// (the out-of-line functions read these through a pointer to the copy the kernel keeps in LDS,
// pt_lds_ctx_off: a reference to the kernel's Args put the whole struct in scratch memory, and
// every a.x of every task became a scratch load)
template <typename T>
struct TpCtx {
    int* ctl;
    int* lcnt;
    int* tflag;
    T* pbuf;
    const PtDist<T>* dist;
    long long tlimit;
    long long* xt;  // GPRX_PT_TRACE (one GPU): phase stamps, TPART(k, c) at 4 (4 k + c), DIAGX(k) at 4 (4 nc + k)
    int nc;
    const int* ver;  // tile versions (A_kk final: ver[k][k] = k - 1)
    int nv;
};
// LDS of a TPART: phase 1 the part's 32 Linv rows (column stride LSB: 16-B aligned vectors);
// phase 2 all of T (the 128 columns of L_{k,k-1}, CPI columns per LDS-DMA instruction, groups
// TQ apart), then the 9th tile's eight k-slices in the same area
template <typename T>
struct TpL {
    static constexpr int E = 16 / (int)sizeof(T);                    // elements per 16-B vector
    static constexpr int LSB = sizeof(T) == 8 ? 34 : 36;
    static constexpr int CPI = 64 * 16 / (DB * (int)sizeof(T));      // 1 (f64), 2 (f32)
    static constexpr int TQ = CPI * DB + (sizeof(T) == 8 ? 4 : 8);
    __device__ static int tcol(int c) { return (c / CPI) * TQ + (c % CPI) * DB; }
};
static_assert(DB * TpL<double>::LSB * sizeof(double) <= gemm_lds<double>(), "TPART staging exceeds the LDS of the launch");
static_assert(DB / TpL<double>::CPI * TpL<double>::TQ * sizeof(double) <= gemm_lds<double>(), "TPART staging exceeds the LDS");
static_assert(DB * TpL<float>::LSB * sizeof(float) <= gemm_lds<float>(), "TPART staging exceeds the LDS of the launch");
static_assert(DB / TpL<float>::CPI * TpL<float>::TQ * sizeof(float) <= gemm_lds<float>(), "TPART staging exceeds the LDS");

// wave 0: Linv_kk available to this rank (local publication, or the owner's push)
template <typename T, bool DIST>
__device__ bool tpart_wait_linv(const TpCtx<T>& a, int kk, bool& remote) {
    const unsigned* rp = nullptr;
    unsigned ep = 0;
    remote = false;
    if constexpr (DIST) {
        const PtDist<T>& D = *a.dist;
        if (__builtin_amdgcn_readfirstlane(D.loc[kk]) < 0) {
            rp = dist_flags(D, D.r) + dist_f_linv(D.nr, D.nc) + kk;
            ep = D.ep;
            remote = !__builtin_amdgcn_readfirstlane(D.acq_agent);
        }
    }
    const long long t0 = wall_clock64();
    for (;;) {
        const bool ok = rp ? (__builtin_amdgcn_readfirstlane(ld_sys(rp)) == ep) : (ld_uni(a.lcnt + kk) >= kk + 1);
        if (ok) return true;
        if (ld_uni(a.ctl + C_ERR)) return false;
        if (wall_clock64() - t0 > a.tlimit) {
            st_agent(a.ctl + C_ERR, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// wave 0: *v == want (A_kk final)
template <typename T>
__device__ bool tpart_wait_ver(const TpCtx<T>& a, const int* v, int want) {
    const long long t0 = wall_clock64();
    return wait_until([&] { return ld_uni(v) == want; }, a.ctl + C_ERR, t0, a.tlimit);
}

// wave 0: lane l < n checks f[l] >= want (one vector load, one ballot per poll)
template <typename T>
__device__ bool tpart_wait_flags(const TpCtx<T>& a, const int* f, int n, int want) {
    const int lane = threadIdx.x & 63;
    const long long t0 = wall_clock64();
    for (;;) {
        const bool good = lane >= n || ld_agent(f + (lane < n ? lane : 0)) >= want;
        if (__builtin_amdgcn_readfirstlane((uint32_t)(__ballot(!good) == 0))) return true;
        if (ld_uni(a.ctl + C_ERR)) return false;
        if (wall_clock64() - t0 > a.tlimit) {
            st_agent(a.ctl + C_ERR, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// TPART(k, p), two phases.
// 1. The 16-column groups p and 7 - p of T = L_{k,k-1} = A_{k,k-1} Linv_{k-1}^T (group g needs
//    K = 16 (g + 1): 36 MFMAs per wave in every part).  Wave w forms rows 16 w .. 16 w + 15: its
//    A fragments (every A element read by one lane of one part) go to registers at task start,
//    before Linv_{k-1} is even waited for; the 32 Linv rows, shared by all waves, through LDS.
//    Stored in place once every part has read its A (tflag 1); then tflag 2.
// 2. Once all of T is stored and A_kk is final: the part's quarter of S = A_kk - T T^T, the 9
//    lower 16 x 16 tiles of tile-rows p and 7 - p (p + 1 and 8 - p of them), from all of T in
//    LDS.  Wave w forms tile w over K = 128 and the 16-deep k-slice w of the 9th tile (36
//    MFMAs each, the slices summed in a fixed order); the tiles go to the shared S buffer;
//    tflag 3.  DIAGX(k) then copies 72 KB, not four 72 KB products (the products' sum had
//    cost it 6 us of loads per step).
// Out of line, one body for every p: inlined into the task loop the parts' code made every
// other task type 2-3x slower (TRSM 16 -> 44 us, even with no TPART in the list) -- the loop's
// registers (it sits at 256 VGPRs) and its hot code in the instruction cache.
// This is the four-part form, which f32 takes (f64: tpart_run8 below).  sb, sld: where the S
// tiles go; f32 passes A_kk and its ld (in place: the rank-8 factor reads its block from memory).
template <typename T, bool DIST>
__device__ __noinline__ bool tpart_run(const TpCtx<T>* ap, T* __restrict__ Akm, const T* __restrict__ Akk, int64_t ld,
                                       const T* __restrict__ Lp, T* __restrict__ sb, int64_t sld, int* tf, int k,
                                       const int C, T* smem, int& s_ok, const int t) {
    typedef TpL<T> Q;
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    typedef typename Tr::vec_t vec_t;
    const TpCtx<T> a = *ap;
    const int lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int g0 = C, g1 = 7 - C;                      // the part's column groups (and tile-rows)
    long long* xs = a.xt ? a.xt + 4 * (4 * (int64_t)k + C) : nullptr;
    const int nk0 = 4 * (g0 + 1), nk1 = 4 * (g1 + 1);  // k-steps of 4 of each group (nk1 > nk0)
    T* Ls = smem;
    // ---- phase 1 ---------------------------------------------------------------------------
    T af[32];  // A fragments: row 16 w + lr, k = 4 kq + lk, kq < nk1 (<= 32)
    {
        const T* ar = Akm + 16 * w + lr + (int64_t)lk * ld;
#pragma unroll
        for (int kq = 0; kq < 32; kq++)
            if (kq < nk1) af[kq] = ar[(int64_t)(4 * kq) * ld];
    }
    if (w == 0) {
        bool remote = false;
        const bool ok = tpart_wait_linv<T, DIST>(a, k - 1, remote);
        if (ok) {
            if (remote) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
    if (xs && w == 0) xs[0] = wall_clock64();  // Linv_{k-1} seen
    // Linv_{k-1} rows 16 g0 + r (r < 16) and 16 g1 + r - 16 (r >= 16), all 128 columns (zero
    // above the diagonal), as Ls[r + col LSB]: 16-B loads (4 per thread f64, 2 f32), all in flight
    {
        constexpr int VPC = 32 / Q::E, NV = 32 * DB / Q::E / NT;
        vec_t lv[NV];
#pragma unroll
        for (int u = 0; u < NV; u++) {
            const int e = u * NT + t, r = Q::E * (e % VPC), col = e / VPC;
            const int row = (r < 16) ? 16 * g0 + r : 16 * g1 + r - 16;
            lv[u] = *reinterpret_cast<const vec_t*>(Lp + row + (int64_t)col * DB);
        }
#pragma unroll
        for (int u = 0; u < NV; u++) {
            const int e = u * NT + t;
            *reinterpret_cast<vec_t*>(Ls + Q::E * (e % VPC) + (e / VPC) * Q::LSB) = lv[u];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (w == 0) st_agent(tf + C, 1);  // "A read": this part's A fragments have landed
    // acc[x][reg] = T(16 w + lr, 16 g_x + orow(lk, reg))
    acc_t acc[2] = {acc_t{0}, acc_t{0}};
#pragma unroll
    for (int kq = 0; kq < 32; kq++) {
        if (kq < nk1) {
            const int kc = 4 * kq + lk;
            acc[1] = Tr::mma(Ls[(16 + lr) + kc * Q::LSB], af[kq], acc[1]);
            if (kq < nk0) acc[0] = Tr::mma(Ls[lr + kc * Q::LSB], af[kq], acc[0]);
        }
    }
    if (xs && w == 0) xs[1] = wall_clock64();  // T computed
    // the in-place stores overwrite A columns the other parts read: wait for their "A read"
    // (the four parts hold consecutive tickets and need only a CU each: P >= 4, potrf_tiles)
    if (w == 0) s_ok = tpart_wait_flags<T>(a, tf, 4, 1) ? 1 : 0;
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++)
            st_sc1(Akm + 16 * w + lr + (int64_t)(16 * (x ? g1 : g0) + Tr::orow(lk, reg)) * ld, acc[x][reg]);
    publish(tf + C, 2, false);  // this part's columns of L_{k,k-1} stored
    if (xs && w == 0) xs[2] = wall_clock64();
    // ---- phase 2 ---------------------------------------------------------------------------
    if (w == 0) {
        bool ok = tpart_wait_flags<T>(a, tf, 4, 2);                           // all of T
        if (ok) ok = tpart_wait_ver<T>(a, a.ver + (int64_t)k * a.nv + k, k - 1);  // A_kk final
        if (ok) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
    // T (column c at smem + tcol(c)) by LDS-DMA, CPI 128-row columns per wave instruction
    {
        constexpr int LPC = 64 / Q::CPI;  // lanes per column
        for (int q = w; q < DB / Q::CPI; q += NT / 64)
            __builtin_amdgcn_global_load_lds(
                (const void*)(Akm + Q::E * (lane % LPC) + (int64_t)(Q::CPI * q + lane / LPC) * ld),
                (__attribute__((address_space(3))) void*)(smem + q * Q::TQ), 16, 0, 0);
    }
    // the quarter's tiles: tau <= p -> (p, tau), else (7 - p, tau - p - 1); wave w: tile w, and
    // the k-slice w of tile 8
    auto tile_of = [&](int tau, int& R, int& Cc) {
        R = (tau <= g0) ? g0 : g1;
        Cc = (tau <= g0) ? tau : tau - g0 - 1;
    };
    int R0, C0, R8, C8;
    tile_of(w, R0, C0);
    tile_of(8, R8, C8);
    acc_t s0;  // A_kk's tile w, loaded while T lands
#pragma unroll
    for (int reg = 0; reg < 4; reg++) s0[reg] = Akk[(16 * R0 + lr) + (int64_t)(16 * C0 + Tr::orow(lk, reg)) * ld];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 8
    for (int kq = 0; kq < 32; kq++) {
        const int kc = 4 * kq + lk;
        s0 = Tr::mma(-smem[Q::tcol(kc) + 16 * C0 + lr], smem[Q::tcol(kc) + 16 * R0 + lr], s0);
    }
    acc_t s8 = acc_t{0};
#pragma unroll
    for (int kq = 4 * w; kq < 4 * w + 4; kq++) {
        const int kc = 4 * kq + lk;
        s8 = Tr::mma(-smem[Q::tcol(kc) + 16 * C8 + lr], smem[Q::tcol(kc) + 16 * R8 + lr], s8);
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++)
        st_sc1(sb + (16 * R0 + lr) + (int64_t)(16 * C0 + Tr::orow(lk, reg)) * sld, s0[reg]);
    __syncthreads();  // every wave done reading T: its area takes the 9th tile's k-slices
#pragma unroll
    for (int reg = 0; reg < 4; reg++) smem[w * 256 + lane * 4 + reg] = s8[reg];
    __syncthreads();
    if (t < 256) {  // the 9th tile: A_kk + the eight k-slices, in order
        const int ln = t >> 2, reg = t & 3;
        const int r = 16 * R8 + (ln & 15), c = 16 * C8 + Tr::orow(ln >> 4, reg);
        T v = Akk[r + (int64_t)c * ld];
#pragma unroll
        for (int w8 = 0; w8 < 8; w8++) v += smem[w8 * 256 + t];
        st_sc1(sb + r + (int64_t)c * sld, v);
    }
    if (xs && w == 0) xs[3] = wall_clock64();  // S quarter computed (its stores in flight)
    publish(tf + C, 3, false);
    return true;
}

// TPART(k, p), eight parts (f64): p = C + 4 h, column groups g0 = C, g1 = 7 - C.
// 1. T's rows 64 h .. 64 h + 63 of groups g0, g1: wave w forms the 16 x 16 block of row tile
//    w & 3 and group w >> 2 (per SIMD, waves w and w + 4: one block of each group, 4 (g0 + 1) +
//    4 (g1 + 1) = 36 MFMAs, half the four-part form's), stored in place once the four parts of
//    the same rows have read their A operand (the other half's parts read other rows); tflag 2.
// 2. Once all of T is stored and A_kk is final: tiles 5 h .. of the quarter of tile-rows g0, g1
//    (5 and 4 of its 9), each over all of T as eight 16-column slices, one per wave (20 or 16
//    MFMAs per wave against 36), summed with A_kk through LDS into the S buffer; tflag 3.  (A
//    split of the quarter by T's column halves halved the staging too, but DIAGX then summed two
//    S buffers: its copy went 1.9 -> 3.5 us.)
// Same tickets and waits as the four-part form (order_tparts: TPART(k, 7) .. (k, 0); P >= 8).
template <typename T, bool DIST>
__device__ __noinline__ bool tpart_run8(const TpCtx<T>* ap, T* __restrict__ Akm, const T* __restrict__ Akk, int64_t ld,
                                        const T* __restrict__ Lp, T* __restrict__ sb, int* tf, int k, const int p,
                                        T* smem, int& s_ok, const int t) {
    typedef TpL<T> Q;
    typedef Mfma<T> Tr;
    typedef typename Tr::acc_t acc_t;
    typedef typename Tr::vec_t vec_t;
    const TpCtx<T> a = *ap;
    const int lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    const int C = p & 3, h = p >> 2;
    const int g0 = C, g1 = 7 - C;
    long long* xs = (a.xt && h == 0) ? a.xt + 4 * (4 * (int64_t)k + C) : nullptr;  // (trace: the h = 0 parts)
    // ---- phase 1 ---------------------------------------------------------------------------
    {
        const int rt = w & 3, gi = w >> 2, g = gi ? g1 : g0, nk = 4 * (g + 1);  // k-steps of 4 (<= 32)
        const int row0 = 64 * h + 16 * rt;
        T* Ls = smem;
        T af[32];  // A fragments: row row0 + lr, k = 4 kq + lk, kq < nk
        {
            const T* ar = Akm + row0 + lr + (int64_t)lk * ld;
#pragma unroll
            for (int kq = 0; kq < 32; kq++)
                if (kq < nk) af[kq] = ar[(int64_t)(4 * kq) * ld];
        }
        if (w == 0) {
            bool remote = false;
            const bool ok = tpart_wait_linv<T, DIST>(a, k - 1, remote);
            if (ok) {
                if (remote) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            s_ok = ok ? 1 : 0;
        }
        __syncthreads();
        if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
        if (xs && w == 0) xs[0] = wall_clock64();  // Linv_{k-1} seen
        // Linv_{k-1} rows 16 g0 + r (r < 16) and 16 g1 + r - 16 (r >= 16), all columns, as
        // Ls[r + col LSB] (the four-part form's staging)
        {
            constexpr int VPC = 32 / Q::E, NV = 32 * DB / Q::E / NT;
            vec_t lv[NV];
#pragma unroll
            for (int u = 0; u < NV; u++) {
                const int e = u * NT + t, r = Q::E * (e % VPC), col = e / VPC;
                const int row = (r < 16) ? 16 * g0 + r : 16 * g1 + r - 16;
                lv[u] = *reinterpret_cast<const vec_t*>(Lp + row + (int64_t)col * DB);
            }
#pragma unroll
            for (int u = 0; u < NV; u++) {
                const int e = u * NT + t;
                *reinterpret_cast<vec_t*>(Ls + Q::E * (e % VPC) + (e / VPC) * Q::LSB) = lv[u];
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (w == 0) st_agent(tf + p, 1);  // "A read"
        acc_t acc = acc_t{0};  // T(row0 + lr, 16 g + orow(lk, reg))
#pragma unroll
        for (int kq = 0; kq < 32; kq++) {
            if (kq < nk) {
                const int kc = 4 * kq + lk;
                acc = Tr::mma(Ls[(16 * gi + lr) + kc * Q::LSB], af[kq], acc);
            }
        }
        if (xs && w == 0) xs[1] = wall_clock64();  // T computed
        if (w == 0) s_ok = tpart_wait_flags<T>(a, tf + 4 * h, 4, 1) ? 1 : 0;  // this half's readers
        __syncthreads();
        if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) st_sc1(Akm + row0 + lr + (int64_t)(16 * g + Tr::orow(lk, reg)) * ld, acc[reg]);
        publish(tf + p, 2, false);
        if (xs && w == 0) xs[2] = wall_clock64();
    }
    // ---- phase 2 ---------------------------------------------------------------------------
    if (w == 0) {
        bool ok = tpart_wait_flags<T>(a, tf, 8, 2);                           // all of T
        if (ok) ok = tpart_wait_ver<T>(a, a.ver + (int64_t)k * a.nv + k, k - 1);  // A_kk final
        if (ok) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
    // all of T (column c at smem + tcol(c)) by LDS-DMA
    {
        constexpr int LPC = 64 / Q::CPI;
        for (int q = w; q < DB / Q::CPI; q += NT / 64)
            __builtin_amdgcn_global_load_lds(
                (const void*)(Akm + Q::E * (lane % LPC) + (int64_t)(Q::CPI * q + lane / LPC) * ld),
                (__attribute__((address_space(3))) void*)(smem + q * Q::TQ), 16, 0, 0);
    }
    // the quarter's tiles tau (tau <= g0: (g0, tau), else (g1, tau - g0 - 1)); this part takes
    // tau = 5 h .. 5 h + nt - 1 (5 and 4 of them), each as eight 16-column slices, slice w on
    // wave w; the slices are summed with A_kk in a fixed order through LDS
    auto tile_of = [&](int tau, int& R, int& Cc) {
        R = (tau <= g0) ? g0 : g1;
        Cc = (tau <= g0) ? tau : tau - g0 - 1;
    };
    const int tau0 = 5 * h, nt = h ? 4 : 5;
    // this thread's output elements (e = t, t + 512, t + 1024 < 256 nt) and their A_kk values,
    // loaded while T lands
    T av[3];
#pragma unroll
    for (int u = 0; u < 3; u++) {
        const int e = t + u * NT;
        av[u] = T(0);
        if (e < 256 * nt) {
            int R, Cc;
            tile_of(tau0 + (e >> 8), R, Cc);
            const int ln = (e & 255) >> 2, reg = e & 3;
            av[u] = Akk[(16 * R + (ln & 15)) + (int64_t)(16 * Cc + Tr::orow(ln >> 4, reg)) * ld];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    acc_t sl[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        sl[i] = acc_t{0};
        if (i < nt) {
            int R, Cc;
            tile_of(tau0 + i, R, Cc);
#pragma unroll
            for (int kq = 4 * w; kq < 4 * w + 4; kq++) {
                const int kc = 4 * kq + lk;
                sl[i] = Tr::mma(-smem[Q::tcol(kc) + 16 * Cc + lr], smem[Q::tcol(kc) + 16 * R + lr], sl[i]);
            }
        }
    }
    __syncthreads();  // every wave done reading T: its area takes the slices
#pragma unroll
    for (int i = 0; i < 5; i++)
        if (i < nt)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) smem[(i * 8 + w) * 256 + lane * 4 + reg] = sl[i][reg];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 3; u++) {
        const int e = t + u * NT;
        if (e < 256 * nt) {
            const int i = e >> 8, el = e & 255;
            int R, Cc;
            tile_of(tau0 + i, R, Cc);
            const int ln = el >> 2, reg = el & 3;
            T v = av[u];
#pragma unroll
            for (int w8 = 0; w8 < 8; w8++) v += smem[(i * 8 + w8) * 256 + el];
            st_sc1(sb + (16 * R + (ln & 15)) + (int64_t)(16 * Cc + Tr::orow(ln >> 4, reg)) * DB, v);
        }
    }
    if (xs && w == 0) xs[3] = wall_clock64();  // the part's S tiles computed (their stores in flight)
    publish(tf + p, 3, false);
    return true;
}

template <typename T, bool DIST>
__device__ __forceinline__ bool tpart_task(const TpCtx<T>* ap, T* Akm, T* Akk, int64_t ld, const T* Lp, int k, int c,
                                           T* smem, int& s_ok, const int t) {
    // S's quarters: f64 into the S buffer (DIAGX copies it into the look-ahead factor's LDS
    // image); f32 in place into A_kk (the rank-8 factor reads its block from memory)
    if constexpr (diag_la<T>)
        return tpart_run8<T, DIST>(ap, Akm, Akk, ld, Lp, ap->pbuf, ap->tflag + TP_STRIDE * k, k, c, smem, s_ok, t);
    else
        return tpart_run<T, DIST>(ap, Akm, Akk, ld, Lp, Akk, ld, ap->tflag + TP_STRIDE * k, k, c, smem, s_ok, t);
}

// DIAGX(k > 0) of the split step, f32 (the parts wrote S into A_kk): wait for the four
// quarters, then L_{k,k-1} is final (lcnt[k] = k)
template <typename T>
__device__ __forceinline__ bool diagx_split_wait(const TpCtx<T>* ap, int k, int& s_ok) {
    const int w = threadIdx.x >> 6;
    if (w == 0) {
        const bool ok = tpart_wait_flags<T>(*ap, ap->tflag + TP_STRIDE * k, 4, 3);
        if (ok) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            st_agent(ap->lcnt + k, k);
        }
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(s_ok) != 0;
}

// DIAGX(k > 0) of the split step: S (the 36 lower 16 x 16 tiles, assembled in the shared S
// buffer by the parts) into the factor's LDS image, then L_{k,k-1} is final (lcnt[k] =
// k).  Each wave waits for the parts itself and copies 576 element pairs, 9 per lane
// (lower tile tau = q / 128, pair q % 8 of its column (q % 128) / 8), one batch of loads.
template <typename T>
__device__ __noinline__ bool diagx_split(const TpCtx<T>* ap, int k, T* smem, int& s_ok, const int t) {
    typedef typename Mfma<T>::vec_t vec_t;
    const TpCtx<T> a = *ap;
    const int lane = t & 63, w = t >> 6;
    const int* tf = a.tflag + TP_STRIDE * k;
    long long* xs = a.xt ? a.xt + 4 * (4 * (int64_t)a.nc + k) : nullptr;
    int rr[9], cc[9];
#pragma unroll
    for (int u = 0; u < 9; u++) {
        const int q = 576 * w + 64 * u + lane, tau = q >> 7, e = q & 127;
        int R = 0;  // lower tile tau = R (R + 1) / 2 + C
        while ((R + 1) * (R + 2) / 2 <= tau) R++;
        const int C = tau - R * (R + 1) / 2;
        rr[u] = 16 * R + 2 * (e & 7);
        cc[u] = 16 * C + (e >> 3);
    }
    constexpr int NP = tp_parts(std::is_same<T, double>::value);
    const bool ok = tpart_wait_flags<T>(a, tf, NP, 3);  // this wave polls the parts itself
    if (ok) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (xs && w == 0) xs[2] = wall_clock64();  // every quarter seen
        vec_t v[9];
#pragma unroll
        for (int u = 0; u < 9; u++) v[u] = *reinterpret_cast<const vec_t*>(a.pbuf + rr[u] + cc[u] * DB);
#pragma unroll
        for (int u = 0; u < 9; u++) {
            smem[rr[u] + cc[u] * SIL] = v[u][0];
            smem[rr[u] + 1 + cc[u] * SIL] = v[u][1];
        }
    }
    if (w == 0) s_ok = ok ? 1 : 0;
    __syncthreads();
    if (!__builtin_amdgcn_readfirstlane(s_ok)) return false;
    // every column block of L_{k,k-1} is stored (each part's flag came after its stores)
    if (w == 0) st_agent(a.lcnt + k, k);
    if (xs && w == 0) xs[3] = wall_clock64();  // S in the image
    return true;
}

}  // namespace pt
}  // namespace gprx
