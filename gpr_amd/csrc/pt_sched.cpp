// pt_sched.cpp — host: the tile factorisation's task lists and their list-schedule simulation.
//
// The persistent kernel (k_ptiles.hip) claims tickets in the order computed here.  Both planners,
// the single-GPU one (make_schedule) and the sharded one (make_schedule_dist), only create their
// tasks and dependency edges; one Dag links, ranks and simulates them:
//   * link() refuses an edge whose producer was created after its consumer, so creation order is a
//     topological order of every graph that gets as far as the simulation;
//   * simulate() starts a task only when all its producers have finished (or published early) and a
//     worker of its rank is free, and each rank's ticket list is its tasks in start order.
// So every task's producers hold earlier tickets -- of its own rank's list or, across ranks, in
// one global start order -- and the unfinished task that started first in the simulation always
// has its inputs and a worker: no deadlock whatever the real durations.
// The single-GPU schedule is the g = 1 case with no transport nodes.
#include "pt_sched.h"

#include <algorithm>
#include <cstdlib>
#include <functional>
#include <map>
#include <queue>
#include <utility>

namespace gprx {

namespace pt {

using namespace mm;

namespace {

// TPART tickets of one k in the order TPART(k, np-1), .., (k, 0): each part waits for
// the reads of the parts with a larger c, so those must hold the earlier tickets (the parts
// have the same inputs and one consumer, DIAGX(k): permuting them over their slots keeps
// every other order of the list)
void order_tparts(std::vector<int4>& list) {
    std::map<int, std::vector<int>> pos;
    for (size_t q = 0; q < list.size(); q++)
        if ((list[q].x & 0xff) == T_TPART) pos[list[q].y].push_back((int)q);
    for (auto& kv : pos) {
        std::vector<int>& v = kv.second;
        std::sort(v.begin(), v.end());
        for (size_t u = 0; u < v.size(); u++) list[v[u]].z = (int)v.size() - 1 - (int)u;
    }
}

// A task graph and its list schedule on g ranks of P workers.
struct Dag {
    struct Task {
        int type, i, j, b0, nb;
        int rank;  // the rank whose worker runs it; -1: a timed node that occupies no worker
        double dur;
        std::vector<int> succ, esucc;  // esucc: released at the early publication (DIAGX)
        int ndep = 0;
        double bl = 0;  // bottom level (longest path to the end, inclusive)
    };
    std::vector<Task> tasks;
    std::vector<std::vector<int>> deps, edeps;  // edeps: on L_{k,k-1}, published early by DIAGX(k)
    std::string name;                           // (error messages)

    int add(int type, int i, int j, int b0, int nb, double dur, int rank = 0) {
        tasks.push_back(Task{type, i, j, b0, nb, rank, dur, {}, {}, 0, 0.0});
        return (int)tasks.size() - 1;
    }
    // `task` needs the output of `on` (< 0: nothing); early: its early publication is enough
    void dep(int task, int on, bool early = false) {
        if (on < 0) return;
        auto& d = early ? edeps : deps;
        if ((int)d.size() <= task) d.resize(task + 1);
        d[task].push_back(on);
    }
    // the edges, each once (an early edge beside a full one is dropped), as successor lists and
    // dependency counts; creation order must put every producer before its consumers
    void link(const char* name_) {
        name = name_;
        const int nt = (int)tasks.size();
        deps.resize(nt);
        edeps.resize(nt);
        for (int id = 0; id < nt; id++) {
            auto& d = deps[id];
            auto& ed = edeps[id];
            std::sort(d.begin(), d.end());
            d.erase(std::unique(d.begin(), d.end()), d.end());
            std::sort(ed.begin(), ed.end());
            ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
            for (int on : d) {
                if (on >= id) throw Error{GPRX_ERR_ARG, name + ": producer created after consumer"};
                tasks[on].succ.push_back(id);
            }
            int ne = 0;
            for (int on : ed) {
                if (on >= id) throw Error{GPRX_ERR_ARG, name + ": producer created after consumer"};
                if (std::binary_search(d.begin(), d.end(), on)) continue;  // full dependency already
                tasks[on].esucc.push_back(id);
                ne++;
            }
            tasks[id].ndep = (int)d.size() + ne;
        }
    }
    // longest path to the end; creation order is topological (link), so in reverse
    void bottom_levels(double early) {
        for (int id = (int)tasks.size() - 1; id >= 0; id--) {
            double m = 0;
            for (int s : tasks[id].succ) m = std::max(m, tasks[s].bl);
            for (int s : tasks[id].esucc) m = std::max(m, tasks[s].bl - (tasks[id].dur - early));
            tasks[id].bl = tasks[id].dur + m;
        }
    }
    // List scheduling on g ranks of P workers each, highest bottom level first (then the higher
    // task id); events in (time, id) order, the ranks served in increasing order at each event.
    // lists[rank]: its tickets in start order.  Returns the makespan.
    double simulate(int g, int P, double early, std::vector<std::vector<int4>>& lists) {
        typedef std::pair<double, int> PQ;
        const int nt = (int)tasks.size();
        std::vector<std::priority_queue<PQ>> ready(g);
        // events: (time, task) finishing, or (time, -1 - task) for an early publication
        std::priority_queue<PQ, std::vector<PQ>, std::greater<PQ>> running;
        std::vector<int> indeg(nt), freew(g, P);
        lists.assign(g, {});
        double now = 0;
        int started = 0;
        auto make_ready = [&](int id) {
            if (tasks[id].rank < 0) {  // transport / release: starts at once, no worker
                running.push({now + tasks[id].dur, id});
                started++;
            } else {
                ready[tasks[id].rank].push({tasks[id].bl, id});
            }
        };
        for (int id = 0; id < nt; id++) {
            indeg[id] = tasks[id].ndep;
            if (indeg[id] == 0) make_ready(id);
        }
        while (started < nt || !running.empty()) {
            for (int rk = 0; rk < g; rk++)
                while (freew[rk] > 0 && !ready[rk].empty()) {
                    const int id = ready[rk].top().second;
                    ready[rk].pop();
                    const Task& tk = tasks[id];
                    lists[rk].push_back(make_int4(tk.type | (tk.nb << 8), tk.i, tk.j, tk.b0));
                    running.push({now + tk.dur, id});
                    if (!tk.esucc.empty()) running.push({now + std::min(early, tk.dur), -1 - id});
                    freew[rk]--;
                    started++;
                }
            if (running.empty()) throw Error{GPRX_ERR_ARG, name + ": dependency cycle"};
            const PQ f = running.top();
            running.pop();
            now = f.first;
            if (f.second < 0) {
                for (int s : tasks[-1 - f.second].esucc)
                    if (--indeg[s] == 0) make_ready(s);
                continue;
            }
            if (tasks[f.second].rank >= 0) freew[tasks[f.second].rank]++;
            for (int s : tasks[f.second].succ)
                if (--indeg[s] == 0) make_ready(s);
        }
        return now;
    }
};

// an update chunk: panels [b0, b0 + nb) of tile (i, j)
struct Chunk {
    int i, j, b0, nb;
};

// producer of L_{i,b} (early: the trsm phase of DIAGX(i) already published it); returned as one
// value, so a call inside an argument list cannot be read before it is made
struct Prod {
    int id;
    bool early;
};
Prod prod_l(const std::vector<int>& diagx, const std::vector<int>& trsm, int nc, int i, int b) {
    if (i < nc && (b == i || b == i - 1)) return {diagx[i], b == i - 1};
    return {trsm[(size_t)i * nc + b], false};
}

// Chunks of the updates of tile (i, j): b in [0, e), e = j (i > j) or j - 1 (diagonal tile:
// the last one is applied inside DIAGX(j)).  Aligned W-chunks up to the last multiple of W
// at or before column j, then the remainder before the last `near` panels in power-of-two
// pieces (W/2, W/4, ..., 1), then single panels -- few tasks (each costs a fixed ~6 us of
// ticket, waits, fences and C read-modify-write), while the last panels of a tile, the ones
// the diagonal chain waits for, still go one at a time.
// s > 0 (an identity row block of the inverse, whose panels before s are zero): the same
// rule on the panels [s, e), shifted.
// ratio > 0 (chosen per shape by the simulated makespan, best_schedule): greedy from the first
// panel, the widest power-of-two piece p <= W (W-aligned when p == W) that ends at least `near`
// panels before e and is at most ratio x the panels left after it.  A piece can start only
// when its last panel is final, so a wide piece close to the tile's last panel holds up the
// tile's consumer: at N = 4096 the [0, 16) piece of tiles (18, 17) and (18, 18) became ready
// with panel 15 and ran 280 us, and DIAGX(18) waited 184 us for it (r03 trace).
void tile_chunks(int i, int j, int W, int near, std::vector<std::pair<int, int>>& out, int s = 0, int ratio = 0) {
    out.clear();
    const int e = ((i == j) ? j - 1 : j) - s;
    if (e <= 0) return;
    if (ratio > 0) {
        for (int b = 0; b < e;) {
            int p = W;
            for (; p > 1; p /= 2) {
                if (p == W && b % W) continue;
                const int end = b + p;
                if (end > e - near || p > ratio * (e - end)) continue;
                break;
            }
            out.push_back({s + b, p});
            b += p;
        }
        return;
    }
    int hb = std::max(0, std::min(W * ((j - s) / W), e));
    hb -= hb % W;
    int b = 0;
    for (; b + W <= hb; b += W) out.push_back({s + b, W});
    for (int p = W / 2; p >= 1; p /= 2)
        if (b + p <= e - near) {
            out.push_back({s + b, p});
            b += p;
        }
    for (; b < e; b++) out.push_back({s + b, 1});
}

// ni > 0: the last ni row blocks are the identity (the inverse L^{-1} riding along as
// L^{-T} rows): identity block a = i - (nr - ni) has zero L blocks before column block a.
// tail > 0: the capped rule (ratio) only for the tiles of the last `tail` column blocks, the
// fixed rule before them
// pair > 0 (round 6): the off-diagonal tiles of column j from row j + pair down to the last label
// row go in vertical pairs (j + pair, j + pair + 1), ..., each pair's identical chunks as ONE
// T_UPD2 task (a 256 x 128 update: tile_gemm_tall); the `pair` - 1 tiles right below the
// diagonal -- the diagonal chain's inputs -- and the identity rows stay single
// narrow: the label row block nc (the only one) updates as a 16-row product (tile_gemm_rows16).  As
// the bottom of a pair it would gain nothing -- the pair lasts as long as the waves that hold the
// matrix row -- so it is never one: the rows i >= nc leave the pairs, row nc - 1 runs single in
// the columns where it was the label row's top, and the label updates are priced at Cost::klab
// id_pair, id_tail: Params' switches of the identity rows' pairing
Schedule make_schedule(int nc, int nr, int W, int near, int P, const Cost& cm0, bool build, int ni, int ratio, bool split,
                       int tail, int pair, bool narrow, bool id_pair, bool id_tail) {
    Cost cm = cm0;
    if (split) cm.early = cm.early_s;
    const int nr0 = nr - ni;
    narrow = narrow && nr0 == nc + 1;
    const int pend = narrow ? nc : nr0;  // the matrix-row pairs end before row block pend
    auto start_of = [&](int i) { return i >= nr0 ? i - nr0 : 0; };
    // identity rows in pairs (E_2s, E_2s+1): both update from panel 2s -- the bottom row's block at
    // column 2s is a stored zero (potrf_tiles zeroes it and starts its counters at 2s), so its
    // one extra panel subtracts nothing and the two rows' chunk lists are identical
    const bool ident_even = id_pair && pair > 0 && ni > 1;
    auto cstart = [&](int i) {
        const int a = start_of(i);
        return (ident_even && i >= nr0) ? a - (a & 1) : a;
    };
    // row i of column j: 1 the top of a pair, 2 its bottom, 0 single
    auto pair_role = [&](int i, int j) {
        if (pair <= 0) return 0;
        if (i >= nr0) {  // identity rows: (E_2s, E_2s+1)
            const int a = i - nr0;
            if (!ident_even) return 0;
            if ((a & 1) == 0) return a + 1 < ni ? 1 : 0;
            return 2;
        }
        const int r0 = j + pair;
        if (i >= r0 && (i - r0) % 2 == 0 && i + 1 < pend) return 1;
        if (i - 1 >= r0 && (i - 1 - r0) % 2 == 0 && i < pend) return 2;
        return 0;
    };
    Dag D;
    D.tasks.reserve((size_t)nr * nc * 2);
    std::vector<int> diagx(nc, -1);
    std::vector<int> trsm((size_t)nr * nc, -1);
    std::vector<int> last_upd((size_t)nr * nc, -1);
    // update chunks bucketed by their last block
    std::vector<std::vector<Chunk>> by_last(nc);
    {
        std::vector<std::pair<int, int>> ch;
        for (int j = 1; j < nc; j++)
            for (int i = j; i < nr; i++) {
                tile_chunks(i, j, W, near, ch, cstart(i), (tail <= 0 || j >= nc - tail) ? ratio : 0);
                for (auto& c : ch) by_last[c.first + c.second - 1].push_back(Chunk{i, j, c.first, c.second});
            }
    }
    auto make_diagx = [&](int k) {
        if (split && k >= 1) {  // TPART(k, np-1..0), then DIAGX(k) on their products
            int tp[8];
            for (int c = cm.np - 1; c >= 0; c--) {
                tp[c] = D.add(T_TPART, k, c, 0, 0, cm.tpart + cm.tpart_c * (c + 1));
                D.dep(tp[c], diagx[k - 1]);
                D.dep(tp[c], last_upd[(size_t)k * nc + (k - 1)]);
                D.dep(tp[c], last_upd[(size_t)k * nc + k]);  // phase 2 starts from A_kk
            }
            const int id = D.add(T_DIAGX, k, k, 0, 0, cm.diagx_s);
            diagx[k] = id;
            for (int c = 0; c < cm.np; c++) D.dep(id, tp[c]);
            D.dep(id, last_upd[(size_t)k * nc + k]);
            return;
        }
        const double dur = (k == 0) ? cm.diag0 : cm.diagx;
        const int id = D.add(T_DIAGX, k, k, 0, 0, dur);
        diagx[k] = id;
        if (k >= 1) {
            D.dep(id, diagx[k - 1]);
            D.dep(id, last_upd[(size_t)k * nc + (k - 1)]);
            D.dep(id, last_upd[(size_t)k * nc + k]);
        }
    };
    // Creation order (checked by Dag::link) puts every producer before its consumers:
    // [BUILD(i, j) for the lower tiles], DIAGX(0); per k: TRSM(., k), DIAGX(k+1), the update
    // chunks ending at block k.  A tile's BUILD is its first "update".
    if (build)
        for (int i = 0; i < nc; i++)
            for (int j = 0; j <= i; j++) last_upd[(size_t)i * nc + j] = D.add(T_BUILD, i, j, 0, 0, cm.build);
    make_diagx(0);
    D.dep(diagx[0], last_upd[0]);
    for (int k = 0; k < nc; k++) {
        for (int i = k + 1; i < nr; i++) {
            if (i == k + 1 && i < nc) continue;  // inside DIAGX(k+1)
            if (k < start_of(i)) continue;        // zero block of an identity row
            const int id = D.add(T_TRSM, i, k, 0, 0, cm.trsm);
            trsm[(size_t)i * nc + k] = id;
            D.dep(id, diagx[k]);
            D.dep(id, last_upd[(size_t)i * nc + k]);
        }
        if (k + 1 < nc) make_diagx(k + 1);
        for (const Chunk& c : by_last[k]) {
            const bool pairable = c.nb >= cm.pair_nbmin && (c.j < nc - cm.pair_tail || (c.i >= nr0 && id_tail));
            const int role = pairable ? pair_role(c.i, c.j) : 0;
            if (role == 2) continue;  // (the pair's top row made the task: identical chunks)
            if (role == 1) {
                const int id = D.add(T_UPD2, c.i, c.j, c.b0, c.nb, cm.ovh + 2.0 * c.nb * cm.k128 * cm.tall);
                for (int r = c.i; r <= c.i + 1; r++) D.dep(id, last_upd[(size_t)r * nc + c.j]);
                for (int r : {c.i, c.i + 1, c.j}) {
                    const Prod p = prod_l(diagx, trsm, nc, r, k);
                    D.dep(id, p.id, p.early);
                }
                last_upd[(size_t)c.i * nc + c.j] = id;
                last_upd[(size_t)(c.i + 1) * nc + c.j] = id;
                continue;
            }
            const bool lab = narrow && c.i == nc && cm.klab >= 0;
            const double dur = cm.ovh + c.nb * (lab ? cm.klab : cm.k128 * (c.i == c.j ? cm.diagf : 1.0));
            const int id = D.add(T_UPD, c.i, c.j, c.b0, c.nb, dur);
            D.dep(id, last_upd[(size_t)c.i * nc + c.j]);
            for (int r : {c.i, c.j}) {
                const Prod p = prod_l(diagx, trsm, nc, r, k);
                D.dep(id, p.id, p.early);
            }
            last_upd[(size_t)c.i * nc + c.j] = id;
        }
    }
    D.link("potrf tile schedule");
    D.bottom_levels(cm.early);
    std::vector<std::vector<int4>> lists;
    Schedule S;
    S.est_us = D.simulate(1, P, cm.early, lists);
    S.list = std::move(lists[0]);
    S.ntasks = (int64_t)D.tasks.size();
    S.ident_even = ident_even;
    if (split) order_tparts(S.list);
    return S;
}

// ------------------------------------------------------------------------------------------
// Distributed schedule (gprx_dist.cpp): the single-GPU task DAG with row block i on rank
// own(i) = (i / gb) mod g (identity row E_a with row a), plus, as timed nodes that occupy no
// worker:
//   push(i, b)   tile L_ib from its rank into the window of every rank that reads row i
//   pushL(k)     Linv_k from DIAGX(k)'s rank into every other rank's Linv array
//   rel(q, p)    rank q's last window-reading update chunk covering panel p is done: the window
//                slot p mod ww may be refilled on q
// A task whose input lives on another rank depends on its push node; a task that pushes a tile
// of panel b into a window depends on rel(q, b - ww) of every consumer q (flow control: chunks
// are at most ww / 2 panels wide, so a release never waits on the panel being pushed).
// Simulated on g x P workers; each rank's ticket list is its tasks in start order.  The
// simulation order is one topological order of the whole DAG, flow control included, so the
// unfinished task that started first in the simulation always has its inputs and a worker:
// the single-GPU deadlock argument, extended to the ranks and their windows.
//
// inv (LML mode): nc identity row blocks E_a = nc + 1 + a ride along (U = L^{-T}, tiles
// (E_a, b), b >= a) and the lower C = U U^T accumulates in tiles (E_a, E_c), c <= a, as
// update chunks over the panels b >= a (C_ac = -sum_b U_ab U_cb^T, stored negated).
// ------------------------------------------------------------------------------------------
void c_chunks(int a, int W, int nc, std::vector<std::pair<int, int>>& out) {
    out.clear();
    for (int b = a; b < nc;) {
        const int e = std::min(nc, (b / W + 1) * W);
        out.push_back({b, e - b});
        b = e;
    }
}

DistSched make_schedule_dist(int nc, bool inv, int W, int near, int P, int g, int gb, int ww, const Cost& cm0, bool build,
                             double push_us, double rel_us, int ratio = 0, bool split = false, int tail = 0) {
    Cost cm = cm0;
    if (split) cm.early = cm.early_s;
    const int nr = nc + 1 + (inv ? nc : 0), nci = inv ? 2 * nc : nc;
    auto own = [&](int i) { return i <= nc ? (i / gb) % g : ((i - nc - 1) / gb) % g; };
    auto colx = [&](int j) { return j > nc ? j - 1 : j; };  // counter column of tile (., j)
    auto start_of = [&](int i) { return i > nc ? i - nc - 1 : 0; };
    Dag D;
    std::vector<int> diagx(nc, -1), pushl(nc, -1);
    std::vector<int> trsm((size_t)nr * nc, -1), push((size_t)nr * nc, -1), last_upd((size_t)nr * nci, -1);
    auto linv = [&](int k, int rk) { return own(k) == rk ? diagx[k] : pushl[k]; };
    // the update chunks, bucketed by their last panel
    std::vector<std::vector<Chunk>> by_last(nc);
    {
        std::vector<std::pair<int, int>> ch;
        for (int j = 1; j < nc; j++)
            for (int i = j; i < nr; i++) {
                if (i > nc && start_of(i) >= j) continue;  // identity row E_a: tiles (E_a, j > a) only
                tile_chunks(i, j, W, near, ch, start_of(i), (tail <= 0 || j >= nc - tail) ? ratio : 0);
                for (auto& c : ch) by_last[c.first + c.second - 1].push_back(Chunk{i, j, c.first, c.second});
            }
        if (inv)
            for (int aa = 0; aa < nc; aa++) {
                c_chunks(aa, W, nc, ch);
                for (int c = 0; c <= aa; c++)
                    for (auto& x : ch) by_last[x.first + x.second - 1].push_back(Chunk{nc + 1 + aa, nc + 1 + c, x.first, x.second});
            }
    }
    // who reads which row through the window, and the window-reading chunks per (rank, panel)
    DistSched S;
    S.cons.assign((size_t)g * nr, 0);
    S.need.assign((size_t)g * nc, 0);
    for (int k = 0; k < nc; k++)
        for (const Chunk& c : by_last[k]) {
            const int q = own(c.i);
            if (own(c.j) == q) continue;
            S.cons[(size_t)q * nr + c.j] = 1;
            for (int p = c.b0; p < c.b0 + c.nb; p++) S.need[(size_t)q * nc + p]++;
        }
    std::vector<int> rel((size_t)g * nc, -1);
    // producers of panel p's window tiles wait for every consumer's release of panel p - ww
    auto flow = [&](int id, int i, int p) {
        if (i == nc || p - ww < 0) return;  // the label rows go to the z area, not the window
        for (int q = 0; q < g; q++)
            if (q != own(i) && S.cons[(size_t)q * nr + i]) D.dep(id, rel[(size_t)q * nc + (p - ww)]);
    };
    auto make_push = [&](int i, int b, int prod) {
        bool any = false;
        for (int q = 0; q < g && !any; q++) any = q != own(i) && S.cons[(size_t)q * nr + i];
        if (!any) return;
        const int id = D.add(-2, i, b, 0, 0, push_us, -1);
        push[(size_t)i * nc + b] = id;
        D.dep(id, prod);
    };
    auto make_diagx = [&](int k) {
        int tp[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
        if (split && k >= 1)  // TPART(k, np-1..0) on the owner of row block k
            for (int c = cm.np - 1; c >= 0; c--) {
                tp[c] = D.add(T_TPART, k, c, 0, 0, cm.tpart + cm.tpart_c * (c + 1), own(k));
                D.dep(tp[c], linv(k - 1, own(k)));
                D.dep(tp[c], last_upd[(size_t)k * nci + (k - 1)]);
                D.dep(tp[c], last_upd[(size_t)k * nci + k]);  // phase 2 starts from A_kk
            }
        const int id = D.add(T_DIAGX, k, k, 0, 0, (k == 0) ? cm.diag0 : (split ? cm.diagx_s : cm.diagx), own(k));
        diagx[k] = id;
        if (k >= 1) {
            for (int c = 0; c < cm.np; c++) D.dep(id, tp[c]);
            D.dep(id, linv(k - 1, own(k)));
            D.dep(id, last_upd[(size_t)k * nci + (k - 1)]);
            D.dep(id, last_upd[(size_t)k * nci + k]);
            flow(id, k, k - 1);  // it pushes L_{k,k-1} into window slot k - 1
            make_push(k, k - 1, id);
        }
        pushl[k] = D.add(-3, k, k, 0, 0, push_us, -1);
        D.dep(pushl[k], id);
    };
    if (build)
        for (int i = 0; i < nc; i++)
            for (int j = 0; j <= i; j++) last_upd[(size_t)i * nci + j] = D.add(T_BUILD, i, j, 0, 0, cm.build, own(i));
    make_diagx(0);
    D.dep(diagx[0], last_upd[0]);
    for (int k = 0; k < nc; k++) {
        if (k - ww >= 0)  // releases of panel k - ww: every chunk covering it was created already
            for (int q = 0; q < g; q++) {
                const int p = k - ww;
                if (!S.need[(size_t)q * nc + p]) continue;
                rel[(size_t)q * nc + p] = D.add(-4, q, p, 0, 0, rel_us, -1);  // its chunks: wired below
            }
        for (int i = k + 1; i < nr; i++) {
            if (i == k + 1 && i < nc) continue;  // inside DIAGX(k+1)
            if (k < start_of(i)) continue;        // zero block of an identity row
            const int id = D.add(T_TRSM, i, k, 0, 0, cm.trsm, own(i));
            trsm[(size_t)i * nc + k] = id;
            D.dep(id, linv(k, own(i)));
            D.dep(id, last_upd[(size_t)i * nci + k]);
            flow(id, i, k);
            make_push(i, k, id);
        }
        if (k + 1 < nc) make_diagx(k + 1);
        for (const Chunk& c : by_last[k]) {
            const int rk = own(c.i);
            const double dur = cm.ovh + c.nb * cm.k128 * (c.i == c.j ? cm.diagf : 1.0);
            const int id = D.add(T_UPD, c.i, c.j, c.b0, c.nb, dur, rk);
            D.dep(id, last_upd[(size_t)c.i * nci + colx(c.j)]);
            const Prod p1 = prod_l(diagx, trsm, nc, c.i, k);
            D.dep(id, p1.id, p1.early);
            if (own(c.j) == rk) {
                const Prod p2 = prod_l(diagx, trsm, nc, c.j, k);
                D.dep(id, p2.id, p2.early);
            } else {
                for (int b = c.b0; b <= k; b++) D.dep(id, push[(size_t)c.j * nc + b]);
            }
            last_upd[(size_t)c.i * nci + colx(c.j)] = id;
        }
    }
    // the release nodes depend on the chunks that read the window (chunks are at most W <= ww / 2
    // panels wide, so every chunk covering panel p was created before rel(., p): Dag::link checks)
    for (int id = 0, nt = (int)D.tasks.size(); id < nt; id++) {
        const Dag::Task& c = D.tasks[id];
        if (c.rank < 0 || c.type != T_UPD || own(c.j) == c.rank) continue;
        for (int p = c.b0; p < c.b0 + c.nb; p++)
            if (rel[(size_t)c.rank * nc + p] >= 0) D.dep(rel[(size_t)c.rank * nc + p], id);
    }
    D.link("potrf dist schedule");
    D.bottom_levels(cm.early);
    S.est_us = D.simulate(g, P, cm.early, S.lists);
    S.W = W;
    if (split)
        for (auto& l : S.lists) order_tparts(l);
    return S;
}

// the chunk rule with the shortest simulated makespan: the fixed rule (ratio 0), or a capped
// rule (ratio 8, 4, 2: width capped by the distance to the tile's last panel) on every tile or
// only on the last 16 / 32 column blocks -- where the chain-bound tail waits for the diagonal
// tiles' last wide chunks (N = 16384: ratio 2 on the last 16 blocks 25.46 -> 25.15 ms, the
// simulation ranks it first too) -- unless GPRX_PT_RATIO fixes it (GPRX_PT_TAIL its reach)
const int kRatios[] = {0, 8, 4, 2};
const int kTails[] = {0, 16, 32};
// Paired updates (T_UPD2) by precision, from same-box A/Bs (profiles/r06f_pair_ab.txt,
// r06lno_pair_sweep.txt, r06uv_pair_tune.txt): rows from j + 4 (f64) / j + 2 (f32), chunks of at
// least 4 panels, not in the last 32 (f64) / 16 (f32) columns -- C3's launch 25.49-25.63 ->
// 24.68-24.85 ms (pairing every chunk: 25.77; every chunk of >= 16 panels before the last 64
// columns: 25.01-25.07; rows from j + 3 or j + 6, >= 2 panels, the last 24 or 40 columns: within
// 0.3% of the default), C4's f32 factor 99.26 -> 95.23-95.26 ms (rows from j + 4: 95.5).  Pairs delay their consumers (both rows wait for the later one), which the
// narrow pieces near a tile's last panel and the chain-bound last columns cannot afford; the bulk
// gains the wider mainloop.  GPRX_PT_PAIR / _NBMIN / _TAIL override.
struct PairRule {
    int pair, nbmin, tail;
};
PairRule default_pair(bool f64) { return f64 ? PairRule{4, 4, 32} : PairRule{2, 4, 16}; }

}  // namespace

Params::Params() {
    auto geti = [](const char* name, int& v, int lo) {  // (returns whether the variable is set)
        const char* e = std::getenv(name);
        if (e) v = std::max(lo, std::atoi(e));
        return e != nullptr;
    };
    auto getd = [](const char* name, double& v) {
        if (const char* e = std::getenv(name)) v = std::atof(e);
    };
    const int any = -(1 << 30);
    geti("GPRX_PT_W", W, 1);
    geti("GPRX_PT_NEAR", near, 0);
    geti("GPRX_PT_RATIO", ratio, 0);
    getd("GPRX_PT_DIAGX_US", cm.diagx);
    getd("GPRX_PT_TRSM_US", cm.trsm);
    getd("GPRX_PT_K128_US", cm.k128);
    getd("GPRX_PT_OVH_US", cm.ovh);
    getd("GPRX_PT_BUILD_US", cm.build);
    geti("GPRX_PT_SPLIT", split, any);
    geti("GPRX_PT_TAIL", tail, any);
    geti("GPRX_PT_PAIR", pair, any);
    getd("GPRX_PT_TALL", cm.tall);
    pair_nbmin_set = geti("GPRX_PT_PAIR_NBMIN", cm.pair_nbmin, 1);
    pair_tail_set = geti("GPRX_PT_PAIR_TAIL", cm.pair_tail, 0);
    getd("GPRX_PT_TPART_US", cm.tpart);
    getd("GPRX_PT_DIAGXS_US", cm.diagx_s);
    getd("GPRX_PT_KLAB_US", cm.klab);
    geti("GPRX_PT_LABEL", label, any);
    int idp = 1, idt = 1;  // (0 turns them off)
    geti("GPRX_PT_IDPAIR", idp, any);
    geti("GPRX_PT_IDTAIL", idt, any);
    id_pair = idp != 0;
    id_tail = idt != 0;
    getd("GPRX_DIST_PUSH_US", push_us);
    getd("GPRX_DIST_REL_US", rel_us);
}

const Params& params() {
    static Params p;
    return p;
}

Schedule best_schedule(int nc, int nr, const Params& pr, int P, bool build, int ni, bool split, bool f64, bool narrow) {
    Cost cm = pr.cost(f64);
    const PairRule pd = default_pair(f64);
    if (!pr.pair_nbmin_set) cm.pair_nbmin = pd.nbmin;
    // with the inverse riding along (ni > 0, the LML) the factor's last columns are not the end of
    // the launch -- the identity rows' updates follow them -- so they pair too: the LML's factor
    // launch 46.83-47.00 -> 46.42-46.57 ms (last 16 columns spared: 46.49-46.60; same box,
    // profiles/r06ls_lml_pair_sweep.txt)
    if (!pr.pair_tail_set) cm.pair_tail = ni > 0 ? 0 : pd.tail;
    const int pair = pr.pair >= 0 ? pr.pair : pd.pair;
    Schedule best;
    bool have = false;
    auto consider = [&](Schedule&& S) {
        // a rule with more tasks must win by > 0.5%
        if (!have || S.est_us < best.est_us * 0.995) {
            best = std::move(S);
            have = true;
        }
    };
    if (pr.ratio >= 0) {
        consider(make_schedule(nc, nr, pr.W, pr.near_for(nc), P, cm, build, ni, pr.ratio, split, pr.tail, pair, narrow, pr.id_pair,
                               pr.id_tail));
        return best;
    }
    for (int r : kRatios)
        for (int tl : kTails) {
            if ((r == 0 && tl) || (tl && tl >= nc)) continue;
            consider(make_schedule(nc, nr, pr.W, pr.near_for(nc), P, cm, build, ni, r, split, tl, pair, narrow, pr.id_pair,
                                   pr.id_tail));
        }
    return best;
}

// the split diagonal step runs for both precisions (f64: S through the look-ahead factor's LDS
// image; f32: S in place for the rank-8 factor), unless GPRX_PT_SPLIT=0
// (the parts of a step wait for each other: at least tp_parts workgroups)
bool split_for(bool f64, int P) { return P >= tp_parts(f64) && params().split != 0; }

}  // namespace pt

// ---- distributed factorisation: per-rank ticket lists ------------------------------------------
DistSched potrf_dist_schedule(int nc, int g, int gb, int ww, int P, bool build, bool inv, int ratio, bool f64, int tail) {
    const pt::Params& pr = pt::params();
    ww = std::max(2, std::min(ww, nc));
    // update chunks at most half a window wide (flow control, make_schedule_dist), powers of two
    int W = 1;
    while (2 * W <= std::min(pr.W, std::max(1, ww / 2))) W *= 2;
    return pt::make_schedule_dist(nc, inv, W, pr.near_for(nc), P, g, std::max(1, gb), ww, pr.cost(f64), build, pr.push_us,
                                  pr.rel_us, pr.ratio >= 0 ? pr.ratio : ratio, pt::split_for(f64, P),
                                  pr.ratio >= 0 ? pr.tail : tail);
}

int64_t potrf_tiles_schedule_stats(int nc, int nr, int P, bool build, double* est_us, int ni, int ratio,
                                   int32_t* list_out, int64_t list_max, int pair, bool narrow, bool f64) {
    if (nc < 1 || nr < nc || P < 1 || ni < 0 || ni > nr - nc)
        throw Error{GPRX_ERR_ARG, "potrf tile schedule: need nc >= 1, nr >= nc + ni, P >= 1"};
    pt::Params pr = pt::params();
    if (pair >= 0) pr.pair = pair;
    const bool split = pt::split_for(f64, P);
    pt::Schedule S = ratio >= 0 ? pt::make_schedule(nc, nr, pr.W, pr.near_for(nc), P, pr.cost(f64), build, ni, ratio, split,
                                                    pr.tail, pr.pair > 0 ? pr.pair : 0, narrow, pr.id_pair, pr.id_tail)
                                : pt::best_schedule(nc, nr, pr, P, build, ni, split, f64, narrow);
    if (est_us) *est_us = S.est_us;
    if (list_out)  // the ticket list: {type | nb << 8, i, j, b0} per ticket
        for (int64_t q = 0; q < (int64_t)S.list.size() && q < list_max; q++) {
            const int4 t = S.list[q];
            list_out[4 * q] = t.x, list_out[4 * q + 1] = t.y, list_out[4 * q + 2] = t.z, list_out[4 * q + 3] = t.w;
        }
    return S.ntasks;
}

bool potrf_split_for(bool f64, int P) { return pt::split_for(f64, P); }

}  // namespace gprx
