// pt_sched_test — the tile schedule planner (gpr_amd/csrc/pt_sched.cpp) on its own: no libgprx, no
// HIP runtime.  Runs the grid of tests/golden/make_schedule_digests.py (single-GPU shapes in both
// precisions, the sharded shapes) and checks what holds for every schedule:
//   * each ticket list is non-empty and the simulated makespan positive;
//   * every ticket of a sharded list works on a row block its rank owns;
//   * the TPART tickets of one k are contiguous among the TPART tickets, in the order TPART(k, np-1),
//     .., (k, 0), between DIAGX(k - 1) and DIAGX(k) (tparts_ordered).
// It prints each case's task counts, chunk width and makespan ("single <case> <tasks> <est_us>",
// "sharded <case> <tasks> <W> <est_us> <tasks per rank>"): tests/test_host_api.py compares them with
// tests/golden/schedule_digests.json, which ties this host-compiler build to the schedules the
// library ships.  Also the program the sanitizer target of the Makefile builds (make pt_sched_asan).
#include <cstdio>
#include <map>
#include <vector>

#include "../../gpr_amd/csrc/pt_sched.h"

using namespace gprx;

static int g_fail = 0;
static void check(bool ok, const char* what, const char* name) {
    if (ok) return;
    g_fail++;
    std::printf("FAIL %s: %s\n", name, what);
}

// The split step's ticket order: the parts of one k are contiguous among the TPART tickets (no other
// k's part lies between them; other task types may: a ticket is a start in the simulation, and a
// worker that frees between two parts takes whatever ranks highest then), in the order np-1, .., 0,
// and all of them come before DIAGX(k) -- and after DIAGX(k - 1) where the list holds it.
static bool tparts_ordered(const std::vector<int4>& list) {
    std::map<int, size_t> diag;
    std::vector<size_t> tp;
    for (size_t q = 0; q < list.size(); q++) {
        if ((list[q].x & 0xff) == mm::T_DIAGX) diag[list[q].y] = q;
        if ((list[q].x & 0xff) == mm::T_TPART) tp.push_back(q);
    }
    std::map<int, int> seen;  // k -> parts so far
    for (size_t u = 0; u < tp.size(); u++) {
        const int4 t = list[tp[u]];
        const bool first = u == 0 || list[tp[u - 1]].y != t.y;
        if (first && seen.count(t.y)) return false;                   // another k's parts lay between
        if (!first && t.z != list[tp[u - 1]].z - 1) return false;     // descending, none skipped
        seen[t.y]++;
        if (u + 1 == tp.size() || list[tp[u + 1]].y != t.y)
            if (t.z != 0) return false;                               // the group ends with part 0
        if (!diag.count(t.y) || tp[u] > diag[t.y]) return false;      // before DIAGX(k), same list
        if (diag.count(t.y - 1) && tp[u] < diag[t.y - 1]) return false;
    }
    return true;
}

enum { BUILD = 1, IDENT = 2, NARROW = 4, F32 = 8, INV = 2 };
static int sel(int ratio, int pair) { return ((ratio + 1) << 8) | ((pair + 1) << 16); }  // -1: the planner's choice

static void single_case(int nc, int nr, int P, int flags) {
    char name[96];
    std::snprintf(name, sizeof name, "single %d,%d,%d,%d", nc, nr, P, flags);
    try {
        double est = 0;
        const int ratio = ((flags >> 8) & 0xff) - 1, pair = ((flags >> 16) & 0xff) - 1;
        const int ni = (flags & IDENT) ? nc : 0;
        const int64_t n = potrf_tiles_schedule_stats(nc, nr, P, (flags & BUILD) != 0, &est, ni, ratio, nullptr, 0, pair,
                                                     (flags & NARROW) != 0, (flags & F32) == 0);
        check(n > 0 && est > 0, "empty list or no makespan", name);
        std::printf("%s %lld %.17g\n", name, (long long)n, est);
        std::vector<int4> list((size_t)n);
        const int64_t n2 = potrf_tiles_schedule_stats(nc, nr, P, (flags & BUILD) != 0, nullptr, ni, ratio, &list[0].x, n, pair,
                                                      (flags & NARROW) != 0, (flags & F32) == 0);
        check(n2 == n, "task count changed between two calls", name);
        check(tparts_ordered(list), "TPART tickets of one k not contiguous and descending", name);
        const bool split = potrf_split_for((flags & F32) == 0, P);
        bool any_tpart = false;
        for (const int4& t : list) any_tpart = any_tpart || (t.x & 0xff) == mm::T_TPART;
        check(any_tpart == (split && nc > 1), "TPART tickets do not match the split step's switch", name);
    } catch (const Error& e) {
        check(false, e.msg.c_str(), name);
    }
}

static void dist_case(int nc, int P, int g, int gb, int ww, int flags) {
    char name[96];
    std::snprintf(name, sizeof name, "sharded %d,%d,%d,%d,%d,%d", nc, P, g, gb, ww, flags);
    try {
        const DistSched S = potrf_dist_schedule(nc, g, gb, ww, P, (flags & BUILD) != 0, (flags & INV) != 0,
                                                ((flags >> 8) & 0xff) - 1, (flags & F32) == 0);
        check(S.est_us > 0 && S.W >= 1 && 2 * S.W <= (ww > 2 ? ww : 2), "no makespan or a chunk wider than half the window",
              name);
        check((int)S.lists.size() == g, "not one list per rank", name);
        size_t total = 0;
        for (const auto& l : S.lists) total += l.size();
        std::printf("%s %zu %d %.17g", name, total, S.W, S.est_us);
        for (const auto& l : S.lists) std::printf(" %zu", l.size());
        std::printf("\n");
        for (int rk = 0; rk < (int)S.lists.size(); rk++) {
            const std::vector<int4>& l = S.lists[rk];
            check(!l.empty(), "a rank with an empty list", name);
            bool owned = true;
            for (const int4& t : l) {
                const int i = t.y;  // the row block the ticket works on (TPART: k)
                const int own = i <= nc ? (i / gb) % g : ((i - nc - 1) / gb) % g;
                owned = owned && own == rk && (t.x & 0xff) <= mm::T_UPD2;
            }
            check(owned, "a ticket on a row block its rank does not own", name);
            check(tparts_ordered(l), "TPART tickets of one k not contiguous and descending", name);
        }
    } catch (const Error& e) {
        check(false, e.msg.c_str(), name);
    }
}

int main() {
    int before = g_fail;
    for (int f : {0, (int)F32}) {
        single_case(1, 1, 256, f);
        single_case(1, 2, 256, f);
        single_case(2, 3, 256, f);
        single_case(9, 10, 256, f | sel(0, 0));
        single_case(9, 10, 7, f | sel(0, 0));
        single_case(33, 34, 256, f | BUILD | sel(2, 2));
        single_case(40, 81, 256, f | IDENT | sel(0, 4));
        single_case(40, 81, 256, f | IDENT | sel(0, 0));
        single_case(70, 73, 256, f | BUILD | sel(2, 4));
        single_case(65, 66, 256, f | BUILD);
        single_case(65, 66, 256, f | BUILD | NARROW);
        single_case(32, 33, 256, f | BUILD);
        single_case(128, 129, 256, f | BUILD);
        single_case(128, 129, 256, f | BUILD | NARROW);
    }
    std::printf("%s single-GPU schedules\n", g_fail == before ? "PASS" : "FAIL");
    before = g_fail;
    for (int ratio : {0, 2}) {
        for (int g : {2, 3, 5})
            for (int ww : {2, 3, 8}) dist_case(24, 30, g, 2, ww, BUILD | sel(ratio, -1));
        dist_case(16, 30, 3, 1, 4, BUILD | INV | sel(ratio, -1));
    }
    dist_case(32, 120, 2, 2, 16, BUILD | sel(0, -1));
    dist_case(32, 120, 2, 2, 16, BUILD | sel(2, -1));
    dist_case(48, 64, 2, 2, 16, BUILD | sel(0, -1));
    dist_case(48, 64, 2, 2, 16, BUILD | INV | sel(0, -1));
    dist_case(128, 256, 1, 1, 128, BUILD | sel(0, -1));
    dist_case(128, 256, 8, 2, 32, BUILD | sel(0, -1));
    dist_case(24, 30, 3, 2, 8, BUILD | F32 | sel(0, -1));
    dist_case(128, 256, 8, 2, 32, BUILD | F32 | sel(0, -1));
    std::printf("%s sharded schedules\n", g_fail == before ? "PASS" : "FAIL");
    return g_fail ? 1 : 0;
}
