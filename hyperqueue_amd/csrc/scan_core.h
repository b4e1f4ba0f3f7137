// The pure host pieces of phase A (scan.h: hqscan::Scanner): the parts that decide buffer sizes and trust device output, with no HIP in sight so that
// tools/scan_core_asan.cpp can run them under AddressSanitizer + UBSan on exact-size heap blocks (tests/test_scan_core.py).
//   runs_from_hist   the sparse run form of a dense (level, request) histogram
//   order_tab_layout the run table k_order_runs writes into pinned memory
//   order_passes     which radix passes the ordered view runs, read off the digit histogram
//   decode_runs      that run table validated and turned into the run form
//   wave_geometry    the slices of the dense scan (K1 / K1b / K4)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/hqtick.h"

namespace hqscan {

struct Table {  // what GPU phase A found in the ready set (Scan, scan.h, adds the launch geometry)
    uint32_t L = 0, Q = 0, G = 0;
    std::vector<uint64_t> levels;
    std::vector<uint32_t> hist;  // [G], g = level*Q + rq  (dense scan only)
    // The sparse form every host stage walks: per request its RUNS (nonempty (request, priority) pairs) in descending priority, runs of request q at
    // [run_off[q], run_off[q + 1]).  run_group = the selection plan's index of the run (dense: level * Q + rq; view: the run index itself), run_level = its
    // level (dense: index into `levels`; view: the global level rank), run_start = its first position in the view's permutation (view only).
    bool ordered = false;
    std::vector<uint32_t> run_off, run_cnt, run_group, run_level, run_start;
    std::vector<uint64_t> run_prio;
};

struct WorkerEval { const uint8_t *flags = nullptr; const uint32_t *tmc = nullptr; };  // K2's output, host addresses (valid until the next scan)

// the runs of a dense histogram: O(L * Q), which the dense scan's caps bound
inline void runs_from_hist(Table &sc) {
    const uint32_t Q = sc.Q;
    sc.ordered = false;
    sc.run_off.assign(Q + 1, 0); sc.run_cnt.clear(); sc.run_group.clear(); sc.run_level.clear(); sc.run_start.clear(); sc.run_prio.clear();
    for (uint32_t q = 0; q < Q; q++) {
        for (uint32_t l = 0; l < sc.L; l++) {
            const uint32_t c = sc.hist[(size_t)l * Q + q];
            if (!c) continue;
            sc.run_cnt.push_back(c); sc.run_group.push_back(l * Q + q); sc.run_level.push_back(l); sc.run_prio.push_back(sc.levels[l]);
        }
        sc.run_off[q + 1] = (uint32_t)sc.run_cnt.size();
    }
}

// the run table of a view of n live slots as order_runs writes it into pinned memory: [n_runs, n_levels, pad][run_rq n][run_start n][run_rank n][run_prio n]
struct OrderTabLayout { size_t o_rq, o_st, o_rk, o_pr, bytes; };
inline OrderTabLayout order_tab_layout(uint32_t n) {
    OrderTabLayout l; l.o_rq = 16; l.o_st = l.o_rq + (size_t)n * 4; l.o_rk = l.o_st + (size_t)n * 4; l.o_pr = (l.o_rk + (size_t)n * 4 + 7) & ~(size_t)7; l.bytes = l.o_pr + (size_t)n * 8 + 16;
    return l;
}

// The passes of the view's radix sort over n_digits 8-bit digits (the first PRIO_DIGITS of ~priority, the rest of rq), from the digit histogram
// gh[dg * 256 + d] of n_live slots: every digit that is not constant over the live set, least significant first.
static const uint32_t PRIO_DIGITS = 8, MAX_DIGITS = 16;
struct Passes {
    uint32_t n = 0, digit[MAX_DIGITS] = {}, level_after = 0;  // level_after: the level ranks are read off the permutation after this pass, the last one on a priority digit (no such pass: one priority, any order)
    uint32_t mask() const { uint32_t m = 0; for (uint32_t i = 0; i < n; i++) m |= 1u << digit[i]; return m; }
};
inline Passes order_passes(const uint32_t *gh, uint32_t n_digits, uint32_t n_live) {
    Passes p;
    for (uint32_t dg = 0; dg < n_digits && dg < MAX_DIGITS; dg++) {
        bool constant = false;
        for (uint32_t d = 0; d < 256 && !constant; d++) constant = gh[dg * 256 + d] == n_live;
        if (!constant) p.digit[p.n++] = dg;
    }
    if (p.n == 0) p.digit[p.n++] = 0;  // (one pass still drops the tombstones)
    for (uint32_t i = 0; i < p.n; i++) if (p.digit[i] < PRIO_DIGITS) p.level_after = i;
    return p;
}

// The run table `tab` (order_tab_layout(n) bytes) of a view of n live slots over Q requests into sc's run form.  0, or HQTICK_E_DEVICE with *why set: the
// table is device output and nothing of it is trusted before it is checked.
inline int decode_runs(const uint8_t *tab, uint32_t n, uint32_t Q, Table *sc, const char **why) {
    const OrderTabLayout tl = order_tab_layout(n);
    const uint32_t nr = reinterpret_cast<const uint32_t *>(tab)[0], nl = reinterpret_cast<const uint32_t *>(tab)[1];
    if (nr == 0 || nr > n || nl == 0 || nl > nr) { *why = "ordered view: inconsistent run table"; return HQTICK_E_DEVICE; }
    const uint32_t *rrq = reinterpret_cast<const uint32_t *>(tab + tl.o_rq), *rst = reinterpret_cast<const uint32_t *>(tab + tl.o_st), *rrk = reinterpret_cast<const uint32_t *>(tab + tl.o_rk);
    const uint64_t *rpr = reinterpret_cast<const uint64_t *>(tab + tl.o_pr);
    sc->run_off.assign(Q + 1, 0);
    sc->run_start.assign(rst, rst + nr); sc->run_level.assign(rrk, rrk + nr); sc->run_prio.assign(rpr, rpr + nr);
    sc->run_cnt.resize(nr); sc->run_group.resize(nr);
    for (uint32_t r = 0; r < nr; r++) {
        if (rrq[r] >= Q || (r && rrq[r] < rrq[r - 1])) { *why = "ordered view: runs out of request order"; return HQTICK_E_DEVICE; }
        sc->run_cnt[r] = (r + 1 < nr ? rst[r + 1] : n) - rst[r]; sc->run_group[r] = r; sc->run_off[rrq[r] + 1]++;
    }
    for (uint32_t q = 0; q < Q; q++) sc->run_off[q + 1] += sc->run_off[q];
    sc->L = nl; sc->G = nr;
    return 0;
}

// The slices of the dense scan over N slots and G groups: a wavefront owns tasks_per_wave contiguous slots, K1b scans one row of n_waves entries per group.
struct Geom { uint32_t tasks_per_wave, n_waves, waves_per_block, tab_stride; };
inline Geom wave_geometry(uint64_t N, uint32_t G, uint32_t tpw_hint, uint32_t max_groups_4w) {
    Geom g;
    g.waves_per_block = G <= max_groups_4w ? 4 : 1;
    uint64_t tpw = tpw_hint ? tpw_hint : 256;
    while (((N + tpw - 1) / tpw) * G > (1ull << 24)) tpw *= 2;  // keep the per-slice table under 64 MiB
    if (!tpw_hint) while ((N + tpw - 1) / tpw > 32768) tpw *= 2;  // and the rows K1b scans short: one wavefront scans a row of n_waves entries, 4096 per
                                                                   // step (64 M tasks at 256 per slice: 250 k entries = 400 us for K1b against 160 us for K1;
                                                                   // 32 k slices of 2048 tasks keep K1 / K4 at 8 k workgroups and K1b at 8 steps)
    g.tasks_per_wave = (uint32_t)tpw; g.n_waves = (uint32_t)((N + tpw - 1) / tpw); g.tab_stride = (g.n_waves + 15u) & ~15u;
    return g;
}

}  // namespace hqscan
