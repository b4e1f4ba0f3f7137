// Grouping of a cancel batch by worker row (hqtick_cancel_tasks): the phases of its kernels and their execution on the host.
//
// Input: route[n], the worker row every batch position is routed to (NONE: no message).  Output: the CancelTasks lists as a CSR — the rows that get a
// message in ascending order, their offsets, and the task ids grouped by row and, inside a row, in ascending batch position.
//
// It is a stable LSD radix sort of (key = row, NONE as W; value = batch position) with 8-bit digits, ceil(log256(W + 1)) passes.  A pass is three kernels
// with a kernel boundary between them: per-tile digit counts, a per-digit scan of those counts, a stable scatter.  Inside a tile (TILE positions of one
// workgroup: ITEMS rounds of BLOCK threads) the rank of a position is the count of its digit in the (round, wavefront) slots before its own — wave-private
// LDS counters, written by one lane per digit and never added to atomically — plus its rank among the equal digits of its wavefront (match-any).  No output
// position depends on the order in which anything arrives: the rule of order.hip.  Two more kernels mark the row boundaries of the sorted keys and write
// the compact lists.
//
// As in wire_core.h a kernel is a fixed sequence of PHASES separated by workgroup barriers: plain functions of (arguments, LDS block, workgroup, tid),
// templated on how a wavefront matches equal digits — DevMatch (cancel.hip: one __ballot per digit bit) or HostMatch (the lanes in a loop over the LDS
// block).  group_on_host runs them one emulated thread after the other in any of three thread orders, every array in a heap block of its exact size.
#pragma once
#include <cstdint>
#include <cstring>
#include <new>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HQC_HD __host__ __device__ inline
#else
#define HQC_HD inline
#endif

namespace hqcancel {

constexpr int BLOCK = 256, WAVE = 64, WAVES = BLOCK / WAVE, ITEMS = 4;
constexpr uint32_t TILE = BLOCK * ITEMS, RADIX = 256, SLOTS = ITEMS * WAVES;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint16_t NO_DIGIT = 0xFFFFu;  // a position of the tile behind n
static_assert(RADIX == (uint32_t)BLOCK, "one thread per digit in the counter phases");

HQC_HD uint32_t n_tiles_of(uint32_t n) { return n / TILE + (n % TILE ? 1u : 0u); }
// digits the keys 0 .. W need
HQC_HD uint32_t passes_of(uint32_t W) { uint32_t p = 1; for (uint32_t v = W >> 8; v; v >>= 8) p++; return p; }

struct SortArgs {
    uint32_t n, W, shift, n_tiles;
    const uint32_t *route;            // the first pass reads the routes (key = row, NONE and anything else not below W: W; value = position) ...
    const uint32_t *key_in, *pos_in;  // ... a later one the pair the pass before it wrote
    uint32_t *key_out, *pos_out;
    uint32_t *cnt;                    // [n_tiles x RADIX], tile-major (the 256 threads of a workgroup touch one row: coalesced in all three kernels): the tile's
                                      // count of a digit; after the scan where the tile's first key of that digit goes
};
struct SortLds { uint16_t dig[TILE]; uint32_t hist[SLOTS][RADIX]; };  // 2 KB + 16 KB

HQC_HD uint32_t key_of(const SortArgs &a, uint32_t j) {
    if (!a.route) return a.key_in[j];
    const uint32_t r = a.route[j];
    return r < a.W ? r : a.W;
}
HQC_HD uint32_t popc64(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(m);
#else
    return (uint32_t)__builtin_popcountll(m);
#endif
}

// the lanes of the wavefront of tile position e whose digit equals its own, as a bit mask: the lanes in a loop
struct HostMatch {
    static uint64_t match(const SortLds &l, uint32_t e, uint32_t d) {
        const uint32_t e0 = e & ~(uint32_t)(WAVE - 1);
        uint64_t m = 0;
        for (uint32_t k = 0; k < (uint32_t)WAVE; k++) if (l.dig[e0 + k] == d) m |= 1ull << k;
        return m;
    }
};

// ---- phases of the count and scatter kernels (workgroup `tile`, thread tid) ----
HQC_HD void sort_p_zero(SortLds &l, int tid) {
    for (uint32_t s = 0; s < SLOTS; s++) l.hist[s][tid] = 0;
}
HQC_HD void sort_p_digits(const SortArgs &a, SortLds &l, uint32_t tile, int tid) {
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t e = (uint32_t)(k * BLOCK + tid);
        const uint64_t j = (uint64_t)tile * TILE + e;
        l.dig[e] = j < a.n ? (uint16_t)((key_of(a, (uint32_t)j) >> a.shift) & 0xFFu) : NO_DIGIT;
    }
}
// the count of every digit in every (round, wavefront) slot: the lowest lane of a group of equal digits writes it
template <class M> HQC_HD void sort_p_hist(SortLds &l, int tid) {
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t e = (uint32_t)(k * BLOCK + tid), d = l.dig[e], lane = (uint32_t)tid & (WAVE - 1);
        const uint64_t m = M::match(l, e, d);
        if (d != NO_DIGIT && (m & ((1ull << lane) - 1ull)) == 0) l.hist[(uint32_t)k * WAVES + (uint32_t)tid / WAVE][d] = popc64(m);
    }
}
HQC_HD void count_p_out(const SortArgs &a, SortLds &l, uint32_t tile, int tid) {
    uint32_t c = 0;
    for (uint32_t s = 0; s < SLOTS; s++) c += l.hist[s][tid];
    a.cnt[(size_t)tile * RADIX + tid] = c;
}
// the slots' counts become where the slot's first key of the digit goes
HQC_HD void scatter_p_base(const SortArgs &a, SortLds &l, uint32_t tile, int tid) {
    uint32_t run = a.cnt[(size_t)tile * RADIX + tid];
    for (uint32_t s = 0; s < SLOTS; s++) { const uint32_t c = l.hist[s][tid]; l.hist[s][tid] = run; run += c; }
}
template <class M> HQC_HD void scatter_p_move(const SortArgs &a, SortLds &l, uint32_t tile, int tid) {
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t e = (uint32_t)(k * BLOCK + tid), d = l.dig[e], lane = (uint32_t)tid & (WAVE - 1);
        const uint64_t m = M::match(l, e, d);
        if (d == NO_DIGIT) continue;
        const uint32_t j = tile * TILE + e, dst = l.hist[(uint32_t)k * WAVES + (uint32_t)tid / WAVE][d] + popc64(m & ((1ull << lane) - 1ull));
        a.key_out[dst] = key_of(a, j);
        a.pos_out[dst] = a.route ? j : a.pos_in[j];
    }
}

// ---- the scan kernel, one workgroup: thread d owns digit d's n_tiles counts (a column of the table; the workgroup walks it row by row); the digits before it
// come through the LDS block.  The order of the sums is digit-major: every tile's keys of digit d lie before any key of digit d + 1 ----
struct ScanLds { uint32_t part[RADIX], base[RADIX]; };
HQC_HD void scan_p1(const SortArgs &a, ScanLds &l, int tid) {
    uint32_t s = 0;
    for (uint32_t t = 0; t < a.n_tiles; t++) s += a.cnt[(size_t)t * RADIX + tid];
    l.part[tid] = s;
}
HQC_HD void scan_p2(ScanLds &l, int tid) {
    if (tid != 0) return;
    uint32_t run = 0;
    for (uint32_t d = 0; d < RADIX; d++) { l.base[d] = run; run += l.part[d]; }
}
HQC_HD void scan_p3(const SortArgs &a, ScanLds &l, int tid) {
    uint32_t run = l.base[tid], t = 0;
    for (; t + 8 <= a.n_tiles; t += 8) {  // eight loads in flight, then eight stores: the walk is bound by the latency of its loads
        uint32_t c[8];
        for (uint32_t k = 0; k < 8; k++) c[k] = a.cnt[(size_t)(t + k) * RADIX + tid];
        for (uint32_t k = 0; k < 8; k++) { a.cnt[(size_t)(t + k) * RADIX + tid] = run; run += c[k]; }
    }
    for (; t < a.n_tiles; t++) { uint32_t *p = &a.cnt[(size_t)t * RADIX + tid]; const uint32_t c = *p; *p = run; run += c; }
}

// ---- the last pass: row boundaries of the sorted keys, then the compact lists ----
struct FinArgs {
    uint32_t n, W;
    const uint32_t *key, *pos;  // sorted
    const uint64_t *id;         // the batch
    const uint32_t *wid;        // worker ids in row order [W]
    const uint32_t *route;      // [n]
    const uint8_t *kind;        // [n] (nullptr: no routes wanted)
    uint32_t *start;            // [W] scratch, NONE on entry: where the row's ids begin
    uint64_t *out_id;           // [n]: the first hdr[1] are the messages' ids
    uint32_t *out_wid, *out_off;  // [W], [W + 1]: the first hdr[0] (+ 1) are the rows with a message
    uint32_t *hdr;              // [2]: rows with a message, ids in the messages
    uint32_t *route_wid;        // [n] worker id per batch position (no_worker: none)
    uint8_t *route_kind;        // [n]
    uint32_t no_worker;
};
HQC_HD void fin_mark(const FinArgs &a, uint64_t g) {
    if (g >= a.n) return;
    const uint32_t j = (uint32_t)g, key = a.key[j];
    if (key < a.W) {
        a.out_id[j] = a.id[a.pos[j]];
        if (j == 0 || a.key[j - 1] != key) a.start[key] = j;
    }
    if (a.kind) {
        const uint32_t r = a.route[j];
        a.route_wid[j] = r < a.W ? a.wid[r] : a.no_worker;
        a.route_kind[j] = a.kind[j];
    }
}
HQC_HD void run_of(uint32_t n, int tid, uint32_t &lo, uint32_t &hi) {
    lo = (uint32_t)((uint64_t)n * (uint32_t)tid / BLOCK);
    hi = (uint32_t)((uint64_t)n * ((uint32_t)tid + 1) / BLOCK);
}
struct FinLds { uint32_t part[BLOCK], base[BLOCK]; };
HQC_HD void fin_p1(const FinArgs &a, FinLds &l, int tid) {
    uint32_t lo, hi, c = 0;
    run_of(a.W, tid, lo, hi);
    for (uint32_t r = lo; r < hi; r++) c += a.start[r] != NONE;
    l.part[tid] = c;
}
HQC_HD void fin_p2(const FinArgs &a, FinLds &l, int tid) {
    if (tid != 0) return;
    uint32_t run = 0;
    for (int k = 0; k < BLOCK; k++) { l.base[k] = run; run += l.part[k]; }
    uint32_t lo = 0, hi = a.n;  // the keys below W: the messages' ids
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a.key[mid] < a.W) lo = mid + 1; else hi = mid; }
    a.hdr[0] = run; a.hdr[1] = lo;
    a.out_off[run] = lo;
}
HQC_HD void fin_p3(const FinArgs &a, FinLds &l, int tid) {
    uint32_t lo, hi, k = l.base[tid];
    run_of(a.W, tid, lo, hi);
    for (uint32_t r = lo; r < hi; r++)
        if (a.start[r] != NONE) { a.out_wid[k] = a.wid[r]; a.out_off[k] = a.start[r]; k++; }
}

// where the sort's scratch sits in one block of u32: [key0 n][pos0 n][key1 n][pos1 n][cnt n_tiles x RADIX][start W]
struct Scratch { size_t key0, pos0, key1, pos1, cnt, start, total; };
HQC_HD Scratch scratch_of(uint32_t n, uint32_t W) {
    Scratch s{};
    s.key0 = 0; s.pos0 = n; s.key1 = 2 * (size_t)n; s.pos1 = 3 * (size_t)n; s.cnt = 4 * (size_t)n; s.start = s.cnt + (size_t)RADIX * n_tiles_of(n); s.total = s.start + W;
    return s;
}

// ---- host execution (debug hook, sanitizer program): a loop end = a workgroup barrier; order 0 ascending, 1 descending (workgroups too), 2 scattered ----
inline bool group_on_host(uint32_t n, uint32_t W, const uint32_t *route, const uint64_t *id, const uint32_t *wid, int order, uint32_t *n_workers, uint32_t *n_ids,
                          uint32_t *out_wid, uint32_t *out_off, uint64_t *out_id) {
    int seq[BLOCK];
    for (int i = 0; i < BLOCK; i++) seq[i] = order == 1 ? BLOCK - 1 - i : order == 2 ? (i * 77 + 13) % BLOCK : i;  // 77 is coprime to 256
    const uint32_t nt = n_tiles_of(n);
    // every array a heap block of its exact size
    uint32_t *key[2] = {new (std::nothrow) uint32_t[n], new (std::nothrow) uint32_t[n]}, *pos[2] = {new (std::nothrow) uint32_t[n], new (std::nothrow) uint32_t[n]};
    uint32_t *cnt = new (std::nothrow) uint32_t[(size_t)RADIX * nt], *start = new (std::nothrow) uint32_t[W], hdr[2] = {0, 0};
    SortLds *sl = new (std::nothrow) SortLds;
    ScanLds *cl = new (std::nothrow) ScanLds;
    FinLds *fl = new (std::nothrow) FinLds;
    const bool ok = key[0] && key[1] && pos[0] && pos[1] && cnt && start && sl && cl && fl;
#define HQC_ALL(stmt) for (int q = 0; q < BLOCK; q++) { const int tid = seq[q]; (void)tid; stmt; }
    if (ok) {
        for (uint32_t w = 0; w < W; w++) start[w] = NONE;
        const uint32_t passes = passes_of(W);
        int cur = 0;
        for (uint32_t p = 0; p < passes; p++) {
            SortArgs a{};
            a.n = n; a.W = W; a.shift = p * 8; a.n_tiles = nt; a.cnt = cnt;
            if (p == 0) a.route = route; else { a.key_in = key[cur]; a.pos_in = pos[cur]; }
            const int nxt = p == 0 ? 0 : cur ^ 1;
            a.key_out = key[nxt]; a.pos_out = pos[nxt];
            for (uint32_t k = 0; k < nt; k++) {
                const uint32_t tile = order == 1 ? nt - 1 - k : k;
                HQC_ALL(sort_p_zero(*sl, tid)) HQC_ALL(sort_p_digits(a, *sl, tile, tid)) HQC_ALL(sort_p_hist<HostMatch>(*sl, tid)) HQC_ALL(count_p_out(a, *sl, tile, tid))
            }
            HQC_ALL(scan_p1(a, *cl, tid)) HQC_ALL(scan_p2(*cl, tid)) HQC_ALL(scan_p3(a, *cl, tid))
            for (uint32_t k = 0; k < nt; k++) {
                const uint32_t tile = order == 1 ? nt - 1 - k : k;
                HQC_ALL(sort_p_zero(*sl, tid)) HQC_ALL(sort_p_digits(a, *sl, tile, tid)) HQC_ALL(sort_p_hist<HostMatch>(*sl, tid)) HQC_ALL(scatter_p_base(a, *sl, tile, tid))
                HQC_ALL(scatter_p_move<HostMatch>(a, *sl, tile, tid))
            }
            cur = nxt;
        }
        FinArgs f{};
        f.n = n; f.W = W; f.key = key[cur]; f.pos = pos[cur]; f.id = id; f.wid = wid; f.route = route; f.start = start;
        f.out_id = out_id; f.out_wid = out_wid; f.out_off = out_off; f.hdr = hdr; f.no_worker = NONE;
        const uint32_t nb = (n + BLOCK - 1) / BLOCK;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t blk = order == 1 ? nb - 1 - k : k;
            HQC_ALL(fin_mark(f, (uint64_t)blk * BLOCK + (uint32_t)tid))
        }
        HQC_ALL(fin_p1(f, *fl, tid)) HQC_ALL(fin_p2(f, *fl, tid)) HQC_ALL(fin_p3(f, *fl, tid))
        *n_workers = hdr[0]; *n_ids = hdr[1];
    }
#undef HQC_ALL
    delete[] key[0]; delete[] key[1]; delete[] pos[0]; delete[] pos[1]; delete[] cnt; delete[] start;
    delete sl; delete cl; delete fl;
    return ok;
}

}  // namespace hqcancel
