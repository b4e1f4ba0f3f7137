// The resident task-attribute table of the wire encoder (include/hqwire.h, hqwire_table_*): the phases of its kernels and its host side.
//
// As in wire_core.h every kernel is a fixed sequence of PHASES separated by workgroup barriers, plain functions of (arguments, LDS block, workgroup,
// tid) compiled for the device (kernels in wire_table.hip) and for the host, where run_kernel_on_host executes them one emulated thread after the other in
// any of three thread orders.  The host side is one class, Table, on a small memory-and-launch Backend: HIP buffers and launches (wire_table.hip), or host
// memory and emulated phases (HostBackend below: the debug hook of include/hqtick_debug.h and tools/wire_table_asan.cpp, which needs no HIP at all).
//
// Layout: the seven columns of hqwire_tables (37 B per row) plus the entry blob, twice (the set in use and a spare one that compaction, merge and growth
// write into), a liveness bitmap of one bit per row, and the configuration arrays.  Bits of rows at or behind n_rows mean nothing.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "wire_core.h"

namespace hqwtab {

using hqwire::BLOCK;
using hqwire::GROUPS;
using hqwire::GSIZE;
constexpr uint32_t TILE = HQWIRE_TABLE_TILE;
static_assert(TILE == (uint32_t)BLOCK, "one thread per row of a tile");
constexpr uint32_t TILE_WORDS = TILE / 32;
constexpr uint64_t RESERVED_ID = 0xFFFFFFFFFFFFFFFEull;  // ids from here on are reserved (find_row's +inf, the graph's sentinels)
constexpr uint64_t MAX_ROWS = 0xFFFFFFFFull;             // row indices are 32 bits in the encoder, 0xFFFFFFFF = none

enum Kernel { K_APPEND = 0, K_CHECK, K_REMOVE, K_SETINST, K_COUNT, K_SCAN, K_MOVE, K_MERGE };
enum Res { R_FLAG = 0, R_HIT, R_BYTES, R_UNKNOWN, R_ROWS, R_BLOB, R_LAST, R_N = 8 };  // the result block, u64 each, in HBM

struct Cols {
    uint64_t *id; uint32_t *rq; uint32_t *inst; uint64_t *prio; uint32_t *cfg; uint8_t *some; uint64_t *off; uint8_t *blob;
    uint32_t *live;  // one bit per row
};
struct Batch {  // a delta batch in the device staging buffer
    const uint64_t *id, *prio, *off;
    const uint32_t *rq, *inst, *cfg, *val;
    const uint8_t *some, *blob;  // blob[0] = the byte at off[0]
};
struct TArgs {
    Cols cur, dst;
    Batch b;
    uint64_t n_rows, n_blob;  // physical rows / blob bytes of cur
    uint64_t n, nb;           // rows (ids) / blob bytes of the batch
    uint64_t last_id;         // highest resident id, dead rows included
    uint32_t has_last, n_configs, n_tiles, with_values;
    uint64_t *res;            // [R_N]
    uint32_t *tile_rows, *tile_row_base;  // [n_tiles] live rows of a tile / of the tiles before it
    uint64_t *tile_bytes, *tile_byte_base;
};

// where the arrays of a batch of n rows and nb blob bytes sit in the staging buffers (8-byte aligned columns first)
struct Stage { uint64_t id, prio, off, rq, inst, cfg, some, blob, total; };
HQW_HD Stage stage_of(uint64_t n, uint64_t nb) {
    Stage s{};
    s.id = 0; s.prio = 8 * n; s.off = 16 * n; s.rq = 24 * n + 8; s.inst = s.rq + 4 * n; s.cfg = s.inst + 4 * n; s.some = s.cfg + 4 * n;
    s.blob = (s.some + n + 15) & ~15ull;
    s.total = s.blob + nb;
    return s;
}

// ---- global-memory atomics (plain on the host: one emulated thread at a time) -----------------------------------------------------------------
HQW_HD uint32_t g_and(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAnd(p, v);
#else
    const uint32_t old = *p;
    *p = old & v;
    return old;
#endif
}
HQW_HD void g_inc(uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, 1u);
#else
    *p += 1;
#endif
}
HQW_HD uint32_t popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}
// Three counters of the result block, summed over the wavefront first: one atomic per wavefront and counter, in HBM.  Every lane of the wavefront calls it.
HQW_HD void wave_add(uint64_t *res, uint64_t hit, uint64_t bytes, uint64_t unknown) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int o = 32; o; o >>= 1) {
        hit += __shfl_down((unsigned long long)hit, o);
        bytes += __shfl_down((unsigned long long)bytes, o);
        unknown += __shfl_down((unsigned long long)unknown, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (hit) atomicAdd((unsigned long long *)&res[R_HIT], (unsigned long long)hit);
        if (bytes) atomicAdd((unsigned long long *)&res[R_BYTES], (unsigned long long)bytes);
        if (unknown) atomicAdd((unsigned long long *)&res[R_UNKNOWN], (unsigned long long)unknown);
    }
#else
    res[R_HIT] += hit; res[R_BYTES] += bytes; res[R_UNKNOWN] += unknown;
#endif
}

HQW_HD uint64_t lower_bound(const uint64_t *v, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the encoder's row search (wire_core.h: find_row) on the table's id column: dead rows are found like live ones
HQW_HD uint32_t row_of(const TArgs &a, uint64_t id) {
    hqwire::Args f{};
    f.t.n_tasks = a.n_rows;
    f.t.task_id = a.cur.id;
    return hqwire::find_row(f, id);
}
HQW_HD bool is_live(const TArgs &a, uint64_t row) { return row < a.n_rows && ((a.cur.live[row >> 5] >> (row & 31)) & 1u); }
// the bitmap word w of cur with the bits of rows at or behind n_rows cleared (a word wholly behind n_rows is not read)
HQW_HD uint32_t live_word(const TArgs &a, uint64_t w) {
    if (w * 32 >= a.n_rows) return 0;
    const uint32_t v = a.cur.live[w];
    const uint64_t left = a.n_rows - w * 32;
    return left >= 32 ? v : v & ((1u << left) - 1u);
}
// what a batch row must satisfy by itself (ascending ids apart)
HQW_HD bool row_bad(const TArgs &a, uint64_t j) {
    const uint64_t o0 = a.b.off[j], o1 = a.b.off[j + 1];
    return a.b.id[j] >= RESERVED_ID || a.b.cfg[j] >= a.n_configs || o1 < o0 || (!a.b.some[j] && o1 != o0);
}

// =========================================================================================================================================
// append: one thread per batch row validates it against its predecessor (row 0: against the last resident id) and writes the seven column
// tails, entry_off shifted by the blob length so far; all threads of the grid move the blob bytes as one range.  Rows behind n_rows are invisible:
// a refused batch (R_FLAG) needs no undo.
// =========================================================================================================================================
HQW_HD void append_p(const TArgs &a, uint64_t g) {
    if (g < a.n) {
        const uint64_t id = a.b.id[g];
        bool bad = row_bad(a, g);
        bad = bad || (g == 0 ? (a.has_last && id <= a.last_id) : id <= a.b.id[g - 1]);
        const uint64_t r = a.n_rows + g;
        a.cur.id[r] = id;
        a.cur.rq[r] = a.b.rq[g];
        a.cur.inst[r] = a.b.inst[g];
        a.cur.prio[r] = a.b.prio[g];
        a.cur.cfg[r] = a.b.cfg[g];
        a.cur.some[r] = a.b.some[g] ? 1 : 0;
        a.cur.off[r + 1] = a.n_blob + (a.b.off[g + 1] - a.b.off[0]);  // (off[n_rows] == n_blob already)
        if (bad) a.res[R_FLAG] = 1;  // the same value from every thread that stores it
    }
}
// (the blob range by the threads of the grid, at most 2^20 of them: 16 bytes per thread and step)
HQW_HD void append_blob(const TArgs &a, uint64_t g, uint64_t n_threads) {
    const uint64_t movers = n_threads < (1u << 20) ? n_threads : (1u << 20);
    if (g < movers) hqwire::copy_bytes(a.cur.blob + a.n_blob, a.b.blob, a.nb, (int)g, (int)movers);
}

// merge add, before anything moves: the batch against itself and against the live rows (a dead row's id may come back)
HQW_HD void check_p(const TArgs &a, uint64_t g) {
    if (g >= a.n) return;
    const uint64_t id = a.b.id[g];
    bool bad = row_bad(a, g) || (g > 0 && id <= a.b.id[g - 1]);
    if (!bad) {
        const uint32_t row = row_of(a, id);
        bad = row != hqwire::NONE && is_live(a, row);
    }
    if (bad) a.res[R_FLAG] = 1;
}

// remove: the ONE thread that clears a row's bit counts the row and its blob bytes -- an id listed twice, or removed before, is "unknown"
HQW_HD void remove_p(const TArgs &a, uint64_t g) {
    uint64_t hit = 0, bytes = 0, unknown = 0;
    if (g < a.n) {
        const uint32_t row = row_of(a, a.b.id[g]);
        unknown = 1;
        if (row != hqwire::NONE) {
            const uint32_t bit = 1u << (row & 31);
            if (g_and(&a.cur.live[row >> 5], ~bit) & bit) {
                hit = 1; unknown = 0;
                bytes = a.cur.off[row + 1] - a.cur.off[row];
            }
        }
    }
    wave_add(a.res, hit, bytes, unknown);
}
HQW_HD void setinst_p(const TArgs &a, uint64_t g) {
    uint64_t hit = 0, unknown = 0;
    if (g < a.n) {
        const uint32_t row = row_of(a, a.b.id[g]);
        if (row != hqwire::NONE && is_live(a, row)) {
            hit = 1;
            if (a.with_values) a.cur.inst[row] = a.b.val[g];
            else g_inc(&a.cur.inst[row]);
        } else unknown = 1;
    }
    wave_add(a.res, hit, 0, unknown);
}

// =========================================================================================================================================
// compaction: (1) per tile its live rows (popcount of the bitmap words) and live blob bytes, (2) one workgroup scans the tiles, (3) per tile the live
// rows move to tile base + rank inside the tile (popcounts again), their blob bytes to tile byte base + prefix inside the tile.  No output position
// depends on the order of anything.
// =========================================================================================================================================
struct MoveLds {
    uint64_t len[BLOCK];             // blob bytes this thread's row moves (0: dead row / no bytes)
    uint64_t grp[GROUPS], gbase[GROUPS];
    const uint8_t *src[BLOCK];
    uint8_t *dst[BLOCK];
};
HQW_HD void tile_p1(const TArgs &a, MoveLds &l, uint32_t t, int tid) {
    const uint64_t r = (uint64_t)t * TILE + (uint32_t)tid;
    l.len[tid] = is_live(a, r) ? a.cur.off[r + 1] - a.cur.off[r] : 0;
}
HQW_HD void tile_p2a(const TArgs &, MoveLds &l, uint32_t, int tid) {
    if (tid >= GROUPS) return;
    uint64_t s = 0;
    for (int k = tid * GSIZE; k < (tid + 1) * GSIZE; k++) s += l.len[k];
    l.grp[tid] = s;
}
HQW_HD void count_p3(const TArgs &a, MoveLds &l, uint32_t t, int tid) {
    if (tid != 0) return;
    uint64_t bytes = 0;
    uint32_t rows = 0;
    for (int g = 0; g < GROUPS; g++) bytes += l.grp[g];
    for (uint32_t w = 0; w < TILE_WORDS; w++) rows += popc(live_word(a, (uint64_t)t * TILE_WORDS + w));
    a.tile_rows[t] = rows;
    a.tile_bytes[t] = bytes;
}

struct ScanLds { uint64_t part_b[BLOCK], base_b[BLOCK], grp_b[GROUPS], gbase_b[GROUPS]; uint32_t part_r[BLOCK], base_r[BLOCK], grp_r[GROUPS], gbase_r[GROUPS]; };
HQW_HD void scan_p1(const TArgs &a, ScanLds &l, int tid) {
    uint32_t lo, hi, r = 0;
    hqwire::run_of(a.n_tiles, tid, lo, hi);
    uint64_t b = 0;
    for (uint32_t t = lo; t < hi; t++) { r += a.tile_rows[t]; b += a.tile_bytes[t]; }
    l.part_r[tid] = r; l.part_b[tid] = b;
}
HQW_HD void scan_p2a(const TArgs &, ScanLds &l, int tid) {
    if (tid >= GROUPS) return;
    uint32_t r = 0;
    uint64_t b = 0;
    for (int k = tid * GSIZE; k < (tid + 1) * GSIZE; k++) { r += l.part_r[k]; b += l.part_b[k]; }
    l.grp_r[tid] = r; l.grp_b[tid] = b;
}
HQW_HD void scan_p2b(const TArgs &a, ScanLds &l, int tid) {
    if (tid != 0) return;
    uint32_t r = 0;
    uint64_t b = 0;
    for (int g = 0; g < GROUPS; g++) { l.gbase_r[g] = r; l.gbase_b[g] = b; r += l.grp_r[g]; b += l.grp_b[g]; }
    a.res[R_ROWS] = r;
    a.res[R_BLOB] = b;
    a.dst.off[r] = b;  // the closing offset of the compacted table
}
HQW_HD void scan_p2c(const TArgs &, ScanLds &l, int tid) {
    uint32_t r = l.gbase_r[tid / GSIZE];
    uint64_t b = l.gbase_b[tid / GSIZE];
    for (int k = (tid / GSIZE) * GSIZE; k < tid; k++) { r += l.part_r[k]; b += l.part_b[k]; }
    l.base_r[tid] = r; l.base_b[tid] = b;
}
HQW_HD void scan_p3(const TArgs &a, ScanLds &l, int tid) {
    uint32_t lo, hi, r = l.base_r[tid];
    hqwire::run_of(a.n_tiles, tid, lo, hi);
    uint64_t b = l.base_b[tid];
    for (uint32_t t = lo; t < hi; t++) {
        a.tile_row_base[t] = r; a.tile_byte_base[t] = b;
        r += a.tile_rows[t]; b += a.tile_bytes[t];
    }
}

HQW_HD void move_p2b(const TArgs &, MoveLds &l, uint32_t, int tid) {
    if (tid != 0) return;
    uint64_t b = 0;
    for (int g = 0; g < GROUPS; g++) { l.gbase[g] = b; b += l.grp[g]; }
}
HQW_HD bool tile_full(const TArgs &a, uint32_t t) {  // every row of the tile alive: rows and blob bytes move as one range
    const uint64_t r0 = (uint64_t)t * TILE, in_tile = a.n_rows - r0 < TILE ? a.n_rows - r0 : TILE;
    return a.tile_rows[t] == in_tile;
}
HQW_HD void move_p3(const TArgs &a, MoveLds &l, uint32_t t, int tid) {
    const uint64_t r = (uint64_t)t * TILE + (uint32_t)tid;
    l.src[tid] = nullptr; l.dst[tid] = nullptr;
    if (!is_live(a, r)) return;
    uint64_t pre = l.gbase[tid / GSIZE];
    for (int k = (tid / GSIZE) * GSIZE; k < tid; k++) pre += l.len[k];
    uint32_t rank = popc(live_word(a, r >> 5) & ((1u << (r & 31)) - 1u));
    for (uint64_t w = (uint64_t)t * TILE_WORDS; w < (r >> 5); w++) rank += popc(live_word(a, w));
    const uint64_t d = (uint64_t)a.tile_row_base[t] + rank, bpos = a.tile_byte_base[t] + pre;
    a.dst.id[d] = a.cur.id[r];
    a.dst.rq[d] = a.cur.rq[r];
    a.dst.inst[d] = a.cur.inst[r];
    a.dst.prio[d] = a.cur.prio[r];
    a.dst.cfg[d] = a.cur.cfg[r];
    a.dst.some[d] = a.cur.some[r];
    a.dst.off[d] = bpos;
    if (d + 1 == a.res[R_ROWS]) a.res[R_LAST] = a.cur.id[r];  // (R_ROWS: written by the scan kernel before this one started)
    l.src[tid] = a.cur.blob + a.cur.off[r];
    l.dst[tid] = a.dst.blob + bpos;
}
// blob bytes with lanes cooperating: a full tile as one range by the whole workgroup; otherwise every wavefront takes the rows of its 64 threads in turn
HQW_HD void blob_p(MoveLds &l, int tid) {
    const int w0 = (tid / 64) * 64;
    for (int k = w0; k < w0 + 64; k++)
        if (l.len[k]) hqwire::copy_bytes(l.dst[k], l.src[k], l.len[k], tid % 64, 64);
}
HQW_HD void move_p4(const TArgs &a, MoveLds &l, uint32_t t, int tid) {
    if (tile_full(a, t)) {
        if (a.tile_bytes[t]) hqwire::copy_bytes(a.dst.blob + a.tile_byte_base[t], a.cur.blob + a.cur.off[(uint64_t)t * TILE], a.tile_bytes[t], tid, BLOCK);
    } else blob_p(l, tid);
}

// =========================================================================================================================================
// merge of two dense ascending tables (cur: every row alive; the batch) into dst: old row i goes to i + lower_bound(batch, id_i), batch row j to
// j + lower_bound(old, id_j); blob positions follow the same way from the two entry_off arrays.  An equal id sets R_FLAG (dst is then dropped).
// One thread per row of either table, workgroup by workgroup; the rows' blob bytes in a second phase.
// =========================================================================================================================================
HQW_HD void merge_p1(const TArgs &a, MoveLds &l, uint32_t blk, int tid) {
    const uint64_t g = (uint64_t)blk * BLOCK + (uint32_t)tid;
    l.len[tid] = 0; l.src[tid] = nullptr; l.dst[tid] = nullptr;
    if (g == 0) {
        a.dst.off[a.n_rows + a.n] = a.n_blob + a.nb;
        const uint64_t lb = a.b.id[a.n - 1];
        a.res[R_LAST] = (a.n_rows && a.cur.id[a.n_rows - 1] > lb) ? a.cur.id[a.n_rows - 1] : lb;
    }
    if (g < a.n_rows) {
        const uint64_t id = a.cur.id[g], k = lower_bound(a.b.id, a.n, id);
        if (k < a.n && a.b.id[k] == id) a.res[R_FLAG] = 1;
        const uint64_t d = g + k, bpos = a.cur.off[g] + (a.b.off[k] - a.b.off[0]);
        a.dst.id[d] = id;
        a.dst.rq[d] = a.cur.rq[g];
        a.dst.inst[d] = a.cur.inst[g];
        a.dst.prio[d] = a.cur.prio[g];
        a.dst.cfg[d] = a.cur.cfg[g];
        a.dst.some[d] = a.cur.some[g];
        a.dst.off[d] = bpos;
        l.len[tid] = a.cur.off[g + 1] - a.cur.off[g];
        l.src[tid] = a.cur.blob + a.cur.off[g];
        l.dst[tid] = a.dst.blob + bpos;
    } else if (g < a.n_rows + a.n) {
        const uint64_t j = g - a.n_rows, id = a.b.id[j], k = lower_bound(a.cur.id, a.n_rows, id);
        const uint64_t d = j + k, bpos = (a.b.off[j] - a.b.off[0]) + a.cur.off[k];
        a.dst.id[d] = id;
        a.dst.rq[d] = a.b.rq[j];
        a.dst.inst[d] = a.b.inst[j];
        a.dst.prio[d] = a.b.prio[j];
        a.dst.cfg[d] = a.b.cfg[j];
        a.dst.some[d] = a.b.some[j] ? 1 : 0;
        a.dst.off[d] = bpos;
        l.len[tid] = a.b.off[j + 1] - a.b.off[j];
        l.src[tid] = a.b.blob + (a.b.off[j] - a.b.off[0]);
        l.dst[tid] = a.dst.blob + bpos;
    }
}

// ---- host execution of a kernel (debug hook, sanitizer program): a loop end = a workgroup barrier; `order` as in hqwire::run_on_host ---------
inline bool run_kernel_on_host(int kernel, const TArgs &a, uint32_t blocks, int order) {
    int seq[BLOCK];
    for (int i = 0; i < BLOCK; i++) seq[i] = order == 1 ? BLOCK - 1 - i : order == 2 ? (i * 77 + 13) % BLOCK : i;
    MoveLds *ml = new (std::nothrow) MoveLds;
    ScanLds *sl = new (std::nothrow) ScanLds;
    const bool ok = ml && sl;
    const uint64_t n_threads = (uint64_t)blocks * BLOCK;
#define HQT_ALL(stmt) for (int q = 0; q < BLOCK; q++) { const int tid = seq[q]; (void)tid; stmt; }
    if (ok) {
        if (kernel == K_SCAN) {
            HQT_ALL(scan_p1(a, *sl, tid)) HQT_ALL(scan_p2a(a, *sl, tid)) HQT_ALL(scan_p2b(a, *sl, tid)) HQT_ALL(scan_p2c(a, *sl, tid)) HQT_ALL(scan_p3(a, *sl, tid))
        } else
            for (uint32_t k = 0; k < blocks; k++) {
                const uint32_t blk = order == 1 ? blocks - 1 - k : k;  // workgroups run in no particular order either
                const uint64_t g0 = (uint64_t)blk * BLOCK;
                switch (kernel) {
                case K_APPEND: HQT_ALL(append_p(a, g0 + tid); append_blob(a, g0 + tid, n_threads)) break;
                case K_CHECK: HQT_ALL(check_p(a, g0 + tid)) break;
                case K_REMOVE: HQT_ALL(remove_p(a, g0 + tid)) break;
                case K_SETINST: HQT_ALL(setinst_p(a, g0 + tid)) break;
                case K_COUNT: HQT_ALL(tile_p1(a, *ml, blk, tid)) HQT_ALL(tile_p2a(a, *ml, blk, tid)) HQT_ALL(count_p3(a, *ml, blk, tid)) break;
                case K_MOVE:
                    HQT_ALL(tile_p1(a, *ml, blk, tid)) HQT_ALL(tile_p2a(a, *ml, blk, tid)) HQT_ALL(move_p2b(a, *ml, blk, tid)) HQT_ALL(move_p3(a, *ml, blk, tid))
                    HQT_ALL(move_p4(a, *ml, blk, tid)) break;
                case K_MERGE: HQT_ALL(merge_p1(a, *ml, blk, tid)) HQT_ALL(blob_p(*ml, tid)) break;
                default: break;
                }
            }
    }
#undef HQT_ALL
    delete ml;
    delete sl;
    return ok;
}

// =========================================================================================================================================
// Host side
// =========================================================================================================================================
struct Backend {
    virtual ~Backend() {}
    virtual void *alloc(size_t bytes) = 0;          // device memory
    virtual void release(void *p) = 0;
    virtual void *alloc_staging(size_t bytes) = 0;  // host memory the host fills and upload() reads (pinned on the device backend)
    virtual void release_staging(void *p) = 0;
    virtual bool upload(void *dev, const void *staging, size_t bytes) = 0;  // enqueued
    virtual bool download(void *host, const void *dev, size_t bytes) = 0;   // returns when the bytes are there (the stream has drained)
    virtual bool fill(void *dev, int byte, size_t bytes) = 0;               // enqueued
    virtual bool launch(int kernel, const TArgs &a, uint32_t blocks) = 0;   // enqueued
    virtual bool sync() = 0;
    virtual void time_begin() {}
    virtual double time_end_us() { return 0; }  // after a sync
};

struct HostBackend : Backend {  // exact-size heap blocks: under AddressSanitizer an out-of-bounds access of a phase aborts
    int order;
    explicit HostBackend(int order_) : order(order_) {}
    void *alloc(size_t bytes) override { return malloc(bytes ? bytes : 1); }
    void release(void *p) override { free(p); }
    void *alloc_staging(size_t bytes) override { return malloc(bytes ? bytes : 1); }
    void release_staging(void *p) override { free(p); }
    bool upload(void *dev, const void *staging, size_t bytes) override { if (bytes) memcpy(dev, staging, bytes); return true; }
    bool download(void *host, const void *dev, size_t bytes) override { if (bytes) memcpy(host, dev, bytes); return true; }
    bool fill(void *dev, int byte, size_t bytes) override { if (bytes) memset(dev, byte, bytes); return true; }
    bool launch(int kernel, const TArgs &a, uint32_t blocks) override { return run_kernel_on_host(kernel, a, blocks, order); }
    bool sync() override { return true; }
};

constexpr int E_INVALID = -1, E_DEVICE = -3;  // HQTICK_E_INVALID / HQTICK_E_DEVICE (include/hqtick.h)

class Table {
public:
    Table(Backend *be, const hqwire_table_config *cfg) : be_(be) {
        if (cfg) c_ = *cfg;
        if (!c_.initial_rows) c_.initial_rows = 1 << 16;
        if (!c_.initial_blob_bytes) c_.initial_blob_bytes = 1 << 20;
        if (!c_.initial_configs) c_.initial_configs = 64;
        if (!c_.initial_body_bytes) c_.initial_body_bytes = 1 << 16;
    }
    ~Table() {
        be_->sync();
        free_set(cur_, cap_rows_, cap_blob_);
        free_set(spare_, spare_rows_, spare_blob_);
        free_cfg();
        free_tiles();
        drop(res_, 8 * R_N);
        drop(dstage_, dstage_cap_);
        if (stage_) be_->release_staging(stage_);
        delete be_;
    }
    bool init() {
        if (c_.initial_rows >= MAX_ROWS) { fail(E_INVALID, "initial_rows too large"); return false; }
        res_ = (uint64_t *)grab(8 * R_N);
        if (!res_ || !alloc_set(cur_, c_.initial_rows, c_.initial_blob_bytes) || !alloc_cfg(c_.initial_configs, c_.initial_body_bytes)) return false;
        cap_rows_ = c_.initial_rows; cap_blob_ = c_.initial_blob_bytes;
        return be_->fill(cfg_.body_off, 0, 8) && be_->sync();
    }
    const char *last_error() const { return err_.c_str(); }
    uint64_t last_unknown() const { return last_unknown_; }

    int64_t add_configs(uint32_t n, const uint8_t *some, const uint64_t *secs, const uint32_t *nanos, const uint64_t *body_off, const uint8_t *body) {
        if (n == 0) return (int64_t)h_some_.size();
        if (!some || !secs || !nanos || !body_off) return fail(E_INVALID, "add_configs: NULL array");
        for (uint32_t i = 0; i < n; i++) if (body_off[i + 1] < body_off[i]) return fail(E_INVALID, "add_configs: body_off is not monotone");
        const uint64_t nb = body_off[n] - body_off[0];
        if (nb && !body) return fail(E_INVALID, "add_configs: NULL body_blob");
        if (h_some_.size() + n > 0xFFFFFFFFull) return fail(E_INVALID, "add_configs: too many configurations");
        const uint64_t first = h_some_.size(), base = h_body_.size();
        const uint64_t n_cfg = first + n, n_body = base + nb;
        be_->time_begin();
        bool grew = false;
        if (n_cfg > cap_cfg_ || n_body > cap_body_) {
            uint64_t cc = cap_cfg_, cb = cap_body_;
            while (cc < n_cfg) cc *= 2;
            while (cb < n_body) cb *= 2;
            if (!be_->sync()) return fail(E_DEVICE, "add_configs: device error");
            free_cfg();
            if (!alloc_cfg(cc, cb)) return fail(E_DEVICE, "add_configs: out of device memory");
            grew = true;
        }
        h_some_.insert(h_some_.end(), some, some + n);
        for (uint32_t i = 0; i < n; i++) { h_secs_.push_back(some[i] ? secs[i] : 0); h_nanos_.push_back(some[i] ? nanos[i] : 0); h_some_[first + i] = some[i] ? 1 : 0; }
        for (uint32_t i = 0; i < n; i++) h_boff_.push_back(base + (body_off[i + 1] - body_off[0]));
        if (nb) h_body_.insert(h_body_.end(), body + body_off[0], body + body_off[n]);
        // a few dozen configurations per server: the arrays go up whole
        const uint64_t o_secs = 0, o_boff = 8 * n_cfg, o_nanos = o_boff + 8 * (n_cfg + 1), o_some = o_nanos + 4 * n_cfg, o_body = o_some + n_cfg;
        if (!ensure_stage(o_body + n_body, false)) return fail(E_DEVICE, "add_configs: out of staging memory");
        memcpy(stage_ + o_secs, h_secs_.data(), 8 * n_cfg);
        memcpy(stage_ + o_boff, h_boff_.data(), 8 * (n_cfg + 1));
        memcpy(stage_ + o_nanos, h_nanos_.data(), 4 * n_cfg);
        memcpy(stage_ + o_some, h_some_.data(), n_cfg);
        if (n_body) memcpy(stage_ + o_body, h_body_.data(), n_body);
        const bool ok = be_->upload(cfg_.secs, stage_ + o_secs, 8 * n_cfg) && be_->upload(cfg_.body_off, stage_ + o_boff, 8 * (n_cfg + 1)) &&
                        be_->upload(cfg_.nanos, stage_ + o_nanos, 4 * n_cfg) && be_->upload(cfg_.some, stage_ + o_some, n_cfg) &&
                        be_->upload(cfg_.body, stage_ + o_body, n_body) && be_->sync();
        if (!ok) return fail(E_DEVICE, "add_configs: device error");
        kernel_us_ = be_->time_end_us();
        if (grew) growths_++;
        return (int64_t)first;
    }

    int64_t add_tasks(uint64_t n, const uint64_t *id, const uint32_t *rq, const uint32_t *inst, const uint64_t *prio, const uint32_t *cfg, const uint8_t *some,
                      const uint64_t *off, const uint8_t *blob) {
        if (n == 0) return 0;
        if (!id || !rq || !prio || !cfg) return fail(E_INVALID, "add_tasks: NULL array");
        if (some && !off) return fail(E_INVALID, "add_tasks: entry_some without entry_off");
        if (n_rows_ + n >= MAX_ROWS) return fail(E_INVALID, "add_tasks: the row total would reach 0xFFFFFFFF");
        uint64_t nb = 0;
        if (off) {
            if (off[n] < off[0]) return fail(E_INVALID, "add_tasks: entry_off is not monotone");
            nb = off[n] - off[0];
            if (nb && !blob) return fail(E_INVALID, "add_tasks: NULL entry_blob");
        }
        be_->time_begin();
        // the batch, laid out once in the staging buffer (array copies only) and sent to the device as one block
        const Stage s = stage_of(n, nb);
        if (!ensure_stage(s.total, true)) return fail(E_DEVICE, "add_tasks: out of staging memory");
        memcpy(stage_ + s.id, id, 8 * n);
        memcpy(stage_ + s.prio, prio, 8 * n);
        if (off) memcpy(stage_ + s.off, off, 8 * (n + 1)); else memset(stage_ + s.off, 0, 8 * (n + 1));
        memcpy(stage_ + s.rq, rq, 4 * n);
        if (inst) memcpy(stage_ + s.inst, inst, 4 * n); else memset(stage_ + s.inst, 0, 4 * n);
        memcpy(stage_ + s.cfg, cfg, 4 * n);
        if (some) memcpy(stage_ + s.some, some, n); else memset(stage_ + s.some, 0, n);
        memset(stage_ + s.some + n, 0, s.blob - (s.some + n));
        if (nb) memcpy(stage_ + s.blob, blob + off[0], nb);
        if (!be_->upload(dstage_, stage_, s.total)) return fail(E_DEVICE, "add_tasks: upload failed");
        TArgs a = args();
        bind_batch(a, s, n, nb);
        const bool append = !has_last_ || id[0] > last_id_;
        uint64_t r[R_N];
        if (append) {
            if (n_live_ + n > cap_rows_ || live_bytes_ + nb > cap_blob_ || n_rows_ + n > cap_rows_ || blob_bytes_ + nb > cap_blob_) {
                // out of room: dropping the dead rows may already do; otherwise the buffers double, the copy being a compaction into the new set
                uint64_t nr = cap_rows_, nbl = cap_blob_;
                while (nr < n_live_ + n) nr *= 2;
                while (nbl < live_bytes_ + nb) nbl *= 2;
                if (nr >= MAX_ROWS) nr = MAX_ROWS - 1;
                const bool grow = nr != cap_rows_ || nbl != cap_blob_;
                const int rc = rebuild(nr, nbl);
                if (rc) return rc;
                if (grow) growths_++;
                a = args();
                bind_batch(a, s, n, nb);
            }
            const uint64_t work = n > nb / 16 ? n : nb / 16;
            uint64_t wb = (work + BLOCK - 1) / BLOCK;
            if (wb > 4096) wb = 4096;
            const uint64_t rb = (n + BLOCK - 1) / BLOCK;
            const uint32_t blocks = (uint32_t)(wb > rb ? wb : rb);
            if (!run(K_APPEND, a, blocks, r)) return fail(E_DEVICE, "add_tasks: device error");
            if (r[R_FLAG]) return fail(E_INVALID, "add_tasks: batch refused (ids not ascending or resident, reserved id, configuration index, entry_off or entry_some)");
            n_rows_ += n; n_live_ += n; blob_bytes_ += nb; live_bytes_ += nb;
            last_id_ = id[n - 1]; has_last_ = true;
            appends_++;
            return (int64_t)n;
        }
        // merge
        if (!run(K_CHECK, a, (uint32_t)((n + BLOCK - 1) / BLOCK), r)) return fail(E_DEVICE, "add_tasks: device error");
        if (r[R_FLAG]) return fail(E_INVALID, "add_tasks: batch refused (ids not ascending or live in the table, reserved id, configuration index, entry_off or entry_some)");
        uint64_t nr = cap_rows_, nbl = cap_blob_;
        while (nr < n_live_ + n) nr *= 2;
        while (nbl < live_bytes_ + nb) nbl *= 2;
        if (nr >= MAX_ROWS) nr = MAX_ROWS - 1;
        const bool grow = nr != cap_rows_ || nbl != cap_blob_;
        if (n_live_ != n_rows_) {  // dead rows go first: the merge wants two dense tables
            const int rc = rebuild(cap_rows_, cap_blob_);
            if (rc) return rc;
        }
        if (!ensure_spare(nr, nbl)) return fail(E_DEVICE, "add_tasks: out of device memory");
        a = args();
        bind_batch(a, s, n, nb);
        a.dst = spare_;
        if (!be_->fill(spare_.live, 0xFF, live_bytes_of(spare_rows_))) return fail(E_DEVICE, "add_tasks: device error");
        if (!run(K_MERGE, a, (uint32_t)((n_rows_ + n + BLOCK - 1) / BLOCK), r)) return fail(E_DEVICE, "add_tasks: device error");
        if (r[R_FLAG]) return fail(E_INVALID, "add_tasks: batch refused (an id is live in the table)");  // (the check above saw it first)
        swap_sets();
        n_rows_ += n; n_live_ += n; blob_bytes_ += nb; live_bytes_ += nb;
        last_id_ = r[R_LAST]; has_last_ = true;
        merges_++;
        if (grow) { growths_++; free_set(spare_, spare_rows_, spare_blob_); }  // (the stream has drained: run() ends in a download)
        return (int64_t)n;
    }

    int64_t remove_tasks(uint64_t n, const uint64_t *id) {
        last_unknown_ = 0;
        if (n == 0) return 0;
        if (!id) return fail(E_INVALID, "remove_tasks: NULL array");
        be_->time_begin();
        uint64_t r[R_N];
        const int rc = id_kernel(K_REMOVE, n, id, nullptr, r);
        if (rc) return rc;
        n_live_ -= r[R_HIT]; live_bytes_ -= r[R_BYTES];
        last_unknown_ = r[R_UNKNOWN];
        const uint64_t dead = n_rows_ - n_live_, dead_bytes = blob_bytes_ - live_bytes_;
        if (dead > n_live_ || dead_bytes > live_bytes_) {
            const int rc2 = rebuild(cap_rows_, cap_blob_);
            if (rc2) return rc2;
        }
        return (int64_t)r[R_HIT];
    }
    int64_t set_instance(uint64_t n, const uint64_t *id, const uint32_t *values) {
        last_unknown_ = 0;
        if (n == 0) return 0;
        if (!id) return fail(E_INVALID, "set_instance: NULL array");
        be_->time_begin();
        uint64_t r[R_N];
        const int rc = id_kernel(K_SETINST, n, id, values, r);
        if (rc) return rc;
        last_unknown_ = r[R_UNKNOWN];
        return (int64_t)r[R_HIT];
    }
    int compact() {
        if (n_live_ == n_rows_) return 0;
        be_->time_begin();
        return rebuild(cap_rows_, cap_blob_);
    }
    void view(hqwire_tables *o) const {
        o->n_tasks = n_rows_;
        o->task_id = cur_.id; o->task_rq = cur_.rq; o->task_instance = cur_.inst; o->task_priority = cur_.prio; o->task_config = cur_.cfg;
        o->entry_some = cur_.some; o->entry_off = cur_.off; o->entry_blob = cur_.blob;
        o->n_configs = (uint32_t)h_some_.size();
        o->config_time_some = cfg_.some; o->config_time_secs = cfg_.secs; o->config_time_nanos = cfg_.nanos; o->body_off = cfg_.body_off; o->body_blob = cfg_.body;
    }
    int copy_out(hqwire_tables *h) {
        const uint64_t n = n_rows_, c = h_some_.size();
        h->n_tasks = n; h->n_configs = (uint32_t)c;
        bool ok = true;
        auto get = [&](const void *dst, const void *src, uint64_t bytes) { if (dst && bytes) ok = ok && be_->download(const_cast<void *>(dst), src, bytes); };
        get(h->task_id, cur_.id, 8 * n); get(h->task_rq, cur_.rq, 4 * n); get(h->task_instance, cur_.inst, 4 * n); get(h->task_priority, cur_.prio, 8 * n);
        get(h->task_config, cur_.cfg, 4 * n); get(h->entry_some, cur_.some, n); get(h->entry_off, cur_.off, 8 * (n + 1)); get(h->entry_blob, cur_.blob, blob_bytes_);
        get(h->config_time_some, cfg_.some, c); get(h->config_time_secs, cfg_.secs, 8 * c); get(h->config_time_nanos, cfg_.nanos, 4 * c);
        get(h->body_off, cfg_.body_off, 8 * (c + 1)); get(h->body_blob, cfg_.body, h_body_.size());
        return ok ? 0 : fail(E_DEVICE, "copy_out: device error");
    }
    void stats(hqwire_table_stats *o) const {
        o->live_rows = n_live_; o->physical_rows = n_rows_; o->blob_bytes = blob_bytes_; o->dead_blob_bytes = blob_bytes_ - live_bytes_;
        o->n_configs = h_some_.size(); o->body_bytes = h_body_.size();
        o->appends = appends_; o->merges = merges_; o->compactions = compactions_; o->growths = growths_;
        o->hbm_bytes = hbm_; o->last_kernel_us = kernel_us_;
    }

private:
    struct Cfg { uint8_t *some = nullptr; uint64_t *secs = nullptr; uint32_t *nanos = nullptr; uint64_t *body_off = nullptr; uint8_t *body = nullptr; };

    int fail(int code, const char *what) { err_ = what; return code; }
    void *grab(uint64_t bytes) {
        void *p = be_->alloc(bytes);
        if (p) hbm_ += bytes;
        return p;
    }
    template <class T> void drop(T *&p, uint64_t bytes) {
        if (p) { be_->release((void *)p); hbm_ -= bytes; }
        p = nullptr;
    }
    static uint64_t live_bytes_of(uint64_t rows) { return 4 * ((rows + 31) / 32); }
    bool alloc_set(Cols &c, uint64_t rows, uint64_t blob) {
        c.id = (uint64_t *)grab(8 * rows); c.rq = (uint32_t *)grab(4 * rows); c.inst = (uint32_t *)grab(4 * rows); c.prio = (uint64_t *)grab(8 * rows);
        c.cfg = (uint32_t *)grab(4 * rows); c.some = (uint8_t *)grab(rows); c.off = (uint64_t *)grab(8 * (rows + 1)); c.blob = (uint8_t *)grab(blob);
        c.live = (uint32_t *)grab(live_bytes_of(rows));
        if (!c.id || !c.rq || !c.inst || !c.prio || !c.cfg || !c.some || !c.off || !c.blob || !c.live) { fail(E_DEVICE, "out of device memory"); return false; }
        return be_->fill(c.off, 0, 8) && be_->fill(c.live, 0xFF, live_bytes_of(rows));
    }
    void free_set(Cols &c, uint64_t &rows, uint64_t &blob) {
        drop(c.id, 8 * rows); drop(c.rq, 4 * rows); drop(c.inst, 4 * rows); drop(c.prio, 8 * rows); drop(c.cfg, 4 * rows); drop(c.some, rows);
        drop(c.off, 8 * (rows + 1)); drop(c.blob, blob); drop(c.live, live_bytes_of(rows));
        rows = blob = 0;
    }
    bool alloc_cfg(uint64_t n, uint64_t body) {
        cfg_.some = (uint8_t *)grab(n); cfg_.secs = (uint64_t *)grab(8 * n); cfg_.nanos = (uint32_t *)grab(4 * n); cfg_.body_off = (uint64_t *)grab(8 * (n + 1));
        cfg_.body = (uint8_t *)grab(body);
        cap_cfg_ = n; cap_body_ = body;
        if (!cfg_.some || !cfg_.secs || !cfg_.nanos || !cfg_.body_off || !cfg_.body) { fail(E_DEVICE, "out of device memory"); return false; }
        return true;
    }
    void free_cfg() {
        drop(cfg_.some, cap_cfg_); drop(cfg_.secs, 8 * cap_cfg_); drop(cfg_.nanos, 4 * cap_cfg_); drop(cfg_.body_off, 8 * (cap_cfg_ + 1)); drop(cfg_.body, cap_body_);
    }
    void free_tiles() {
        drop(tile_rows_, 4 * tiles_cap_); drop(tile_row_base_, 4 * tiles_cap_); drop(tile_bytes_, 8 * tiles_cap_); drop(tile_byte_base_, 8 * tiles_cap_);
        tiles_cap_ = 0;
    }
    bool ensure_tiles(uint64_t n_tiles) {
        if (n_tiles <= tiles_cap_) return true;
        if (!be_->sync()) return false;
        free_tiles();
        tile_rows_ = (uint32_t *)grab(4 * n_tiles); tile_row_base_ = (uint32_t *)grab(4 * n_tiles);
        tile_bytes_ = (uint64_t *)grab(8 * n_tiles); tile_byte_base_ = (uint64_t *)grab(8 * n_tiles);
        tiles_cap_ = n_tiles;
        return tile_rows_ && tile_row_base_ && tile_bytes_ && tile_byte_base_;
    }
    // staging of exactly the size asked for (it grows only); `device`: the device-side copy as well
    bool ensure_stage(uint64_t bytes, bool device) {
        if (bytes > stage_cap_) {
            if (!be_->sync()) return false;
            if (stage_) be_->release_staging(stage_);
            stage_ = (uint8_t *)be_->alloc_staging(bytes);
            stage_cap_ = stage_ ? bytes : 0;
            if (!stage_) return false;
        }
        if (device && bytes > dstage_cap_) {
            if (!be_->sync()) return false;
            drop(dstage_, dstage_cap_);
            dstage_ = (uint8_t *)grab(bytes);
            dstage_cap_ = dstage_ ? bytes : 0;
            if (!dstage_) return false;
        }
        return true;
    }
    bool ensure_spare(uint64_t rows, uint64_t blob) {
        if (spare_.id && spare_rows_ == rows && spare_blob_ == blob) return true;
        if (!be_->sync()) return false;
        free_set(spare_, spare_rows_, spare_blob_);
        if (!alloc_set(spare_, rows, blob)) return false;
        spare_rows_ = rows; spare_blob_ = blob;
        return true;
    }
    void swap_sets() {
        Cols c = cur_; cur_ = spare_; spare_ = c;
        uint64_t t = cap_rows_; cap_rows_ = spare_rows_; spare_rows_ = t;
        t = cap_blob_; cap_blob_ = spare_blob_; spare_blob_ = t;
    }
    TArgs args() const {
        TArgs a{};
        a.cur = cur_; a.dst = spare_;
        a.n_rows = n_rows_; a.n_blob = blob_bytes_;
        a.last_id = last_id_; a.has_last = has_last_ ? 1 : 0;
        a.n_configs = (uint32_t)h_some_.size();
        a.res = res_;
        a.tile_rows = tile_rows_; a.tile_row_base = tile_row_base_; a.tile_bytes = tile_bytes_; a.tile_byte_base = tile_byte_base_;
        return a;
    }
    void bind_batch(TArgs &a, const Stage &s, uint64_t n, uint64_t nb) const {
        const uint8_t *p = dstage_;
        a.n = n; a.nb = nb;
        a.b.id = (const uint64_t *)(p + s.id); a.b.prio = (const uint64_t *)(p + s.prio); a.b.off = (const uint64_t *)(p + s.off);
        a.b.rq = (const uint32_t *)(p + s.rq); a.b.inst = (const uint32_t *)(p + s.inst); a.b.cfg = (const uint32_t *)(p + s.cfg);
        a.b.some = p + s.some; a.b.blob = p + s.blob; a.b.val = nullptr;
    }
    // one kernel and its round trip: the result block cleared, the kernel, the block read back
    bool run(int kernel, const TArgs &a, uint32_t blocks, uint64_t r[R_N]) {
        const bool ok = be_->fill(res_, 0, 8 * R_N) && be_->launch(kernel, a, blocks) && be_->download(r, res_, 8 * R_N);
        if (ok) kernel_us_ = be_->time_end_us();
        return ok;
    }
    int id_kernel(int kernel, uint64_t n, const uint64_t *id, const uint32_t *values, uint64_t r[R_N]) {
        const uint64_t bytes = 8 * n + (values ? 4 * n : 0);
        if (!ensure_stage(bytes, true)) return fail(E_DEVICE, "out of staging memory");
        memcpy(stage_, id, 8 * n);
        if (values) memcpy(stage_ + 8 * n, values, 4 * n);
        if (!be_->upload(dstage_, stage_, bytes)) return fail(E_DEVICE, "upload failed");
        TArgs a = args();
        a.n = n;
        a.b.id = (const uint64_t *)dstage_;
        a.b.val = values ? (const uint32_t *)(dstage_ + 8 * n) : nullptr;
        a.with_values = values ? 1 : 0;
        if (!run(kernel, a, (uint32_t)((n + BLOCK - 1) / BLOCK), r)) return fail(E_DEVICE, "device error");
        return 0;
    }
    // The live rows of cur into a set of (rows, blob) capacity -- the spare one, or a new one when the capacities change (growth) --, which becomes cur.
    int rebuild(uint64_t rows, uint64_t blob) {
        const bool had_dead = n_live_ != n_rows_;
        const bool resize = rows != cap_rows_ || blob != cap_blob_;
        if (n_live_ == 0 && !resize) {  // nothing survives: the columns are simply empty again
            if (!be_->fill(cur_.live, 0xFF, live_bytes_of(cap_rows_)) || !be_->sync()) return fail(E_DEVICE, "compact: device error");
            n_rows_ = 0; blob_bytes_ = 0; has_last_ = false; last_id_ = 0;
            if (had_dead) compactions_++;
            return 0;
        }
        if (!ensure_spare(rows, blob)) return fail(E_DEVICE, "out of device memory");
        const uint64_t n_tiles = (n_rows_ + TILE - 1) / TILE;
        if (!ensure_tiles(n_tiles ? n_tiles : 1)) return fail(E_DEVICE, "out of device memory");
        TArgs a = args();
        a.n_tiles = (uint32_t)n_tiles;
        uint64_t r[R_N] = {0};
        bool ok = be_->fill(spare_.live, 0xFF, live_bytes_of(spare_rows_)) && be_->fill(res_, 0, 8 * R_N);
        if (n_tiles) ok = ok && be_->launch(K_COUNT, a, (uint32_t)n_tiles);
        ok = ok && be_->launch(K_SCAN, a, 1);
        if (n_tiles) ok = ok && be_->launch(K_MOVE, a, (uint32_t)n_tiles);
        ok = ok && be_->download(r, res_, 8 * R_N);
        if (!ok) return fail(E_DEVICE, "compact: device error");
        kernel_us_ = be_->time_end_us();
        if (r[R_ROWS] != n_live_ || r[R_BLOB] != live_bytes_) return fail(E_DEVICE, "compact: the device's live counts differ from the host's");
        swap_sets();
        n_rows_ = n_live_; blob_bytes_ = live_bytes_;
        has_last_ = n_rows_ != 0; last_id_ = has_last_ ? r[R_LAST] : 0;
        if (had_dead) compactions_++;
        if (resize) free_set(spare_, spare_rows_, spare_blob_);  // the old, smaller set (the stream has drained)
        return 0;
    }

    Backend *be_;
    hqwire_table_config c_{};
    Cols cur_{}, spare_{};
    uint64_t cap_rows_ = 0, cap_blob_ = 0, spare_rows_ = 0, spare_blob_ = 0;
    uint64_t n_rows_ = 0, n_live_ = 0, blob_bytes_ = 0, live_bytes_ = 0, last_id_ = 0;
    bool has_last_ = false;
    Cfg cfg_;
    uint64_t cap_cfg_ = 0, cap_body_ = 0;
    std::vector<uint8_t> h_some_, h_body_;  // the configurations once more on the host (append-only, a few dozen)
    std::vector<uint64_t> h_secs_, h_boff_{0};
    std::vector<uint32_t> h_nanos_;
    uint64_t *res_ = nullptr;
    uint32_t *tile_rows_ = nullptr, *tile_row_base_ = nullptr;
    uint64_t *tile_bytes_ = nullptr, *tile_byte_base_ = nullptr, tiles_cap_ = 0;
    uint8_t *stage_ = nullptr, *dstage_ = nullptr;
    uint64_t stage_cap_ = 0, dstage_cap_ = 0;
    uint64_t appends_ = 0, merges_ = 0, compactions_ = 0, growths_ = 0, hbm_ = 0, last_unknown_ = 0;
    double kernel_us_ = 0;
    std::string err_;
};

}  // namespace hqwtab
