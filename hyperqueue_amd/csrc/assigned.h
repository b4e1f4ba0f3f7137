// Assignment ledger: every single-node task in state Assigned / Running — and every Retracting task counted on its
// redirect target (server/worker.rs:249-252) — with the worker it runs on, kept in HBM between ticks, together with the per-worker
// (rq, variant) counts that GapCache and Worker::is_free read and the free rows of the resident worker set.
//
// Layout:
//   id -> entry: open-addressing hash table (linear probing, tombstones, rebuilt at half load), SoA columns indexed by bucket:
//     key u64 (HT_EMPTY / HT_TOMB) | worker id u32 | rq u32 | variant u8 | priority u64 | claim u32 (batch position of a release, else NONE)
//   counts u32 [W x stride]: running tasks per (worker row, variant slot); slot = rq_variant_off[rq] + variant
//   free / total rows: the resident worker set's own rows in HBM (hqtick_cluster_*), updated in place
// Everything here is integer work bound by HBM latency; no MFMA.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hqasg {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t HT_EMPTY = ~0ull, HT_TOMB = ~0ull - 1;  // task ids must be below HT_TOMB
constexpr uint32_t RQ_LOOKUP = 0xFFFFFFFFu;              // insert item whose rq / priority come from the ready-set columns

struct Table {
    uint64_t *key; uint32_t *worker; uint32_t *rq; uint8_t *variant; uint64_t *prio; uint32_t *claim;
    uint32_t mask;  // capacity - 1 (a power of two)
};
// the request tables (ResourceRqMap) as the ledger needs them: rq -> variant slots -> entries
struct Req {
    const uint32_t *rq_off; const uint32_t *ventry_off; const uint32_t *ent_res; const uint8_t *ent_kind; const uint64_t *ent_amount;
    uint32_t Q;
};
// the resident worker set: ids in row order, total / free rows, the count table
struct Rows {
    const uint32_t *wid; uint32_t W, R;
    const uint64_t *total; uint64_t *free_;
    uint32_t *counts; uint32_t stride;
};
// an insert batch from explicit columns (wid: worker ids)
struct Items {
    uint32_t n;
    const uint64_t *id; const uint32_t *wid; const uint32_t *rq; const uint8_t *variant; const uint64_t *prio;
    // rq / priority of an item with rq == RQ_LOOKUP: the ready-set columns, ids ascending
    const uint64_t *col_id; const uint64_t *col_prio; const uint32_t *col_rq; uint64_t col_n;
};
// a tick's placement as the mapping kernel staged it in HBM (kernels.h: hqk::Stage), one entry per record; meta = variant | kind << 8, entries whose kind
// is not HQ_REC_ASSIGN are skipped.  The priority is levels[level] (the dense scan's level table, n_levels entries); levels == nullptr (the ordered view,
// whose run table lives in host memory): the priority alone is looked up by id in the ready-set columns col_id / col_prio.
struct Staged {
    uint32_t n;
    const uint64_t *task; const uint32_t *rq; const uint32_t *row; const uint32_t *level; const uint16_t *meta;
    const uint64_t *levels; uint32_t n_levels;
    const uint64_t *col_id; const uint64_t *col_prio; uint64_t col_n;
};
// counters of one operation, in device memory, one atomic per wavefront (insert: C_OUT = entries that were not there before; evict: entries gathered)
enum Ctr : uint32_t { C_DONE = 0, C_UNKNOWN = 1, C_DUP = 2, C_FULL = 3, C_BAD = 4, C_OUT = 5, C_N = 8 };

hipError_t clear(Table t, hipStream_t s);
// insert (upsert != 0: an id already present moves to the new worker / variant, its old count is given back; else it is counted as a duplicate).
// apply_free != 0: Worker::insert_sn_task's free.remove on the worker's row (AMOUNT subtracts with saturation, ALL sets 0; these commute).
hipError_t insert(Table t, Req q, Rows r, Items it, int upsert, int apply_free, uint32_t *ctr, hipStream_t s);
// the staged placement of a tick as upserts, free rows untouched (they become the tick's new_free)
hipError_t insert_staged(Table t, Req q, Rows r, Staged st, uint32_t *ctr, hipStream_t s);
// release in batch order with the last-ALL rule; scratch: pos [n] u32, last_all [W * R] u32, delta [W * R] u64 (zero on entry and on return)
hipError_t release(Table t, Req q, Rows r, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, uint32_t *ctr, hipStream_t s);
// every entry of the workers `lost` (sorted ids) leaves the table; (id, rq, priority) appended to out_* [cap_out] (order undefined), count in ctr[C_OUT]
hipError_t evict(Table t, uint32_t n_lost, const uint32_t *lost, uint64_t *out_id, uint32_t *out_rq, uint64_t *out_prio, uint32_t cap_out, uint32_t *ctr, hipStream_t s);
// live entries of `from` re-inserted into the (cleared) table `to`
hipError_t rehash(Table from, Table to, uint32_t *ctr, hipStream_t s);
// dst row w = src row src_row[w] (NONE or >= W_src: a zero row), columns [0, n_cols)
hipError_t repack_counts(const uint32_t *src, uint32_t src_stride, uint32_t W_src, const uint32_t *src_row, uint32_t W_dst, uint32_t *dst, uint32_t dst_stride,
                         uint32_t n_cols, hipStream_t s);
hipError_t lookup(Table t, uint32_t n, const uint64_t *id, uint32_t *out_wid, uint8_t *out_variant, hipStream_t s);

}  // namespace hqasg
