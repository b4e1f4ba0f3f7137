// Kernels of the assignment ledger (assigned.h).  gfx950 only.
#include "assigned.h"
#include "cancel.h"
#include "fail_core.h"
#include "lose_core.h"
#include "kernels.h"
#include "finish_core.h"
#include "reject_core.h"
#include "start_core.h"

#include "../../include/hqtick.h"

namespace hqasg {

namespace {

constexpr uint32_t TPB = 256;
enum RelMode : int { M_RELEASE = 0, M_CANCEL = 1, M_FINISH = 2, M_FAIL = 3, M_REJECT = 4 };  // what the release's four passes run as (release / hqtick_cancel_tasks / hqtick_finish_tasks / hqtick_fail_tasks / hqtick_reject_tasks)
// the three modes with a reporter per position share their claims; what differs is the rule and its constants
template <int MODE> __device__ __forceinline__ bool rep_accepted(uint32_t kind) { return MODE == M_REJECT ? hqreject::accepted(kind) : MODE == M_FAIL ? hqfail::accepted(kind) : hqfinish::accepted(kind); }
template <int MODE> __device__ __forceinline__ uint32_t rep_repeat(uint32_t kind) {
    return MODE == M_REJECT ? hqreject::after_claim(kind, true) : MODE == M_FAIL ? hqfail::after_claim(kind, true) : hqfinish::after_claim(kind, true);
}
template <int MODE> __device__ __forceinline__ uint32_t rep_retracting() { return MODE == M_REJECT ? HQ_REJECT_RETRACTING : MODE == M_FAIL ? HQ_FAIL_RETRACTING : HQ_FINISH_RETRACTING; }
inline unsigned nblk(uint64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

__device__ __forceinline__ uint32_t ht_hash(uint64_t k) {  // murmur3 finaliser (graph.hip's)
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}
__device__ __forceinline__ uint32_t ht_find(const Table &t, uint64_t id) {
    uint32_t h = ht_hash(id) & t.mask;
    for (uint32_t probe = 0; probe <= t.mask; probe++) {
        const uint64_t k = __atomic_load_n(&t.key[h], __ATOMIC_RELAXED);
        if (k == id) return h;
        if (k == HT_EMPTY) return NONE;
        h = (h + 1) & t.mask;
    }
    return NONE;
}
// bucket of `id`: *fresh = 1 if this call claimed an empty bucket for it, 0 if it was there; NONE = table full.  Tombstones are not reused
// (a probe sequence never changes under concurrent inserts); the host rebuilds the table before live + tombstones pass half the capacity.
__device__ __forceinline__ uint32_t ht_claim(const Table &t, uint64_t id, int *fresh) {
    uint32_t h = ht_hash(id) & t.mask;
    for (uint32_t probe = 0; probe <= t.mask; probe++) {
        const uint64_t k = __atomic_load_n(&t.key[h], __ATOMIC_RELAXED);
        if (k == id) { *fresh = 0; return h; }
        if (k == HT_EMPTY) {
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(&t.key[h]), (unsigned long long)HT_EMPTY, (unsigned long long)id);
            if (old == HT_EMPTY) { *fresh = 1; return h; }
            if (old == id) { *fresh = 0; return h; }
        }
        h = (h + 1) & t.mask;
    }
    return NONE;
}
// one atomic per wavefront for a per-lane flag (every lane of the wave must call)
__device__ __forceinline__ void wave_add(uint32_t *c, bool v) {
    const uint64_t m = __ballot(v);
    if (m && __lane_id() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(c, (uint32_t)__popcll(m));
}
// position of the calling lane among the lanes that want a slot; one atomic per wavefront (graph.hip's)
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, bool want) {
    const uint64_t m = __ballot(want);
    if (m == 0) return 0;
    const uint32_t lane = __lane_id(), leader = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ uint32_t row_of(const Rows &r, uint32_t wid) {  // ids ascend in row order
    uint32_t lo = 0, hi = r.W;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (r.wid[mid] < wid) lo = mid + 1; else hi = mid; }
    return (lo < r.W && r.wid[lo] == wid) ? lo : NONE;
}
__device__ __forceinline__ bool variant_ok(const Req &q, uint32_t rq, uint32_t v) { return rq < q.Q && v < q.rq_off[rq + 1] - q.rq_off[rq]; }
// free.remove of one entry (workerload.rs:156-166): AMOUNT subtracts with saturation, ALL sets 0 — order-free, so plain atomics do
__device__ __forceinline__ void free_remove(uint64_t *f, uint8_t kind, uint64_t amount) {
    if (kind == HQ_ENTRY_ALL) { atomicExch(reinterpret_cast<unsigned long long *>(f), 0ull); return; }
    unsigned long long cur = __atomic_load_n(reinterpret_cast<unsigned long long *>(f), __ATOMIC_RELAXED);
    for (;;) {
        const unsigned long long want = cur > amount ? cur - amount : 0ull;
        const unsigned long long got = atomicCAS(reinterpret_cast<unsigned long long *>(f), cur, want);
        if (got == cur) return;
        cur = got;
    }
}

__global__ void k_clear(Table t) {
    const uint32_t b = blockIdx.x * TPB + threadIdx.x;
    if (b > t.mask) return;
    t.key[b] = HT_EMPTY; t.claim[b] = NONE; t.run[b] = 0;
}

enum InsertStatus : int { S_SKIP = 0, S_FRESH, S_MOVED, S_DUP, S_BAD, S_FULL, S_PF_IN, S_PF_OUT };  // (S_PF_IN: a prefilled entry entered; S_PF_OUT: one became an assigned entry)
// the entry (id -> wid, rq, v, prio) enters its bucket and the count of (row, slot) is raised
// (run: the running byte a fresh entry takes; an entry that is moved to another worker or variant is not running there yet)
__device__ __forceinline__ int enter(const Table &t, const Req &q, const Rows &r, uint64_t id, uint32_t row, uint32_t wid, uint32_t rq, uint32_t v, uint64_t prio, int upsert,
                                     int apply_free, uint8_t run = 0) {
    if (row >= r.W || id >= HT_TOMB) return S_BAD;
    if (!variant_ok(q, rq, v) || q.rq_off[rq] + v >= r.stride) return S_BAD;
    int fresh = 0; bool from_pf = false;
    const uint32_t b = ht_claim(t, id, &fresh);
    if (b == NONE) return S_FULL;
    if (!fresh) {
        if (!upsert || t.variant[b] == MN_VARIANT) return S_DUP;  // (a multi-node task never moves: it has no count to give back)
        const uint32_t orow = row_of(r, t.worker[b]);  // a re-targeted redirect: the old target's count goes back (its free row is the tick's)
        from_pf = t.variant[b] == PF_VARIANT;          // out of a prefill set (remove_prefill_task, mapping.rs:85-88): the old worker's prefilled count instead
        if (from_pf) { if (orow != NONE && r.pf && t.rq[b] < r.pf_stride) atomicSub(&r.pf[(size_t)orow * r.pf_stride + t.rq[b]], 1u); }
        else if (orow != NONE) atomicSub(&r.counts[(size_t)orow * r.stride + q.rq_off[t.rq[b]] + t.variant[b]], 1u);
    }
    if (fresh) t.run[b] = run; else if (t.worker[b] != wid || t.variant[b] != (uint8_t)v) t.run[b] = 0;
    t.worker[b] = wid; t.rq[b] = rq; t.variant[b] = (uint8_t)v; t.prio[b] = prio; t.claim[b] = NONE;
    const uint32_t slot = q.rq_off[rq] + v;
    atomicAdd(&r.counts[(size_t)row * r.stride + slot], 1u);
    if (apply_free)
        for (uint32_t e = q.ventry_off[slot]; e < q.ventry_off[slot + 1]; e++) free_remove(&r.free_[(size_t)row * r.R + q.ent_res[e]], q.ent_kind[e], q.ent_amount[e]);
    return fresh ? S_FRESH : from_pf ? S_PF_OUT : S_MOVED;
}
// a prefilled task enters: no (row, slot) count, no free row — the prefilled count of (row, rq) alone.  The id must be new.
__device__ __forceinline__ int enter_pf(const Table &t, const Req &q, const Rows &r, uint64_t id, uint32_t row, uint32_t wid, uint32_t rq, uint64_t prio) {
    if (row >= r.W || id >= HT_TOMB || rq >= q.Q || rq >= r.pf_stride) return S_BAD;
    int fresh = 0;
    const uint32_t b = ht_claim(t, id, &fresh);
    if (b == NONE) return S_FULL;
    if (!fresh) return S_DUP;
    t.worker[b] = wid; t.rq[b] = rq; t.variant[b] = PF_VARIANT; t.prio[b] = prio; t.claim[b] = NONE; t.run[b] = 0;
    atomicAdd(&r.pf[(size_t)row * r.pf_stride + rq], 1u);
    return S_PF_IN;
}
// index of `id` in the ascending ready-set id column, ~0 if absent (a consumed task keeps its id and priority)
__device__ __forceinline__ uint64_t col_find(const uint64_t *col_id, uint64_t col_n, uint64_t id) {
    uint64_t lo = 0, hi = col_n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (col_id[mid] < id) lo = mid + 1; else hi = mid; }
    return (lo < col_n && col_id[lo] == id) ? lo : ~0ull;
}
__device__ __forceinline__ void count_status(uint32_t *ctr, int st) {
    wave_add(&ctr[C_DONE], st == S_FRESH || st == S_MOVED || st == S_PF_IN || st == S_PF_OUT); wave_add(&ctr[C_OUT], st == S_FRESH);
    wave_add(&ctr[C_PF], st == S_PF_IN || st == S_PF_OUT);
    wave_add(&ctr[C_DUP], st == S_DUP); wave_add(&ctr[C_BAD], st == S_BAD); wave_add(&ctr[C_FULL], st == S_FULL);
}
__device__ __forceinline__ int insert_one(const Table &t, const Req &q, const Rows &r, const Items &it, int upsert, int apply_free, uint32_t i) {
    const uint64_t id = it.id[i]; uint64_t prio = it.prio ? it.prio[i] : 0;
    const uint32_t wid = it.wid[i], v = it.variant[i]; uint32_t rq = it.rq ? it.rq[i] : RQ_LOOKUP;
    const uint32_t row = row_of(r, wid);
    if (row == NONE || id >= HT_TOMB) return S_BAD;
    if (r.pf && upsert) {  // a task out of a prefill set is in no queue: its prefilled entry knows request and priority
        const uint32_t b = ht_find(t, id);
        if (b != NONE && t.variant[b] == PF_VARIANT) { rq = t.rq[b]; prio = t.prio[b]; }
    }
    if (rq == RQ_LOOKUP) {  // rq and priority of a task of the ready set
        const uint64_t j = col_find(it.col_id, it.col_n, id);
        if (j == ~0ull) return S_BAD;
        rq = it.col_rq[j]; prio = it.col_prio[j];
    }
    return enter(t, q, r, id, row, wid, rq, v, prio, upsert, apply_free, it.run);
}
__global__ void k_insert(Table t, Req q, Rows r, Items it, int upsert, int apply_free, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    count_status(ctr, i < it.n ? insert_one(t, q, r, it, upsert, apply_free, i) : S_SKIP);
}
// the staged placement of a tick (K5b's extra output): every array is read once, coalesced; no search in the ready-set columns on the dense path
__global__ void k_insert_staged(Table t, Req q, Rows r, Staged st, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    int status = S_SKIP;
    if (i < st.n) {
        const uint32_t meta = st.meta[i];
        const bool assign = (meta >> 8) == HQ_REC_ASSIGN;
        if (assign || r.pf) {  // (r.pf == nullptr, uniform: prefills do not enter the ledger)
            const uint64_t id = st.task[i]; const uint32_t row = st.row[i], lvl = st.level[i], rq = st.rq[i];
            uint64_t prio = 0; bool ok = row < r.W;
            if (st.levels) { ok = ok && lvl < st.n_levels; if (ok) prio = st.levels[lvl]; }
            else { const uint64_t j = col_find(st.col_id, st.col_n, id); ok = ok && j != ~0ull; if (ok) prio = st.col_prio[j]; }
            if (!ok) status = S_BAD;
            else status = assign ? enter(t, q, r, id, row, r.wid[row], rq, meta & 0xFFu, prio, 1, 0) : enter_pf(t, q, r, id, row, r.wid[row], rq, prio);
        }
    }
    count_status(ctr, status);
}

// index of `id` in the ascending ids of the Retracting overrides, NONE if absent
__device__ __forceinline__ uint32_t retr_find(const CancelCols &cc, uint64_t id) {
    uint32_t lo = 0, hi = cc.n_retr;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cc.retr_id[mid] < id) lo = mid + 1; else hi = mid; }
    return (lo < cc.n_retr && cc.retr_id[lo] == id) ? lo : NONE;
}
// release, pass 1: the bucket of every id; the first position of an id in the batch claims it (later ones are duplicates)
// CANCEL (hqtick_cancel_tasks, the same four passes): a prefilled entry is claimed like the others, every position starts with no route, and the first position
// of an id of the Retracting overrides claims its override the same way
// FINISH (hqtick_finish_tasks): finish_core.h's rule decides from the entry, the override and the REPORTER of the position what the position is; only a position
// with an accepted kind is eligible, and it claims the entry and the override of its id alike -- both atomicMin run over the same eligible positions, so both
// name the same winner whatever order they arrive in.  A refused position keeps pos NONE: the later passes never see it.
// FAIL (hqtick_fail_tasks): the same with fail_core.h's rule.  A prefilled entry reported by its worker IS claimed (pass 3 takes it out as the cancel mode does); a
// _WAITING position (reporter HQ_NO_WORKER, neither entry nor override) is accepted but has nothing here to claim: the graph step settles its repeats.
// REJECT (hqtick_reject_tasks): reject_core.h's rule, which also reads the rejected variant, the running byte and the request tables (q, r and rj are read in this
// mode alone).  A position the overrides decide claims its override and never an entry: a redirect target's entry stays where it is.  The pair the position
// blocks follows from the same inputs and is written here; a position that later loses its claim keeps it, and the host drops it by the final kind.
template <int MODE>
__global__ void k_rel_claim(Table t, uint32_t n, const uint64_t *id, uint32_t *pos, CancelCols cc, uint32_t *ctr, Req q, Rows r, RejectCols rj) {
    constexpr bool CANCEL = MODE == M_CANCEL, FINISH = MODE == M_FINISH, FAIL = MODE == M_FAIL, REJECT = MODE == M_REJECT;
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    uint32_t b = NONE;
    if (i < n) {
        b = id[i] < HT_TOMB ? ht_find(t, id[i]) : NONE;
        if (MODE == M_RELEASE && b != NONE && t.variant[b] == PF_VARIANT) b = NONE;  // a prefilled task is not running: unknown to a release
        if (FINISH || FAIL) {
            const uint32_t k = retr_find(cc, id[i]), rep = cc.reporter[i];
            const uint32_t cls = b == NONE ? hqfinish::E_SN : t.variant[b] == PF_VARIANT ? hqfinish::E_PF : t.variant[b] == MN_VARIANT ? hqfinish::E_MN : hqfinish::E_SN;
            const bool e_match = b != NONE && t.worker[b] == rep, o_match = k != NONE && cc.retr_wid[k] == rep;
            const uint32_t kind = FAIL ? hqfail::kind_before_claim(b != NONE, cls, e_match, k != NONE, o_match, rep == HQ_NO_WORKER)
                                       : hqfinish::kind_before_claim(b != NONE, cls, e_match, k != NONE, o_match);
            cc.kind[i] = (uint8_t)kind;
            if (rep_accepted<MODE>(kind)) { if (k != NONE) atomicMin(&cc.retr_hit[k], i); }
            else b = NONE;
            // a prefilled entry is never claimed under a Retracting override, and by a finish not at all
            if (b != NONE && t.variant[b] == PF_VARIANT && !(FAIL && kind == HQ_FAIL_PREFILLED)) b = NONE;
        }
        if (REJECT) {
            const uint32_t k = retr_find(cc, id[i]), rep = cc.reporter[i], v = rj.variant[i];
            const uint32_t ev = b == NONE ? 0u : t.variant[b];
            const uint32_t cls = ev == PF_VARIANT ? hqreject::E_PF : ev == MN_VARIANT ? hqreject::E_MN : hqreject::E_SN;
            const uint32_t rq = k != NONE ? (rj.rq_in ? rj.rq_in[i] : NONE) : b != NONE ? t.rq[b] : NONE;  // the request of the task: the caller's for an override, else the entry's
            const bool v_none = v == 0xFFu, v_exists = !v_none && v < PF_VARIANT && rq != NONE && variant_ok(q, rq, v);
            const uint32_t kind = hqreject::kind_before_claim(b != NONE, cls, b != NONE && t.worker[b] == rep, ev == v, b != NONE && t.run[b] != 0, v_none, v_exists, k != NONE,
                                                              k != NONE && cc.retr_wid[k] == rep, false);
            cc.kind[i] = (uint8_t)kind;
            rj.blk_rq[i] = hqreject::blocks(kind, v_none, v_exists, row_of(r, rep) != NONE) ? rq : NONE;
            rj.flag[i] = 0;
            if (k != NONE) { if (hqreject::accepted(kind)) atomicMin(&cc.retr_hit[k], i); b = NONE; }
            else if (!hqreject::accepted(kind)) b = NONE;
        }
        pos[i] = b;
        if (b != NONE) atomicMin(&t.claim[b], i);
        if (CANCEL) {
            cc.route[i] = NONE; cc.kind[i] = HQ_CANCEL_NONE;
            const uint32_t k = retr_find(cc, id[i]);
            if (k != NONE) atomicMin(&cc.retr_hit[k], i);
        }
    }
    wave_add(&ctr[C_UNKNOWN], i < n && b == NONE);
}
// pass 2: per (worker row, resource) the position + 1 of the batch's last ALL entry
template <int MODE>
__global__ void k_rel_last_all(Table t, Req q, Rows r, uint32_t n, uint32_t *pos, uint32_t *last_all, CancelCols cc, uint32_t *ctr) {
    constexpr bool CANCEL = MODE == M_CANCEL, REPORTED = MODE == M_FINISH || MODE == M_FAIL || MODE == M_REJECT, PF_LEAVES = MODE == M_CANCEL || MODE == M_FAIL || MODE == M_REJECT;
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    const uint32_t b = i < n ? pos[i] : NONE;
    bool dup = false, bad = false;
    if (b != NONE) {
        const uint32_t row = row_of(r, t.worker[b]);
        if (t.claim[b] != i) { pos[i] = NONE; dup = true; if (CANCEL) cc.kind[i] = HQ_CANCEL_REPEAT; if (REPORTED) cc.kind[i] = (uint8_t)rep_repeat<MODE>(cc.kind[i]); }
        else if (t.variant[b] == MN_VARIANT) {}  // a multi-node task: no count, no entry of any resource (its rows are reset by pass 4)
        else if (PF_LEAVES && t.variant[b] == PF_VARIANT) {}  // a prefilled task: no count in a slot, no free row (pass 3 lowers its prefilled count)
        else if (row == NONE) { pos[i] = NONE; bad = true; t.claim[b] = NONE; }  // (left in the table, unclaimed: a later batch finds it as before)
        else {
            const uint32_t slot = q.rq_off[t.rq[b]] + t.variant[b];
            for (uint32_t e = q.ventry_off[slot]; e < q.ventry_off[slot + 1]; e++)
                if (q.ent_kind[e] == HQ_ENTRY_ALL) atomicMax(&last_all[(size_t)row * r.R + q.ent_res[e]], i + 1);
        }
    }
    wave_add(&ctr[C_DUP], dup); wave_add(&ctr[C_BAD], bad);
}
// pass 3: the AMOUNT entries behind the last ALL of their (row, resource) are summed; the entry leaves the table
// CANCEL: a prefilled entry lowers its prefilled count instead (k_pf_remove's step); before the entry leaves, its position's route (the row of the entry's
// worker: the root of a multi-node task) and kind are written.  Then the Retracting overrides: the claiming position is routed to the worker the task is
// retracting from, whatever the ledger said, and any other position of that id is a repeat.
// FINISH: the kinds are pass 1's; an eligible position of a Retracting id that did not win its override is a repeat (an id with no ledger entry has no other
// pass to learn that from).  C_OUT counts the accepted positions: those that leave the table and the Retracting ids that had no entry.
// FAIL: as FINISH, and a claimed prefilled entry leaves as in the cancel mode -- its prefilled count drops, no free row and no last-ALL word is touched, so the
// order-dependent arithmetic of the other positions never sees it.  C_OUT counts the _WAITING positions too.
// REJECT: as FAIL; every entry that leaves goes back into the ready set, so its priority and request are recorded at its position, with its flag, before the key
// becomes a tombstone (the compaction behind this pass makes the dense columns of them).  No claimed entry stays, so no claim word is left behind.
template <int MODE>
__global__ void k_rel_apply(Table t, Req q, Rows r, uint32_t n, const uint64_t *id, const uint32_t *pos, const uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr,
                            RejectCols rj) {
    constexpr bool CANCEL = MODE == M_CANCEL, REPORTED = MODE == M_FINISH || MODE == M_FAIL || MODE == M_REJECT, PF_LEAVES = MODE == M_CANCEL || MODE == M_FAIL || MODE == M_REJECT;
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    const uint32_t b = i < n ? pos[i] : NONE;
    bool mn = false, pf = false;
    if (b != NONE) {
        mn = t.variant[b] == MN_VARIANT; pf = PF_LEAVES && t.variant[b] == PF_VARIANT;
        if (pf) {
            const uint32_t row = row_of(r, t.worker[b]), rq = t.rq[b];
            if (row != NONE && r.pf && rq < r.pf_stride) atomicSub(&r.pf[(size_t)row * r.pf_stride + rq], 1u);
        } else if (!mn) {
            const uint32_t row = row_of(r, t.worker[b]);
            const uint32_t slot = q.rq_off[t.rq[b]] + t.variant[b];
            for (uint32_t e = q.ventry_off[slot]; e < q.ventry_off[slot + 1]; e++) {
                const size_t j = (size_t)row * r.R + q.ent_res[e];
                if (q.ent_kind[e] == HQ_ENTRY_AMOUNT && i + 1 > last_all[j]) atomicAdd(reinterpret_cast<unsigned long long *>(&delta[j]), (unsigned long long)q.ent_amount[e]);
            }
            atomicSub(&r.counts[(size_t)row * r.stride + slot], 1u);
        }
        if (CANCEL) { cc.route[i] = row_of(r, t.worker[b]); cc.kind[i] = pf ? HQ_CANCEL_PREFILLED : mn ? HQ_CANCEL_MN : HQ_CANCEL_ASSIGNED; }
        if (MODE == M_REJECT) { rj.rec_prio[i] = t.prio[b]; rj.rec_rq[i] = t.rq[b]; rj.flag[i] = 1; }
        t.key[b] = HT_TOMB; t.claim[b] = NONE;
    }
    if (CANCEL && i < n) {
        const uint32_t k = retr_find(cc, id[i]);
        if (k != NONE) {
            const bool first = cc.retr_hit[k] == i;
            cc.route[i] = first ? row_of(r, cc.retr_wid[k]) : NONE; cc.kind[i] = first ? HQ_CANCEL_RETRACTING : HQ_CANCEL_REPEAT;
        }
    }
    bool acc = false;
    if (REPORTED && i < n) {
        uint32_t kind = cc.kind[i];
        if (kind == rep_retracting<MODE>()) {
            const uint32_t k = retr_find(cc, id[i]);
            if (k == NONE || cc.retr_hit[k] != i) { kind = rep_repeat<MODE>(kind); cc.kind[i] = (uint8_t)kind; }
        }
        acc = rep_accepted<MODE>(kind);
    }
    wave_add(&ctr[C_DONE], b != NONE); wave_add(&ctr[C_MN], mn);
    if (PF_LEAVES) wave_add(&ctr[C_PF], pf);
    if (REPORTED) wave_add(&ctr[C_OUT], acc);
}
// reset_mn_task (worker.rs:172-175) of a row whose multi-node task has left the table: SN bit set, free row = total row, columns cleared
__device__ __forceinline__ void mn_reset_row(const Table &t, const Rows &r, const MnRows &m, uint32_t row) {
    const uint64_t id = m.task[row];
    if (id == HT_EMPTY || ht_find(t, id) != NONE) return;
    for (uint32_t c = 0; c < r.R; c++) r.free_[(size_t)row * r.R + c] = r.total[(size_t)row * r.R + c];
    m.task[row] = HT_EMPTY; m.root[row] = 0; m.flags[row] = (uint8_t)(m.flags[row] | HQ_WORKER_SN);
}
// pass 4: free.add per (row, resource) — ALL sets the total (workerload.rs:194-202), the AMOUNTs after it add
__global__ void k_rel_rows(Table t, Rows r, MnRows m, uint32_t *last_all, uint64_t *delta) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= r.W * r.R) return;
    const uint32_t la = last_all[j]; const uint64_t d = delta[j];
    if (la) r.free_[j] = r.total[j] + d; else if (d) r.free_[j] += d;
    last_all[j] = 0; delta[j] = 0;
    // multi-node tasks of the batch (pass 3 took their entries out): the thread of a row's first resource resets the whole row.  A row that holds a multi-node
    // task holds no single-node task (Worker::set_mn_task wants is_free), so no entry of the batch names it: la == 0 and d == 0 in all its R threads, nothing
    // above wrote its free row, and the last-ALL ordering of the other rows is untouched.  m.live == 0 (uniform): the columns are not read at all.
    if (m.live && j % r.R == 0) mn_reset_row(t, r, m, j / r.R);
}
__global__ void k_mn_reset_rows(Table t, Rows r, MnRows m) {
    const uint32_t row = blockIdx.x * TPB + threadIdx.x;
    if (row < r.W) mn_reset_row(t, r, m, row);
}
// multi-node placements, pass 1: per worker row the first task of the batch that lists it
__global__ void k_mn_claim(Rows r, MnItems it, uint32_t *owner) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= it.n_wid) return;
    uint32_t lo = 0, hi = it.n;  // the task whose list holds position j: the last i with off[i] <= j
    while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (it.off[mid] <= j) lo = mid; else hi = mid; }
    const uint32_t row = row_of(r, it.wid[j]);
    if (row != NONE) atomicMin(&owner[row], lo);
}
// pass 2: one thread per task (a task has a handful of workers; a tick places few of them)
__global__ void k_mn_enter(Table t, Rows r, MnRows m, MnItems it, const uint32_t *owner, int check, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    int status = S_SKIP;
    if (i < it.n) {
        const uint64_t id = it.id[i];
        const uint32_t b0 = it.off[i], b1 = it.off[i + 1];
        uint64_t prio = 0;
        bool ok = id < HT_TOMB && b0 < b1 && b1 <= it.n_wid;
        if (ok && it.prio) prio = it.prio[i];
        else if (ok) { const uint64_t c = col_find(it.col_id, it.col_n, id); ok = c != ~0ull; if (ok) prio = it.col_prio[c]; }
        for (uint32_t j = b0; ok && j < b1; j++) {
            const uint32_t row = row_of(r, it.wid[j]);
            ok = row != NONE && owner[row] == i && m.task[row] == HT_EMPTY;
            for (uint32_t k = b0; ok && k < j; k++) ok = it.wid[k] != it.wid[j];
            if (ok && check) {  // Worker::is_free (worker.rs:134-137), or a worker uploaded without its SN bit that holds nothing yet
                ok = (m.flags[row] & HQ_WORKER_STOPPING) == 0;
                for (uint32_t c = 0; ok && c < r.stride; c++) ok = r.counts[(size_t)row * r.stride + c] == 0;
            }
        }
        status = S_BAD;
        if (ok) {
            int fresh = 0;
            const uint32_t b = ht_claim(t, id, &fresh);
            if (b == NONE) status = S_FULL;
            else if (!fresh) status = S_DUP;
            else {
                t.worker[b] = it.wid[b0]; t.rq[b] = it.rq[i]; t.variant[b] = MN_VARIANT; t.prio[b] = prio; t.claim[b] = NONE; t.run[b] = 0;
                for (uint32_t j = b0; j < b1; j++) {  // set_mn_task (worker.rs:160-166): the free row stays as it is
                    const uint32_t row = row_of(r, it.wid[j]);
                    m.task[row] = id; m.root[row] = j == b0 ? 1 : 0; m.flags[row] = (uint8_t)(m.flags[row] & ~HQ_WORKER_SN);
                }
                status = S_FRESH;
            }
        }
    }
    count_status(ctr, status);
}

__global__ void k_evict(Table t, uint32_t n_lost, const uint32_t *lost, uint64_t *out_id, uint32_t *out_rq, uint64_t *out_prio, uint8_t *out_var, uint8_t *out_run, uint32_t cap_out,
                        uint32_t *ctr) {
    const uint32_t b = blockIdx.x * TPB + threadIdx.x;
    const uint64_t k = b <= t.mask ? t.key[b] : HT_EMPTY;
    bool hit = false;
    if (k < HT_TOMB) {
        const uint32_t w = t.worker[b];
        uint32_t lo = 0, hi = n_lost;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (lost[mid] < w) lo = mid + 1; else hi = mid; }
        hit = lo < n_lost && lost[lo] == w;
    }
    wave_add(&ctr[C_MN], hit && t.variant[b] == MN_VARIANT);  // (its worker column is the root: a lost root evicts the task, reactor.rs:107-128)
    wave_add(&ctr[C_PF], hit && t.variant[b] == PF_VARIANT);  // (move_prefilled_task_to_ready; the row's prefilled counts go with the row in the re-pack)
    const uint32_t o = wave_append(&ctr[C_OUT], hit);
    if (!hit || o >= cap_out) return;  // (the host sized the output by its live count: more is reported as an error and nothing is written past the end)
    out_id[o] = k; out_rq[o] = t.rq[b]; out_prio[o] = t.prio[b]; out_var[o] = t.variant[b]; out_run[o] = t.run[b];
    t.key[b] = HT_TOMB;
}

// ---- prefilled tasks (r.pf != nullptr) ----
__global__ void k_pf_seed(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint64_t *prio, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    int status = S_SKIP;
    if (i < n) {
        const uint32_t row = row_of(r, wid[i]);
        status = (row == NONE || !(m.flags[row] & HQ_WORKER_SN)) ? S_BAD : enter_pf(t, q, r, id[i], row, wid[i], rq[i], prio[i]);
    }
    count_status(ctr, status);
}
// the variant byte of bucket b goes from PF_VARIANT to v, atomically on its 32-bit word (the buckets beside it may change in the same launch): true for the
// one thread that made the change
__device__ __forceinline__ bool pf_take_variant(const Table &t, uint32_t b, uint8_t v) {
    unsigned int *word = reinterpret_cast<unsigned int *>(t.variant) + (b >> 2);
    const unsigned int sh = (b & 3u) * 8u;
    unsigned int cur = __atomic_load_n(word, __ATOMIC_RELAXED);
    for (;;) {
        if (((cur >> sh) & 0xFFu) != PF_VARIANT) return false;
        const unsigned int want = (cur & ~(0xFFu << sh)) | ((unsigned int)v << sh);
        const unsigned int got = atomicCAS(word, cur, want);
        if (got == cur) return true;
        cur = got;
    }
}
// task_from_prefilled_to_started (worker.rs:212-221): every step is an atomic that commutes with the others of the batch
__global__ void k_pf_start(Table t, Req q, Rows r, uint32_t n, const uint64_t *id, const uint8_t *variant, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    bool done = false, unknown = false, bad = false;
    if (i < n) {
        const uint32_t b = id[i] < HT_TOMB ? ht_find(t, id[i]) : NONE;
        if (b == NONE) unknown = true;
        else {
            const uint32_t rq = t.rq[b], v = variant[i], row = row_of(r, t.worker[b]);  // (these columns of a prefilled entry do not change in this launch)
            if (v >= PF_VARIANT || !variant_ok(q, rq, v) || q.rq_off[rq] + v >= r.stride || row == NONE || rq >= r.pf_stride) {
                const uint8_t cur = t.variant[b];
                if (cur == PF_VARIANT) bad = true; else unknown = true;
            } else if (!pf_take_variant(t, b, (uint8_t)v)) unknown = true;  // an assigned entry, or a repeat of the id within the batch
            else {
                const uint32_t slot = q.rq_off[rq] + v;
                atomicSub(&r.pf[(size_t)row * r.pf_stride + rq], 1u);
                atomicAdd(&r.counts[(size_t)row * r.stride + slot], 1u);
                for (uint32_t e = q.ventry_off[slot]; e < q.ventry_off[slot + 1]; e++) free_remove(&r.free_[(size_t)row * r.R + q.ent_res[e]], q.ent_kind[e], q.ent_amount[e]);
                t.run[b] = 1;  // (the one thread that took the variant: the task runs)
                done = true;
            }
        }
    }
    wave_add(&ctr[C_DONE], done); wave_add(&ctr[C_UNKNOWN], unknown); wave_add(&ctr[C_BAD], bad);
}
// remove_prefill_task outside a tick: the one thread that turns the key into a tombstone takes the count down
__global__ void k_pf_remove(Table t, Rows r, uint32_t n, const uint64_t *id, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    bool done = false;
    if (i < n && id[i] < HT_TOMB) {
        const uint32_t b = ht_find(t, id[i]);
        if (b != NONE && t.variant[b] == PF_VARIANT) {
            const uint32_t rq = t.rq[b], row = row_of(r, t.worker[b]);
            done = atomicCAS(reinterpret_cast<unsigned long long *>(&t.key[b]), (unsigned long long)id[i], (unsigned long long)HT_TOMB) == id[i];
            if (done && row != NONE && rq < r.pf_stride) atomicSub(&r.pf[(size_t)row * r.pf_stride + rq], 1u);
        }
    }
    wave_add(&ctr[C_DONE], done); wave_add(&ctr[C_UNKNOWN], i < n && !done);
}
__global__ void k_pf_drop_all(Table t, uint32_t *ctr) {
    const uint32_t b = blockIdx.x * TPB + threadIdx.x;
    const bool hit = b <= t.mask && t.key[b] < HT_TOMB && t.variant[b] == PF_VARIANT;
    if (hit) t.key[b] = HT_TOMB;
    wave_add(&ctr[C_DONE], hit);
}

__global__ void k_rehash(Table from, Table to, uint32_t *ctr) {
    const uint32_t b = blockIdx.x * TPB + threadIdx.x;
    const uint64_t k = b <= from.mask ? from.key[b] : HT_EMPTY;
    uint32_t d = NONE;
    if (k < HT_TOMB) {
        int fresh = 0;
        d = ht_claim(to, k, &fresh);
        if (d != NONE) { to.worker[d] = from.worker[b]; to.rq[d] = from.rq[b]; to.variant[d] = from.variant[b]; to.prio[d] = from.prio[b]; to.claim[d] = NONE; to.run[d] = from.run[b]; }
    }
    wave_add(&ctr[C_DONE], k < HT_TOMB && d != NONE); wave_add(&ctr[C_FULL], k < HT_TOMB && d == NONE);
}

__global__ void k_repack_counts(const uint32_t *src, uint32_t src_stride, uint32_t W_src, const uint32_t *src_row, uint32_t W_dst, uint32_t *dst, uint32_t dst_stride, uint32_t n_cols,
                                MnRows ms, MnRows md, const uint8_t *new_flags, PfMove pf) {
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (j >= (uint64_t)W_dst * n_cols) return;
    const uint32_t w = (uint32_t)(j / n_cols), c = (uint32_t)(j % n_cols);
    const uint32_t sr = src_row ? src_row[w] : w;
    dst[(size_t)w * dst_stride + c] = sr < W_src ? src[(size_t)sr * src_stride + c] : 0u;
    if (pf.dst && c < pf.n_cols) pf.dst[(size_t)w * pf.dst_stride + c] = sr < W_src ? pf.src[(size_t)sr * pf.src_stride + c] : 0u;  // (pf.dst == nullptr, uniform: not tracked)
    if (c == 0 && md.task) {  // the row's multi-node columns travel with its first count
        const bool old = sr < W_src;
        md.task[w] = old ? ms.task[sr] : HT_EMPTY; md.root[w] = old ? ms.root[sr] : (uint8_t)0; md.flags[w] = old ? ms.flags[sr] : new_flags[w];
    }
}

__global__ void k_lookup(Table t, uint32_t n, const uint64_t *id, uint32_t *out_wid, uint8_t *out_variant) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = id[i] < HT_TOMB ? ht_find(t, id[i]) : NONE;
    out_wid[i] = b == NONE ? HQ_NO_WORKER : t.worker[b];
    out_variant[i] = b == NONE ? (uint8_t)0xFF : t.variant[b];
}
__global__ void k_running(Table t, uint32_t n, const uint64_t *id, uint8_t *out_run) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = id[i] < HT_TOMB ? ht_find(t, id[i]) : NONE;
    out_run[i] = b == NONE ? (uint8_t)0xFF : t.run[b];
}

// ---- hqtick_start_tasks: task_running for the staged positions [lo, hi); a position with a mask byte is the host's (an id of the Retracting table)
// pass 1: the bucket of every id and start_core.h's rule on the tables as they are.  Only an _ASSIGNED or _PREFILLED position keeps its bucket in pos and claims it;
// every other position has pos NONE and is final here.
__global__ void k_start_claim(Table t, Req q, Rows r, StartCols sc, uint32_t lo, uint32_t hi) {
    const uint32_t i = lo + blockIdx.x * TPB + threadIdx.x;
    if (i >= hi || (sc.mask && sc.mask[i])) return;
    const uint64_t id = sc.id[i];
    const uint32_t b = id < HT_TOMB ? ht_find(t, id) : NONE;
    uint32_t kind = HQ_START_NONE;
    if (b != NONE) {
        const uint32_t ev = t.variant[b], v = sc.variant[i], rq = t.rq[b];
        const uint32_t cls = ev == PF_VARIANT ? hqstart::E_PF : ev == MN_VARIANT ? hqstart::E_MN : hqstart::E_SN;
        bool v_exists = false;
        if (cls == hqstart::E_PF)  // what pf_start wants of the variant: the request has it, its slot and the row are in the tables
            v_exists = v < PF_VARIANT && variant_ok(q, rq, v) && q.rq_off[rq] + v < r.stride && r.pf && rq < r.pf_stride && row_of(r, t.worker[b]) != NONE;
        kind = hqstart::kind_before_claim(true, cls, t.worker[b] == sc.reporter[i], ev == v, t.run[b] != 0, v_exists, false, false);
    }
    const bool claims = kind == HQ_START_ASSIGNED || kind == HQ_START_PREFILLED;
    sc.kind[i] = (uint8_t)kind; sc.pos[i] = claims ? b : NONE;
    if (claims) atomicMin(&t.claim[b], i);
}
// pass 2: the winner of a claim starts its task and gives the claim word back; a loser is a repeat
__global__ void k_start_apply(Table t, Req q, Rows r, StartCols sc, uint32_t lo, uint32_t hi, uint32_t *ctr) {
    const uint32_t i = lo + blockIdx.x * TPB + threadIdx.x;
    bool acc = false, pf = false, mn = false;
    if (i < hi && !(sc.mask && sc.mask[i])) {
        const uint32_t b = sc.pos[i];
        if (b == NONE) mn = acc = sc.kind[i] == HQ_START_MN;
        else if (t.claim[b] != i) sc.kind[i] = HQ_START_REPEAT;
        else {
            acc = true; pf = sc.kind[i] == HQ_START_PREFILLED;
            if (pf) {  // task_from_prefilled_to_started with the winner's variant: k_pf_start's arithmetic; the claim made the writer of the byte unique
                const uint32_t rq = t.rq[b], v = sc.variant[i], row = row_of(r, t.worker[b]), slot = q.rq_off[rq] + v;
                t.variant[b] = (uint8_t)v;
                atomicSub(&r.pf[(size_t)row * r.pf_stride + rq], 1u);
                atomicAdd(&r.counts[(size_t)row * r.stride + slot], 1u);
                for (uint32_t e = q.ventry_off[slot]; e < q.ventry_off[slot + 1]; e++) free_remove(&r.free_[(size_t)row * r.R + q.ent_res[e]], q.ent_kind[e], q.ent_amount[e]);
            }
            t.run[b] = 1;
            t.claim[b] = NONE;  // the entry stays: a word left here would beat every later batch's claim of this id
        }
    }
    wave_add(&ctr[C_OUT], acc); wave_add(&ctr[C_PF], pf); wave_add(&ctr[C_MN], mn);
}
__global__ void k_start_unclaim(Table t, StartCols sc, uint32_t lo, uint32_t hi) {
    const uint32_t i = lo + blockIdx.x * TPB + threadIdx.x;
    if (i >= hi || (sc.mask && sc.mask[i])) return;
    const uint32_t b = sc.pos[i];
    if (b != NONE && b <= t.mask) t.claim[b] = NONE;
}

// ---- hqtick_reject_tasks: the requeue's compaction.  perm lists the batch positions by ascending (id, position); the apply pass left a flag, a
// priority and a request at every position whose entry went back.  One wavefront per 256-entry slice of perm, as the ready set's rebuild walks its columns.
// pass 1: flagged positions per slice
__global__ void __launch_bounds__(TPB) k_rej_count(RejectCols rj, uint32_t n, uint32_t n_slices) {
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = __lane_id();
    if (wave >= n_slices) return;
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t j = wave * 256 + (uint32_t)u * 64 + lane;
        const uint32_t p = j < n ? rj.perm[j] : NONE;
        c += (uint32_t)__popcll(__ballot(p < n && rj.flag[p] != 0));
    }
    if (lane == 0) rj.slices[wave] = c;
}
// pass 2 (behind the scan of the slice table): entry j of perm lands at slice offset + flagged entries before it in the slice
__global__ void __launch_bounds__(TPB) k_rej_compact(RejectCols rj, const uint64_t *id, uint32_t n, uint32_t n_slices) {
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = __lane_id();
    if (wave >= n_slices) return;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t run = rj.slices[wave];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t j = wave * 256 + (uint32_t)u * 64 + lane;
        const uint32_t p = j < n ? rj.perm[j] : NONE;
        const bool f = p < n && rj.flag[p] != 0;
        const uint64_t b = __ballot(f);
        const uint32_t dst = run + (uint32_t)__popcll(b & lt);
        run += (uint32_t)__popcll(b);
        if (!f || dst >= n) continue;  // (at most n flags: the bound holds whatever perm lists)
        const uint64_t k = id[p], pr = rj.rec_prio[p]; const uint32_t rq = rj.rec_rq[p];
        rj.out_id[dst] = k; rj.out_prio[dst] = pr; rj.out_rq[dst] = rq;
        rj.o_id[dst] = k; rj.o_prio[dst] = pr; rj.o_rq[dst] = rq;
    }
}

// ---- hqtick_lose_workers.  The append of the eviction is the only place where the order of arrival shows; the sort by id behind it removes it,
// and everything after the sort writes position j from the sorted arrays alone.
// index of worker id w in the sorted list (NONE: not lost)
__device__ __forceinline__ uint32_t lost_find(const uint32_t *lost, uint32_t n_lost, uint32_t w) {
    uint32_t lo = 0, hi = n_lost;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (lost[mid] < w) lo = mid + 1; else hi = mid; }
    return lo < n_lost && lost[lo] == w ? lo : NONE;
}
// k_evict's pass; a hit leaves (id, bucket) for the sort instead of its columns
__global__ void __launch_bounds__(TPB) k_lose_evict(Table t, LoseCols lc, uint32_t cap_out, uint32_t *ctr) {
    const uint32_t b = blockIdx.x * TPB + threadIdx.x;
    const uint64_t k = b <= t.mask ? t.key[b] : HT_EMPTY;
    const bool hit = k < HT_TOMB && lost_find(lc.lost, lc.n_lost, t.worker[b]) != NONE;
    const uint8_t v = hit ? t.variant[b] : (uint8_t)0;
    wave_add(&ctr[C_MN], hit && v == MN_VARIANT);
    wave_add(&ctr[C_PF], hit && v == PF_VARIANT);
    const uint32_t o = wave_append(&ctr[C_OUT], hit);
    if (!hit || o >= cap_out) return;  // (sized by the host's live count: more is reported as an error and nothing is written past the end)
    lc.skey[o] = k; lc.sval[o] = b;
    t.key[b] = HT_TOMB;
}
// the lost NON-root members of multi-node tasks, one thread per lost worker of the caller's list; behind the eviction (a task whose root was lost with it is no
// longer found) and before the rows are reset or re-packed
__global__ void __launch_bounds__(TPB) k_lose_mn(Table t, Rows r, MnRows m, LoseCols lc) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= lc.n_lost) return;
    uint64_t task = HT_EMPTY; uint32_t root = NONE;
    const uint32_t row = row_of(r, lc.call[i]);
    if (row != NONE && m.task[row] != HT_EMPTY && m.root[row] == 0) {
        const uint32_t b = ht_find(t, m.task[row]);
        if (b != NONE) { task = m.task[row]; root = t.worker[b]; }
    }
    lc.mn_task[i] = task; lc.mn_root[i] = root;
}
// sorted position j: the entry's columns from its bucket (the tombstone left them), the kind, the worker's index in the caller's list
__global__ void __launch_bounds__(TPB) k_lose_gather(Table t, LoseCols lc, uint32_t k) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= k) return;
    const uint64_t id = lc.skey[j];
    const uint32_t b = lc.sval[j] & t.mask;  // (a bucket the eviction wrote; the mask keeps every read inside the table whatever the pair holds)
    const uint64_t pr = t.prio[b]; const uint32_t rq = t.rq[b]; const uint8_t v = t.variant[b];
    const uint32_t at = lost_find(lc.lost, lc.n_lost, t.worker[b]);
    lc.id[j] = id; lc.prio[j] = pr; lc.rq[j] = rq;
    lc.o_id[j] = id; lc.o_prio[j] = pr; lc.o_rq[j] = rq;
    lc.kind[j] = (uint8_t)hqlose::kind_of_entry(v == MN_VARIANT ? hqlose::E_MN : v == PF_VARIANT ? hqlose::E_PF : hqlose::E_SN, t.run[b] != 0);
    lc.widx[j] = at != NONE ? lc.lost_idx[at] : 0u;  // (every evicted entry's worker is in the list; 0 keeps the key a valid index if the table were damaged)
}
// offsets and CSR columns from the sorted worker indices: lose_core.h's two phases, one thread per offset and per element
__global__ void __launch_bounds__(TPB) k_lose_group(hqlose::GroupArgs a) {
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    hqlose::grp_p_offset(a, g);
    hqlose::grp_p_gather(a, g);
}

}  // namespace

hipError_t lose_evict(Table t, Rows r, MnRows m, LoseCols lc, uint32_t cap_out, uint32_t *ctr, hipStream_t s) {
    hipLaunchKernelGGL(k_lose_evict, dim3(nblk((uint64_t)t.mask + 1)), dim3(TPB), 0, s, t, lc, cap_out, ctr);
    if (m.live && lc.n_lost) hipLaunchKernelGGL(k_lose_mn, dim3(nblk(lc.n_lost)), dim3(TPB), 0, s, t, r, m, lc);
    return hipGetLastError();
}
hipError_t lose_gather(Table t, LoseCols lc, uint32_t k, hipStream_t s) {
    if (!k) return hipSuccess;
    hipLaunchKernelGGL(k_lose_gather, dim3(nblk(k)), dim3(TPB), 0, s, t, lc, k);
    return hipGetLastError();
}
hipError_t lose_group(LoseCols lc, uint32_t k, hipStream_t s) {
    const uint32_t *key = nullptr, *pos = nullptr;
    if (k) { if (hipError_t rc = hqcancel::sort_rows(k, lc.n_lost, lc.widx, lc.scratch, &key, &pos, s); rc != hipSuccess) return rc; }
    const hqlose::GroupArgs a{k, lc.n_lost, key, pos, lc.id, lc.prio, lc.rq, lc.kind, lc.c_off, lc.c_id, lc.c_prio, lc.c_rq, lc.c_kind};
    hipLaunchKernelGGL(k_lose_group, dim3(nblk((uint64_t)k > (uint64_t)lc.n_lost + 1 ? (uint64_t)k : (uint64_t)lc.n_lost + 1)), dim3(TPB), 0, s, a);
    return hipGetLastError();
}


hipError_t clear(Table t, hipStream_t s) {
    hipLaunchKernelGGL(k_clear, dim3(nblk((uint64_t)t.mask + 1)), dim3(TPB), 0, s, t);
    return hipGetLastError();
}
hipError_t insert(Table t, Req q, Rows r, Items it, int upsert, int apply_free, uint32_t *ctr, hipStream_t s) {
    if (!it.n) return hipSuccess;
    hipLaunchKernelGGL(k_insert, dim3(nblk(it.n)), dim3(TPB), 0, s, t, q, r, it, upsert, apply_free, ctr);
    return hipGetLastError();
}
hipError_t insert_staged(Table t, Req q, Rows r, Staged st, uint32_t *ctr, hipStream_t s) {
    if (!st.n) return hipSuccess;
    hipLaunchKernelGGL(k_insert_staged, dim3(nblk(st.n)), dim3(TPB), 0, s, t, q, r, st, ctr);
    return hipGetLastError();
}
hipError_t release(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, uint32_t *ctr, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rel_claim<M_RELEASE>, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, pos, CancelCols{}, ctr, q, r, RejectCols{});
    hipLaunchKernelGGL(k_rel_last_all<M_RELEASE>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, pos, last_all, CancelCols{}, ctr);
    hipLaunchKernelGGL(k_rel_apply<M_RELEASE>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, id, pos, last_all, delta, CancelCols{}, ctr, RejectCols{});
    if (r.W && r.R) hipLaunchKernelGGL(k_rel_rows, dim3(nblk((uint64_t)r.W * r.R)), dim3(TPB), 0, s, t, r, m, last_all, delta);
    return hipGetLastError();
}
hipError_t cancel(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rel_claim<M_CANCEL>, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, pos, cc, ctr, q, r, RejectCols{});
    hipLaunchKernelGGL(k_rel_last_all<M_CANCEL>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, pos, last_all, cc, ctr);
    hipLaunchKernelGGL(k_rel_apply<M_CANCEL>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, id, pos, last_all, delta, cc, ctr, RejectCols{});
    if (r.W && r.R) hipLaunchKernelGGL(k_rel_rows, dim3(nblk((uint64_t)r.W * r.R)), dim3(TPB), 0, s, t, r, m, last_all, delta);
    return hipGetLastError();
}
hipError_t finish(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rel_claim<M_FINISH>, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, pos, cc, ctr, q, r, RejectCols{});
    hipLaunchKernelGGL(k_rel_last_all<M_FINISH>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, pos, last_all, cc, ctr);
    hipLaunchKernelGGL(k_rel_apply<M_FINISH>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, id, pos, last_all, delta, cc, ctr, RejectCols{});
    if (r.W && r.R) hipLaunchKernelGGL(k_rel_rows, dim3(nblk((uint64_t)r.W * r.R)), dim3(TPB), 0, s, t, r, m, last_all, delta);
    return hipGetLastError();
}
hipError_t fail(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rel_claim<M_FAIL>, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, pos, cc, ctr, q, r, RejectCols{});
    hipLaunchKernelGGL(k_rel_last_all<M_FAIL>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, pos, last_all, cc, ctr);
    hipLaunchKernelGGL(k_rel_apply<M_FAIL>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, id, pos, last_all, delta, cc, ctr, RejectCols{});
    if (r.W && r.R) hipLaunchKernelGGL(k_rel_rows, dim3(nblk((uint64_t)r.W * r.R)), dim3(TPB), 0, s, t, r, m, last_all, delta);
    return hipGetLastError();
}
hipError_t reject(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, RejectCols rj, uint32_t *ctr,
                  hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_rel_claim<M_REJECT>, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, pos, cc, ctr, q, r, rj);
    hipLaunchKernelGGL(k_rel_last_all<M_REJECT>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, pos, last_all, cc, ctr);
    hipLaunchKernelGGL(k_rel_apply<M_REJECT>, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, id, pos, last_all, delta, cc, ctr, rj);
    if (r.W && r.R) hipLaunchKernelGGL(k_rel_rows, dim3(nblk((uint64_t)r.W * r.R)), dim3(TPB), 0, s, t, r, m, last_all, delta);
    const uint32_t n_slices = (n + 255) / 256;
    hipLaunchKernelGGL(k_rej_count, dim3((n_slices + 3) / 4), dim3(TPB), 0, s, rj, n, n_slices);
    if (hipError_t e = hqk::scan_waves(rj.slices, hqk::WaveGeom{256, n_slices, 4, (n_slices + 15u) & ~15u}, 1, rj.total, nullptr, nullptr, s); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rej_compact, dim3((n_slices + 3) / 4), dim3(TPB), 0, s, rj, id, n, n_slices);
    return hipGetLastError();
}
hipError_t evict(Table t, uint32_t n_lost, const uint32_t *lost, uint64_t *out_id, uint32_t *out_rq, uint64_t *out_prio, uint8_t *out_var, uint8_t *out_run, uint32_t cap_out, uint32_t *ctr,
                 hipStream_t s) {
    if (!n_lost) return hipSuccess;
    hipLaunchKernelGGL(k_evict, dim3(nblk((uint64_t)t.mask + 1)), dim3(TPB), 0, s, t, n_lost, lost, out_id, out_rq, out_prio, out_var, out_run, cap_out, ctr);
    return hipGetLastError();
}
hipError_t pf_seed(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint64_t *prio, uint32_t *ctr, hipStream_t s) {
    if (!n || !r.pf) return hipSuccess;
    hipLaunchKernelGGL(k_pf_seed, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, m, n, id, wid, rq, prio, ctr);
    return hipGetLastError();
}
hipError_t pf_start(Table t, Req q, Rows r, uint32_t n, const uint64_t *id, const uint8_t *variant, uint32_t *ctr, hipStream_t s) {
    if (!n || !r.pf) return hipSuccess;
    hipLaunchKernelGGL(k_pf_start, dim3(nblk(n)), dim3(TPB), 0, s, t, q, r, n, id, variant, ctr);
    return hipGetLastError();
}
hipError_t pf_remove(Table t, Rows r, uint32_t n, const uint64_t *id, uint32_t *ctr, hipStream_t s) {
    if (!n || !r.pf) return hipSuccess;
    hipLaunchKernelGGL(k_pf_remove, dim3(nblk(n)), dim3(TPB), 0, s, t, r, n, id, ctr);
    return hipGetLastError();
}
hipError_t pf_drop_all(Table t, uint32_t *ctr, hipStream_t s) {
    hipLaunchKernelGGL(k_pf_drop_all, dim3(nblk((uint64_t)t.mask + 1)), dim3(TPB), 0, s, t, ctr);
    return hipGetLastError();
}
hipError_t rehash(Table from, Table to, uint32_t *ctr, hipStream_t s) {
    hipLaunchKernelGGL(k_rehash, dim3(nblk((uint64_t)from.mask + 1)), dim3(TPB), 0, s, from, to, ctr);
    return hipGetLastError();
}
hipError_t repack_counts(const uint32_t *src, uint32_t src_stride, uint32_t W_src, const uint32_t *src_row, uint32_t W_dst, uint32_t *dst, uint32_t dst_stride,
                         uint32_t n_cols, MnRows ms, MnRows md, const uint8_t *new_flags, hipStream_t s, PfMove pf) {
    if (!W_dst || !n_cols) return hipSuccess;
    hipLaunchKernelGGL(k_repack_counts, dim3(nblk((uint64_t)W_dst * n_cols)), dim3(TPB), 0, s, src, src_stride, W_src, src_row, W_dst, dst, dst_stride, n_cols, ms, md, new_flags, pf);
    return hipGetLastError();
}
hipError_t mn_enter(Table t, Rows r, MnRows m, MnItems it, uint32_t *owner, int check, uint32_t *ctr, hipStream_t s) {
    if (!it.n || !it.n_wid) return hipSuccess;
    hipLaunchKernelGGL(k_mn_claim, dim3(nblk(it.n_wid)), dim3(TPB), 0, s, r, it, owner);
    hipLaunchKernelGGL(k_mn_enter, dim3(nblk(it.n)), dim3(TPB), 0, s, t, r, m, it, owner, check, ctr);
    return hipGetLastError();
}
hipError_t mn_reset_rows(Table t, Rows r, MnRows m, hipStream_t s) {
    if (!r.W) return hipSuccess;
    hipLaunchKernelGGL(k_mn_reset_rows, dim3(nblk(r.W)), dim3(TPB), 0, s, t, r, m);
    return hipGetLastError();
}
hipError_t lookup(Table t, uint32_t n, const uint64_t *id, uint32_t *out_wid, uint8_t *out_variant, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_lookup, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, out_wid, out_variant);
    return hipGetLastError();
}
hipError_t running(Table t, uint32_t n, const uint64_t *id, uint8_t *out_run, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_running, dim3(nblk(n)), dim3(TPB), 0, s, t, n, id, out_run);
    return hipGetLastError();
}
hipError_t start_claim(Table t, Req q, Rows r, StartCols sc, uint32_t lo, uint32_t hi, hipStream_t s) {
    if (lo >= hi) return hipSuccess;
    hipLaunchKernelGGL(k_start_claim, dim3(nblk(hi - lo)), dim3(TPB), 0, s, t, q, r, sc, lo, hi);
    return hipGetLastError();
}
hipError_t start_unclaim(Table t, StartCols sc, uint32_t lo, uint32_t hi, hipStream_t s) {
    if (lo >= hi) return hipSuccess;
    hipLaunchKernelGGL(k_start_unclaim, dim3(nblk(hi - lo)), dim3(TPB), 0, s, t, sc, lo, hi);
    return hipGetLastError();
}
hipError_t start_apply(Table t, Req q, Rows r, StartCols sc, uint32_t lo, uint32_t hi, uint32_t *ctr, hipStream_t s) {
    if (lo >= hi) return hipSuccess;
    hipLaunchKernelGGL(k_start_apply, dim3(nblk(hi - lo)), dim3(TPB), 0, s, t, q, r, sc, lo, hi, ctr);
    return hipGetLastError();
}

}  // namespace hqasg
