// The host side of the resident ready set (hqtick_upload_ready, hqtick_ready_*): ReadySet owns the three columns in HBM (id, priority, request id;
// a task that left keeps its slot as a tombstone, request id RQ_TOMBSTONE, until a compaction), their alternates, the staging of the deltas, the counts, the bound
// that decides between appending and merging, and what is known of the last tick's selection.  The kernels are kernels.hip's; hqtick.cpp validates the arguments
// of the C ABI and forwards.  Like hqasg::Ledger and hqcluster::WorkerSet, a method returns an HQTICK_E_* code (negative) with `err` set and enqueues on the
// stream it is given.  The set knows nothing of the graph, the ledger or the worker set: they are handed its columns (cols()) and call its deltas.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/hqtick.h"
#include "devbuf.h"

namespace hqready {

struct Env { int device; hipStream_t stream; hipEvent_t done; bool wait_on_kernel; };  // done: carried by an append's dispatch, which the host then waits on (HQTICK_WAIT_ON_KERNEL=0: on the stream)
struct Cols { uint64_t *id, *prio; uint32_t *rq; uint64_t n; };                         // n: physical length, tombstones included

class ReadySet {
  public:
    std::string err;
    // ---- what the tick, the graph, the ledger's Env, the query and the hooks read
    bool resident() const { return resident_; }
    uint64_t live() const { return live_; }
    uint32_t appends() const { return n_appends; }  // batches written behind the columns so far (hqtick_kernel_stats.ready_appends)
    Cols cols() const { return Cols{d_id.as<uint64_t>(), d_prio.as<uint64_t>(), d_rq.as<uint32_t>(), n_}; }
    // ---- the set as a whole
    int upload(const Env &e, uint64_t n, const uint64_t *id, const uint64_t *prio, const uint32_t *rq, bool sorted);  // (validated by the caller); blocking
    int load(hipStream_t st, const hqtick_snapshot *s, bool with_ids);  // a non-resident tick's / query's columns: asynchronous, leaves resident() false
    void drop() { resident_ = false; }
    void release();
    // ---- deltas.  Each abandons the last tick's selection; a refused batch leaves the set as it was.
    int stage(uint64_t n, uint64_t **id, uint64_t **prio, uint32_t **rq);  // room for n tasks in the pinned staging buffer
    int add_staged(const Env &e, uint64_t n);                              // ... of which the first n join the set (sets the device)
    int add_packed(const Env &e, uint64_t n, uint32_t n_id_runs, const uint64_t *id_run_start, const uint32_t *id_run_len, const uint32_t *id_off, uint32_t n_prio_runs,
                   const uint64_t *prio_run_value, const uint32_t *prio_run_len, const uint16_t *task_rq);  // (the run tables validated by the caller)
    int add_device(const Env &e, const uint64_t *id, const uint64_t *prio, const uint32_t *rq, uint32_t n) { return rebuild(e, id, prio, rq, n); }  // the graph's releases: no id range on the host, always merged
    int ensure_add(uint64_t n_add);  // every buffer a later add_device of up to n_add tasks needs, so that a caller can rule its allocation failure out before it changes anything else
    int remove(const Env &e, uint64_t n, const uint64_t *host_ids);  // >= 0: how many were in the set
    int remove_device(const Env &e, const uint64_t *dev_ids, uint32_t n);
    bool compact_due() const { return n_ > 4096 && live_ * 2 < n_; }  // more tombstones than tasks, and enough rows to be worth a pass
    int compact(const Env &e) { return rebuild(e, nullptr, nullptr, nullptr, 0); }
    // ---- the last tick's selection (the launch tables that replay it are the tick's and stay with it)
    void selection_void() { valid_ = false; held_ = false; }  // the tick is overwriting the plan the selection would be replayed from
    void selected(uint32_t n_sel) { n_sel_ = n_sel; consumed_ = n_sel == 0; held_ = false; if (n_sel) valid_ = true; }
    // a tick that selected nothing may still have produced something that becomes state at the consume (redirects, multi-node placements, free rows): its caller
    // holds the empty selection, which then is live until hqtick_ready_consume_last has entered that (entered()) or a delta abandons it, like any selection
    void hold_empty() { if (!n_sel_ && consumed_) held_ = true; }
    void entered() { held_ = false; }
    void consumed_in_tick() { live_ -= n_sel_; consumed_ = true; unconfirmed_ = true; }  // HQTICK_FLAG_CONSUME_IN_TICK: the selection kernel is writing the tombstones itself
    bool unconfirmed() const { return unconfirmed_; }  // ... and its tick has not returned yet
    void confirm() { unconfirmed_ = false; }
    void put_back() { live_ += n_sel_; n_sel_ = 0; abandon_selection(); }  // that tick failed and the restore succeeded
    void lost() { resident_ = false; n_sel_ = 0; abandon_selection(); }    // ... or did not: the set is dropped
    int consumed(const Env &e);  // after the replay wrote the tombstones: counts, flags, compaction if due
    uint32_t selected_count() const { return n_sel_; }
    bool selection_valid() const { return valid_; }
    bool selection_pending() const { return !consumed_; }
    bool selection_live() const { return (valid_ && !consumed_) || held_; }

  private:
    int fail(int code, const std::string &m) { err = m; return code; }
    void abandon_selection() { valid_ = false; consumed_ = true; held_ = false; }  // the ONE place a delta invalidates the selection
    bool can_append(uint64_t n_add, uint64_t first_id, uint64_t last_id) const;
    int refused(uint32_t flag_word);  // what the append / merge kernels found wrong with a batch
    int appended(const Env &e, bool waits_on_kernel, uint64_t n_add, uint64_t last_id, const double *trace = nullptr);  // wait, decode, counts, compaction if due
    int add_columns(const Env &e, const uint64_t *id, const uint64_t *prio, const uint32_t *rq, uint32_t n, uint64_t first_id, uint64_t last_id);
    int rebuild(const Env &e, const uint64_t *aid, const uint64_t *aprio, const uint32_t *arq, uint32_t n_add);
    int mark_removed(const Env &e, const uint64_t *dev_ids, uint32_t n);

    hqbuf::DevBuf d_id, d_prio, d_rq; uint64_t n_ = 0; bool resident_ = false;
    hqbuf::DevBuf d_id2, d_prio2, d_rq2, d_slice, d_add, d_pre8;  // alternate columns (swapped in by a rebuild) + scratch of the deltas
    hqbuf::PinBuf h_add, h_addp;  // staging of a batch: three columns / the packed form (read in place by its kernel)
    hqbuf::PinBuf h_flag;         // 64 bytes the kernels report into: words 0 and 1 flags and counts, bytes 16..23 the new last id
    uint64_t live_ = 0, staged_n = 0;  // (staged_n: tasks stage() made room for, 0: nothing staged)
    uint64_t max_id = 0; bool max_id_valid = false;  // an upper bound of every resident id (the last one after an upload / a rebuild): a batch that starts above it is appended
    uint32_t n_appends = 0;
    uint32_t n_sel_ = 0; bool consumed_ = true, valid_ = false, unconfirmed_ = false, held_ = false;
};

}  // namespace hqready
