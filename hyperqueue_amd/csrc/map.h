// The host side of the mapping: the plan of a tick (map_core.h) and GPU phase C on it.  A Mapper owns the plan and the part of the result that
// needs no GPU output, the pinned buffer the plan's big tables are built in, the selection's output and the HBM copy of the plan, the sweep tables of K5a, the
// pinned record buffer — and what it takes to launch the last selection once more:
//   launch_sweep_early()  K5a right behind plan_keys, on the key tables alone, while the host plans redirects, prefills and outputs
//   check_capacity()      the two limits of the kernels' LDS staging, directly behind plan_outputs
//   phase_c()             pack, K4 (dense: select_scatter; view: order_select), K5a unless it went out early, K5b, the host part of the result and the caller's own work while they run, the wait
//   export_result()       the pointers of hqtick_result
//   replay_selection()    the last selection again: writing tombstones (hqtick_ready_consume_last), giving back what a failed HQTICK_FLAG_CONSUME_IN_TICK tick took,
//                         or as it was launched (hqtick_time_kernel)
// The kernels are kernels.hip's and order.hip's.  Like hqscan::Scanner, a method returns an HQTICK_E_* code (negative) with `err` set and enqueues on the stream it
// is given.  The stages of the plan are map_core.h's functions on `plan` and `res`: the tick calls them itself, between its marks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>

#include "../../include/hqtick.h"
#include "devbuf.h"
#include "kernels.h"
#include "map_core.h"
#include "ready.h"
#include "scan.h"

namespace hqmap {

struct Timeline {  // the tick's debug timeline (hqtick_timeline): us since t0
    double t0; double *tl; int *n;
    void mark() const;
};

// What the mapper uses of its context.  The event pairs are recorded only where `timing` asks for them; k5b_stop is carried by K5b's dispatch in any case — it is
// what the host waits on.
struct Env {
    hipStream_t stream;
    hipEvent_t k4_start, k4_stop, k5a_start, k5a_stop, k5b_start, k5b_stop;
    bool timing, wait_on_kernel;
    uint32_t flags;                   // of the config
    void *sink; size_t sink_bytes;    // hqtick_set_record_sink (device memory)
    uint32_t shard_index, shard_count;
    Timeline tl;
};
// A tick's phase C: the scan it follows, the ready set whose selection it becomes, and what the assignment ledger needs of it — as values.
struct PhaseC {
    const hqscan::Scan *sc; hqscan::Scanner *scan; hqready::ReadySet *ready;
    const PlanIn *in;
    bool consume_in_tick;   // K4 writes the tombstones of what it selects
    bool ledger_pfq_rq;     // pfq_rq rides behind the plan: the ledger's staging names the request of a PREFILL record
    uint32_t *saved_rq;     // where the request-id column is copied before K4 tombstones it (null: not needed)
    hqk::Stage stage;       // K5b's staging of the placement (task == nullptr: none)
    // (may be null) host work that needs nothing of phase C's output, run once behind assemble_host_part, before the wait — as hqscan::Scanner::scan's.  Not run
    // when phase_c returns an error before it gets there.
    const std::function<void()> *while_gpu_runs;
};
struct Timings { double select_us = -1, sweep_us = -1, other_us = -1; };  // of the last phase_c(); < 0: not measured
enum Replay { REPLAY_TOMBSTONE, REPLAY_RESTORE, REPLAY_TIMED };

class Mapper {
  public:
    std::string err;
    Plan plan;
    HostResult res;
    void release();
    static uint32_t *plan_storage(void *mapper, size_t words);  // PlanIn::storage of a tick: the head of the pinned plan buffer
    int launch_sweep_early(const Env &e);
    int check_capacity(bool ordered);
    int phase_c(const Env &e, const PhaseC &pc);
    void export_result(const Env &e, const hqhost::Counts &cnt, hqtick_result *out);
    const Timings &timings() const { return t_; }
    // The tick discards the phase C it has just waited for (a deferred row check that failed): nothing of its launches is replayed or timed again.
    void forget_selection() { sweep_launched = false; last_ordered = false; last_os = hqk::OrderSelect{}; last_geom = hqk::WaveGeom{}; last_L = last_Q = last_G = 0; last_tb = last_plan_bytes = 0; t_ = Timings{}; }
    // The last selection (ready.selection_valid()) once more, on the tables its tick left.  REPLAY_RESTORE waits and returns 0 only if the request ids are back
    // (scratch: 64 pinned bytes for the kernel's count); REPLAY_TIMED is the dense K4 as the tick launched it, plan copy included.
    int replay_selection(hipStream_t st, Replay mode, const hqready::Cols &cols, const hqscan::Scanner &scan, uint32_t n_sel, hqbuf::PinBuf *scratch = nullptr);
    struct Last { bool ordered; hqk::WaveGeom geom; uint32_t L, Q, G; };  // what K1 / K1b are re-launched on (hqtick_time_kernel)
    Last last_selection() const { return Last{last_ordered, last_geom, last_L, last_Q, last_G}; }

  private:
    int fail(int code, const std::string &m) { err = m; return code; }

    hqbuf::DevBuf d_sel_task, d_sel_level, d_map, d_tsweep, d_bits, d_pre;
    hqbuf::PinBuf h_plan, h_rec, h_sinkhdr, h_k5a;
    bool sweep_inflight = false;  // an early K5a launch not yet covered by a stream synchronisation
    bool sweep_launched = false;  // K5a went out right after the key tables (launch_sweep_early)
    // layout of the pinned record buffer of the last phase_c()
    size_t o_rv = 0, o_rk = 0, o_mn = 0, o_fl = 0, o_rs = 0, o_rf = 0; bool delta16 = false;
    // launch state of the last selection
    bool last_ordered = false; hqk::OrderSelect last_os{};  // the view's: its tables (HBM copy of the plan, the permutation)
    hqk::WaveGeom last_geom{}; uint32_t last_L = 0, last_Q = 0, last_G = 0; size_t last_tb = 0, last_plan_bytes = 0;
    Timings t_;
};

}  // namespace hqmap
