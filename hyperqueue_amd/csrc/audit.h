// The host side of hqtick_resident_check: Auditor owns the audit's scratch in HBM (4 B per graph slot for the edge census, the report's
// counters), its staging and its two events — allocated at the first call, released at hqtick_destroy — and has one method.  hqtick.cpp validates the
// arguments, builds the views (audit_core.h: State) from the const accessors of ReadySet, Graph, Ledger and Retracting, and forwards; the kernels are audit.hip's.
// Like the other host classes, run() returns an HQTICK_E_* code (negative) with `err` set; it enqueues on the stream it is given and has synchronised it when it
// returns.  Nothing it launches writes to a table it was handed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hqtick.h"
#include "audit_core.h"
#include "devbuf.h"

namespace hqaudit {

// the report in device memory: count [HQ_INV_N] | first [HQ_INV_N] | live: rows of the ready columns, slots of the graph, single-node / multi-node / prefilled
// entries of the ledger
struct Out { unsigned long long *count, *first, *live; };
constexpr size_t OUT_WORDS = 2 * HQ_INV_N + 5;

// every pass the State needs (audit_core.h: wants_*), in stream order; cnt: scratch [n_slots] u32, x: the ledger's census — both zeroed here
hipError_t launch(const State &S, Out o, uint32_t *cnt, LedgerScratch x, hipStream_t s);
// bytes of the ledger's census behind one base pointer: [cen_counts W x stride][cen_pf W x pf_stride][roots mask + 1] u32
size_t ledger_scratch_bytes(const State &S);

// the ledger's request tables as the host has them (hqasg::Ledger's vectors), staged for one call
struct ReqHost { const std::vector<uint32_t> *rq_off, *vent_off, *ent_res, *var_nodes; const std::vector<uint8_t> *ent_kind; const std::vector<uint64_t> *ent_amt; };

// the Retracting table as the host hands it over for one call
struct RetrHost { std::vector<uint64_t> task; std::vector<uint32_t> target; std::vector<uint8_t> variant, flags; };

class Auditor {
  public:
    std::string err;
    // S.retr and the request tables of S.ledger are filled in here from `retr` / `req` (copied into pinned staging the kernels read in place)
    int run(hipStream_t s, State S, const Totals &t, const RetrHost &retr, const ReqHost &req, hqtick_check_report *out);
    void release();

  private:
    int fail(int code, const std::string &m) { err = m; return code; }
    hqbuf::DevBuf d_out, d_cnt, d_led;
    hqbuf::PinBuf h_out, h_retr, h_req;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

}  // namespace hqaudit
