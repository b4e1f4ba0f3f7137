// The decision rule of hqtick_reject_tasks (include/hqtick.h): what one batch position of a task_reject batch is, from what the ledger and the
// Retracting table hold for its id, who reported it and which variant it rejected.  Plain host + device code: assigned.hip's claim pass calls it per position, the
// host settles _RETRACTING against _REDIRECTED with it, and hqtick_debug_reject_kind evaluates it on host arrays so that the CPU suite pins the rule itself.
//
// Two deliberate deviations from task_reject (server/reactor.rs:365-445):
//   - an Assigned or Prefilled task reported by a worker that does not hold it: the reference logs, then requeues the task WITHOUT releasing it from the worker that
//     holds it -- a state its own sanity_check rejects.  Here such a position is refused (_WRONG_WORKER) after its block.
//   - a reporter that is not in the resident worker set is _WRONG_WORKER and blocks nothing (the reference would not have found the worker at all).
// The reference's unreachable!() arms (multi-node, running) are refusals that change nothing.
#pragma once

#include <cstdint>

#include "../../include/hqtick.h"

#if defined(__HIPCC__)
#define HQ_REJECT_HD __host__ __device__
#else
#define HQ_REJECT_HD
#endif

namespace hqreject {

// the variant class of a ledger entry (finish_core.h's values)
enum EntryClass : uint32_t { E_SN = 0, E_MN = 1, E_PF = 2 };

HQ_REJECT_HD inline bool accepted(uint32_t kind) { return kind == HQ_REJECT_ASSIGNED || kind == HQ_REJECT_PREFILLED || kind == HQ_REJECT_RETRACTING || kind == HQ_REJECT_REDIRECTED; }
// every accepted kind changes its task and therefore claims its id
HQ_REJECT_HD inline bool eligible(uint32_t kind) { return accepted(kind); }
// the kinds whose position ran worker.block_request (reactor.rs:389-391) before the state was looked at and refused or accepted
HQ_REJECT_HD inline bool blocks_kind(uint32_t kind) { return accepted(kind) || kind == HQ_REJECT_WRONG_WORKER || kind == HQ_REJECT_WRONG_VARIANT; }
// ... and whether it adds its (request, variant) pair: a variant was named, the task's request has it, the reporter is a resident worker
HQ_REJECT_HD inline bool blocks(uint32_t kind, bool variant_none, bool variant_exists, bool reporter_resident) { return blocks_kind(kind) && !variant_none && variant_exists && reporter_resident; }
// task_reject returns true (the handler asks for scheduling) for these; a redirected task is Assigned again and needs none
HQ_REJECT_HD inline bool asks_scheduling(uint32_t kind) { return kind == HQ_REJECT_ASSIGNED || kind == HQ_REJECT_PREFILLED || kind == HQ_REJECT_RETRACTING; }

// What a position is BEFORE the claims of its id are compared:
//   the id is in the Retracting table   the table decides, whatever the ledger names: reported by anyone but the worker it is retracting FROM it is _WRONG_WORKER;
//                                       a named variant the task's request does not have is _BAD_VARIANT; else _REDIRECTED with a redirect, _RETRACTING without
//   no entry                            _NONE
//   a multi-node entry                  _MN
//   an entry of another worker          _WRONG_WORKER
//   a named variant the entry's request does not have   _BAD_VARIANT
//   a prefilled entry                   _PREFILLED (any variant, None included)
//   a single-node entry                 _RUNNING if its running byte is set; _WRONG_VARIANT for None or a variant that is not the entry's; else _ASSIGNED
// entry_* are read only with entry_found, override_* only with override_found; variant_exists is about the request of the entry, or of the task for an id of the
// Retracting table, and is read only with !variant_none.
HQ_REJECT_HD inline uint32_t kind_before_claim(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool entry_variant_match, bool entry_run, bool variant_none,
                                               bool variant_exists, bool override_found, bool override_worker_match, bool override_redirect) {
    const bool bad_variant = !variant_none && !variant_exists;
    if (override_found) return !override_worker_match ? HQ_REJECT_WRONG_WORKER : bad_variant ? HQ_REJECT_BAD_VARIANT : override_redirect ? HQ_REJECT_REDIRECTED : HQ_REJECT_RETRACTING;
    if (!entry_found) return HQ_REJECT_NONE;
    if (entry_class == E_MN) return HQ_REJECT_MN;
    if (!entry_worker_match) return HQ_REJECT_WRONG_WORKER;
    if (bad_variant) return HQ_REJECT_BAD_VARIANT;
    if (entry_class == E_PF) return HQ_REJECT_PREFILLED;
    if (entry_run) return HQ_REJECT_RUNNING;
    if (variant_none || !entry_variant_match) return HQ_REJECT_WRONG_VARIANT;
    return HQ_REJECT_ASSIGNED;
}
// Only the accepted positions claim their id; the lowest of them wins.  A refused position claims nothing, so it is never a repeat and never makes one.
HQ_REJECT_HD inline uint32_t after_claim(uint32_t kind, bool earlier_eligible) { return earlier_eligible && eligible(kind) ? (uint32_t)HQ_REJECT_REPEAT : kind; }

HQ_REJECT_HD inline uint32_t kind_of(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool entry_variant_match, bool entry_run, bool variant_none, bool variant_exists,
                                     bool override_found, bool override_worker_match, bool override_redirect, bool earlier_eligible) {
    return after_claim(kind_before_claim(entry_found, entry_class, entry_worker_match, entry_variant_match, entry_run, variant_none, variant_exists, override_found, override_worker_match,
                                         override_redirect), earlier_eligible);
}

}  // namespace hqreject
