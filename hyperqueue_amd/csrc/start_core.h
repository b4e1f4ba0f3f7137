// The decision rule of hqtick_start_tasks (include/hqtick.h): what one batch position of a task_running batch is, from what the ledger and the
// Retracting table hold for its id, who reported it and with which variant.  Plain host + device code: assigned.hip's claim pass calls it per position, the host
// calls it for the positions the Retracting table decides, and hqtick_debug_start_kind evaluates it on host arrays so that the CPU suite pins the rule itself.
#pragma once

#include <cstdint>

#include "../../include/hqtick.h"

#if defined(__HIPCC__)
#define HQ_START_HD __host__ __device__
#else
#define HQ_START_HD
#endif

namespace hqstart {

// the variant class of a ledger entry (finish_core.h's values)
enum EntryClass : uint32_t { E_SN = 0, E_MN = 1, E_PF = 2 };

HQ_START_HD inline bool accepted(uint32_t kind) { return kind == HQ_START_ASSIGNED || kind == HQ_START_MN || kind == HQ_START_PREFILLED || kind == HQ_START_RETRACTING; }
// the accepted kinds that change their task and therefore claim its id; a multi-node position changes nothing and is accepted every time it is rightly reported
HQ_START_HD inline bool eligible(uint32_t kind) { return kind == HQ_START_ASSIGNED || kind == HQ_START_PREFILLED || kind == HQ_START_RETRACTING; }

// What a position is BEFORE the claims of its id are compared (task_running's `match task.state`, reactor.rs:286-350, with the reference's assertions as kinds):
//   the id is in the Retracting table   the table decides, whatever the ledger names: reported by the worker the task is retracting FROM it is _RETRACTING
//                                       (_BAD_VARIANT if the task's request has no such variant), by anyone else _WRONG_WORKER
//   no entry                            _NONE
//   a prefilled entry                   reported by its worker _PREFILLED (_BAD_VARIANT if its request has no such variant), else _WRONG_WORKER
//   a single-node entry                 another worker _WRONG_WORKER; its worker with another variant _WRONG_VARIANT; its worker and variant: _RUNNING if the
//                                       running byte is set (unreachable! in the reference), else _ASSIGNED
//   a multi-node entry                  _MN if the reporter is the root, else _WRONG_WORKER
// entry_* are read only with entry_found, override_worker_match only with override_found; variant_exists is about the request of the entry, or of the task for
// an id of the Retracting table.
HQ_START_HD inline uint32_t kind_before_claim(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool entry_variant_match, bool entry_run, bool variant_exists,
                                              bool override_found, bool override_worker_match) {
    if (override_found) return !override_worker_match ? HQ_START_WRONG_WORKER : variant_exists ? HQ_START_RETRACTING : HQ_START_BAD_VARIANT;
    if (!entry_found) return HQ_START_NONE;
    if (!entry_worker_match) return HQ_START_WRONG_WORKER;
    if (entry_class == E_MN) return HQ_START_MN;
    if (entry_class == E_PF) return variant_exists ? HQ_START_PREFILLED : HQ_START_BAD_VARIANT;
    if (!entry_variant_match) return HQ_START_WRONG_VARIANT;
    return entry_run ? HQ_START_RUNNING : HQ_START_ASSIGNED;
}
// Only the eligible positions claim their id; the lowest of them wins.  A refused position and a multi-node one claim nothing, so they are never a repeat and
// never make one: `earlier_eligible` changes an eligible kind into _REPEAT and nothing else.
HQ_START_HD inline uint32_t after_claim(uint32_t kind, bool earlier_eligible) { return earlier_eligible && eligible(kind) ? (uint32_t)HQ_START_REPEAT : kind; }

HQ_START_HD inline uint32_t kind_of(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool entry_variant_match, bool entry_run, bool variant_exists, bool override_found,
                                    bool override_worker_match, bool earlier_eligible) {
    return after_claim(kind_before_claim(entry_found, entry_class, entry_worker_match, entry_variant_match, entry_run, variant_exists, override_found, override_worker_match), earlier_eligible);
}

}  // namespace hqstart
