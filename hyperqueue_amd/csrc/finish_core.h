// The decision rule of hqtick_finish_tasks (include/hqtick.h): what one batch position of a task_finished batch is, from what the ledger and the
// Retracting table hold for its id and who reported it.  Plain host + device code: the finish mode of assigned.hip's release passes calls it per position, and
// hqtick_debug_finish_kind evaluates it on host arrays so that the CPU suite pins the rule itself.
#pragma once

#include <cstdint>

#include "../../include/hqtick.h"

#if defined(__HIPCC__)
#define HQ_FINISH_HD __host__ __device__
#else
#define HQ_FINISH_HD
#endif

namespace hqfinish {

// the variant class of a ledger entry
enum EntryClass : uint32_t { E_SN = 0, E_MN = 1, E_PF = 2 };

HQ_FINISH_HD inline bool accepted(uint32_t kind) { return kind == HQ_FINISH_ASSIGNED || kind == HQ_FINISH_MN || kind == HQ_FINISH_RETRACTING; }

// What a position is BEFORE the claims of its id are compared (task_finished's `match task.state`, reactor.rs:529-562, with the reference's assertions as kinds):
//   the id is in the Retracting table   the table decides, whatever the ledger names (its entry, if any, is the redirect target's): reported by the worker the
//                                       task is retracting FROM it is _RETRACTING, by anyone else _WRONG_WORKER
//   a prefilled entry                   _PREFILLED whoever reports it (unreachable! in the reference)
//   a single-node / multi-node entry    _ASSIGNED / _MN if the reporter is the entry's worker (the root of a multi-node task), else _WRONG_WORKER
//   neither                             _NONE
// entry_class and entry_worker_match are read only with entry_found, override_worker_match only with override_found.
HQ_FINISH_HD inline uint32_t kind_before_claim(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool override_found, bool override_worker_match) {
    if (override_found) return override_worker_match ? HQ_FINISH_RETRACTING : HQ_FINISH_WRONG_WORKER;
    if (!entry_found) return HQ_FINISH_NONE;
    if (entry_class == E_PF) return HQ_FINISH_PREFILLED;
    if (!entry_worker_match) return HQ_FINISH_WRONG_WORKER;
    return entry_class == E_MN ? HQ_FINISH_MN : HQ_FINISH_ASSIGNED;
}
// Only the positions with an accepted kind are ELIGIBLE to claim their id; the lowest eligible position wins.  A refused position claims nothing, so it is never
// a repeat and never makes one: `earlier_accepted` changes an accepted kind into _REPEAT and nothing else.
HQ_FINISH_HD inline uint32_t after_claim(uint32_t kind, bool earlier_accepted) { return earlier_accepted && accepted(kind) ? (uint32_t)HQ_FINISH_REPEAT : kind; }

HQ_FINISH_HD inline uint32_t kind_of(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool override_found, bool override_worker_match, bool earlier_accepted) {
    return after_claim(kind_before_claim(entry_found, entry_class, entry_worker_match, override_found, override_worker_match), earlier_accepted);
}

}  // namespace hqfinish
