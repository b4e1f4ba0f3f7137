// The decision rule of hqtick_fail_tasks (include/hqtick.h): what one batch position of a task_failed batch is, from what the ledger and the
// Retracting table hold for its id and who reported it.  Plain host + device code: the fail mode of assigned.hip's release passes calls it per position, and
// hqtick_debug_fail_kind evaluates it on host arrays so that the CPU suite pins the rule itself.  The graph step (graph.hip) can only REFUSE what this rule
// accepted as _WAITING: _NONE (the graph does not know the id), _REPEAT (an earlier _WAITING position of the id) or _GONE (an earlier position's closure holds it).
#pragma once

#include <cstdint>

#include "../../include/hqtick.h"

#if defined(__HIPCC__)
#define HQ_FAIL_HD __host__ __device__
#else
#define HQ_FAIL_HD
#endif

namespace hqfail {

// the variant class of a ledger entry (finish_core.h's values)
enum EntryClass : uint32_t { E_SN = 0, E_MN = 1, E_PF = 2 };

HQ_FAIL_HD inline bool accepted(uint32_t kind) { return kind >= HQ_FAIL_ASSIGNED && kind <= HQ_FAIL_WAITING; }
// the accepted kinds that hold something in the ledger or the Retracting table (a _WAITING position holds neither)
HQ_FAIL_HD inline bool holds_entry(uint32_t kind) { return kind >= HQ_FAIL_ASSIGNED && kind <= HQ_FAIL_RETRACTING; }

// What a position is BEFORE the claims of its id are compared (task_failed's arms, reactor.rs:624-669, with the reference's assertions as kinds):
//   reported by HQ_NO_WORKER            the server's own task_failed(None, ..): _WAITING if the id has neither an entry nor a place in the Retracting table,
//                                       else _NOT_WAITING (assert!(task.is_waiting()))
//   the id is in the Retracting table   the table decides, whatever the ledger names (its entry, if any, is the redirect target's): reported by the worker the
//                                       task is retracting FROM it is _RETRACTING, by anyone else _WRONG_WORKER
//   no entry                            _NONE
//   an entry of any class               _ASSIGNED / _MN / _PREFILLED if the reporter is the entry's worker (the root of a multi-node task), else _WRONG_WORKER
// entry_class and entry_worker_match are read only with entry_found, override_worker_match only with override_found.
HQ_FAIL_HD inline uint32_t kind_before_claim(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool override_found, bool override_worker_match, bool reporter_none) {
    if (reporter_none) return entry_found || override_found ? HQ_FAIL_NOT_WAITING : HQ_FAIL_WAITING;
    if (override_found) return override_worker_match ? HQ_FAIL_RETRACTING : HQ_FAIL_WRONG_WORKER;
    if (!entry_found) return HQ_FAIL_NONE;
    if (!entry_worker_match) return HQ_FAIL_WRONG_WORKER;
    return entry_class == E_PF ? HQ_FAIL_PREFILLED : entry_class == E_MN ? HQ_FAIL_MN : HQ_FAIL_ASSIGNED;
}
// Only the positions with an accepted kind are ELIGIBLE to claim their id; the lowest eligible position wins.  A refused position claims nothing, so it is never
// a repeat and never makes one: `earlier_accepted` changes an accepted kind into _REPEAT and nothing else.
HQ_FAIL_HD inline uint32_t after_claim(uint32_t kind, bool earlier_accepted) { return earlier_accepted && accepted(kind) ? (uint32_t)HQ_FAIL_REPEAT : kind; }

HQ_FAIL_HD inline uint32_t kind_of(bool entry_found, uint32_t entry_class, bool entry_worker_match, bool override_found, bool override_worker_match, bool reporter_none,
                                   bool earlier_accepted) {
    return after_claim(kind_before_claim(entry_found, entry_class, entry_worker_match, override_found, override_worker_match, reporter_none), earlier_accepted);
}

}  // namespace hqfail
