// The device side of a cancel batch's grouping (cancel_core.h): the launches of hqtick_cancel_tasks behind the ledger's passes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cancel_core.h"

namespace hqcancel {

// What a grouping reads and writes.  route / kind / id / wid: device memory.  scratch: scratch_of(n, W).total u32 of device memory, its start[W] part NONE on
// entry.  The out_* arrays, hdr and the route_* arrays: pinned host memory as the device sees it (FinArgs says how long each is).
struct Group {
    uint32_t n, W;
    const uint32_t *route; const uint8_t *kind; const uint64_t *id; const uint32_t *wid;
    uint32_t *scratch;
    uint64_t *out_id; uint32_t *out_wid, *out_off, *hdr, *route_wid; uint8_t *route_kind;
    uint32_t no_worker;
};
// 3 launches per radix digit of W, then 2: everything is enqueued on s, nothing is waited for
hipError_t group(const Group &g, hipStream_t s);
// The stable sort of a grouping alone, for any key below W (hqtick_fail_tasks groups a closure's ascending ids by the batch position that owns them, W = the batch
// size: graph.hip).  route [n]: the keys, anything not below W counts as W and ends up last; scratch: scratch_of(n, W).total u32 (its start[W] part is not touched).
// *key / *pos: where in scratch the sorted keys and the positions 0 .. n - 1 in sorted order are.  3 launches per radix digit of W, nothing is waited for.
hipError_t sort_rows(uint32_t n, uint32_t W, const uint32_t *route, uint32_t *scratch, const uint32_t **key, const uint32_t **pos, hipStream_t s);

}  // namespace hqcancel
