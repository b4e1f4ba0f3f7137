// The remaining lifetime of a resident worker from its termination time and the clock (hqtick_cluster_set_clock): plain functions compiled for
// the device (k_clock_rows, kernels.hip) and for the host (hqcluster::WorkerSet's mirror, the debug hook of include/hqtick_debug.h, tools/clock_core_asan.cpp).
//
// The worker evaluation reads a remaining lifetime through one test per variant, `rem == INT64_MAX || (rem >= 0 && rem >= min_time[v])`, and the host groups
// workers by comparing it exactly.  So what a tick needs of `deadline - now` is which of the request table's min_time thresholds it still passes, and the value
// written is canonical for that: the largest threshold it passes.  Workers that differ only in deadlines between the same two thresholds get the same value.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HQC_HD __host__ __device__ inline
#else
#define HQC_HD inline
#endif

namespace hqclock {

constexpr int64_t NO_LIMIT = INT64_MAX;       // HQ_NO_TIME_LIMIT
constexpr int64_t FINITE_MAX = INT64_MAX - 1;  // the largest value a deadline or a remaining lifetime with a limit can take: saturation never makes it "no limit"
constexpr uint32_t CHUNK = 256;                // thresholds k_clock_rows stages in LDS at a time (one per thread of its workgroup)

// a + b and a - b, saturating into [INT64_MIN, FINITE_MAX]
HQC_HD int64_t sat_add(int64_t a, int64_t b) {
    int64_t r;
    if (__builtin_add_overflow(a, b, &r)) return b < 0 ? INT64_MIN : FINITE_MAX;
    return r < FINITE_MAX ? r : FINITE_MAX;
}
HQC_HD int64_t sat_sub(int64_t a, int64_t b) {
    int64_t r;
    if (__builtin_sub_overflow(a, b, &r)) return b > 0 ? INT64_MIN : FINITE_MAX;
    return r < FINITE_MAX ? r : FINITE_MAX;
}

// the termination time of a worker whose remaining lifetime at `now` is `remaining`
HQC_HD int64_t deadline_of(int64_t now, int64_t remaining) { return remaining == NO_LIMIT ? NO_LIMIT : sat_add(now, remaining); }
// ... and back: the true remaining lifetime (negative: the worker is past its termination time)
HQC_HD int64_t remaining_of(int64_t deadline, int64_t now) { return deadline == NO_LIMIT ? NO_LIMIT : sat_sub(deadline, now); }

// what the worker evaluation asks of a remaining lifetime (server/worker.rs:320-326)
HQC_HD bool time_ok(int64_t rem, uint64_t min_time) { return rem == NO_LIMIT || (rem >= 0 && (uint64_t)rem >= min_time); }

// One step of the canonical value of r >= 0: `best` folded over n more thresholds (the whole table on the host, one LDS chunk in the kernel).  Starts at 0.
HQC_HD uint64_t fold_thresholds(uint64_t best, int64_t r, const uint64_t *T, uint32_t n) {
    for (uint32_t v = 0; v < n; v++) { const uint64_t t = T[v]; if (t <= (uint64_t)r && t > best) best = t; }
    return best;
}

// The linear form: T[0..nv) as the request table has them, in any order, duplicates and all.
HQC_HD int64_t canonical_linear(int64_t deadline, int64_t now, const uint64_t *T, uint32_t nv) {
    if (deadline == NO_LIMIT) return NO_LIMIT;
    const int64_t r = sat_sub(deadline, now);
    if (r < 0) return -1;
    return (int64_t)fold_thresholds(0, r, T, nv);
}

// The sorted form: S[0..ns) ascending without duplicates (the host's copy, rebuilt when the request table changes); a binary search per worker.
HQC_HD int64_t canonical_sorted(int64_t deadline, int64_t now, const uint64_t *S, uint32_t ns) {
    if (deadline == NO_LIMIT) return NO_LIMIT;
    const int64_t r = sat_sub(deadline, now);
    if (r < 0) return -1;
    uint32_t lo = 0, hi = ns;  // the first S[i] > r
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (S[mid] <= (uint64_t)r) lo = mid + 1; else hi = mid; }
    return lo ? (int64_t)S[lo - 1] : 0;
}

}  // namespace hqclock
