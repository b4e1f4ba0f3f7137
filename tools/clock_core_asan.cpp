// The phase function of k_clock_rows (hyperqueue_amd/csrc/clock_core.h) under AddressSanitizer + UBSan: a stand-alone program over the edge cases and a random
// campaign, every array in an exact-size heap block.  It checks what the tick relies on: each threshold's time test answers for the canonical value as for the
// true remaining lifetime, the linear (chunked) fold equals the sorted search, and no step overflows.  Built and run by tests/test_cluster_clock.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o clock_core_asan tools/clock_core_asan.cpp && ./clock_core_asan [rounds]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../hyperqueue_amd/csrc/clock_core.h"

using namespace hqclock;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

static int64_t chunked(int64_t deadline, int64_t now, const uint64_t *T, uint32_t nv) {  // the kernel's walk over the table
    if (deadline == NO_LIMIT) return NO_LIMIT;
    const int64_t r = sat_sub(deadline, now);
    if (r < 0) return -1;
    uint64_t best = 0;
    for (uint32_t v0 = 0; v0 < nv; v0 += CHUNK) best = fold_thresholds(best, r, T + v0, std::min(CHUNK, nv - v0));
    return (int64_t)best;
}

static long checks = 0;
static void check_one(int64_t deadline, int64_t now, const std::vector<uint64_t> &table) {
    const uint32_t nv = (uint32_t)table.size();
    std::unique_ptr<uint64_t[]> T(new uint64_t[nv]);  // exact size: a read past the table is a report
    std::copy(table.begin(), table.end(), T.get());
    std::vector<uint64_t> sorted(table);
    std::sort(sorted.begin(), sorted.end()); sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    std::unique_ptr<uint64_t[]> S(new uint64_t[sorted.size()]);
    std::copy(sorted.begin(), sorted.end(), S.get());
    const int64_t lin = canonical_linear(deadline, now, T.get(), nv), ch = chunked(deadline, now, T.get(), nv), so = canonical_sorted(deadline, now, S.get(), (uint32_t)sorted.size());
    const int64_t truth = remaining_of(deadline, now);
    bool ok = lin == ch && lin == so;
    ok = ok && ((lin == NO_LIMIT) == (deadline == NO_LIMIT));
    for (uint32_t v = 0; v < nv; v++) ok = ok && time_ok(lin, T[v]) == time_ok(truth, T[v]);
    ok = ok && time_ok(lin, 0) == time_ok(truth, 0);
    if (!ok) { fprintf(stderr, "mismatch: deadline %lld now %lld nv %u -> linear %lld chunked %lld sorted %lld true %lld\n", (long long)deadline, (long long)now, nv, (long long)lin, (long long)ch, (long long)so, (long long)truth); exit(1); }
    checks++;
}

int main(int argc, char **argv) {
    const long rounds = argc > 1 ? atol(argv[1]) : 2000;
    const int64_t edge_t[] = {INT64_MIN, INT64_MIN + 1, -1000000000000ll, -1, 0, 1, 9999999999ll, 10000000000ll, 10000000001ll, INT64_MAX - 2, INT64_MAX - 1, INT64_MAX};
    const std::vector<std::vector<uint64_t>> tables = {
        {}, {0}, {0, 0, 0}, {10000000000ull}, {0, 10000000000ull, 100000000000ull}, {100000000000ull, 10000000000ull, 10000000000ull, 0}, {1ull << 63}, {0, UINT64_MAX, (1ull << 63) - 1, (1ull << 63) - 2},
        {5, 5, 7, 7, 7, 1}};
    for (const auto &t : tables) for (int64_t d : edge_t) for (int64_t n : edge_t) check_one(d, n, t);
    // r == T[v] and r == T[v] - 1, both ends of the range for now + remaining
    for (const auto &t : tables) for (uint64_t thr : t) if (thr <= (uint64_t)FINITE_MAX) for (int64_t now : {(int64_t)0, (int64_t)-7, (int64_t)123456789}) {
        check_one(sat_add(now, (int64_t)thr), now, t);
        if (thr) check_one(sat_add(now, (int64_t)thr - 1), now, t);
    }
    for (int64_t now : edge_t) for (int64_t rem : edge_t) {
        const int64_t d = deadline_of(now, rem);
        if ((d == NO_LIMIT) != (rem == NO_LIMIT)) { fprintf(stderr, "deadline_of(%lld, %lld) = %lld\n", (long long)now, (long long)rem, (long long)d); return 1; }
        checks++;
    }
    for (long i = 0; i < rounds; i++) {  // random tables, some longer than one chunk
        const uint32_t nv = (uint32_t)(rnd() % (i % 50 == 0 ? 3 * CHUNK : 12));
        std::vector<uint64_t> t(nv);
        for (auto &x : t) { const uint64_t k = rnd() % 8; x = k == 0 ? 0 : k == 1 ? rnd() : (rnd() % 200) * 1000000000ull; }
        for (int j = 0; j < 16; j++) {
            const int64_t now = (int64_t)(rnd() % 400000000000ull) - 100000000000ll;
            const uint64_t k = rnd() % 10;
            const int64_t d = k == 0 ? NO_LIMIT : k == 1 ? (int64_t)rnd() : now + (int64_t)(rnd() % 300000000000ull) - 50000000000ll;
            check_one(d, now, t);
        }
    }
    printf("clock_core_asan: %ld checks ok\n", checks);
    return 0;
}
