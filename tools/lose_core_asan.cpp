// The host functions of hqtick_lose_workers (hyperqueue_amd/csrc/lose_core.h) under AddressSanitizer + UBSan: a stand-alone program, every input and output
// array in a heap block of its exact size (group_on_host allocates its own scratch the same way).  The rule over its whole input table; the grouping for 0 .. 1030
// evicted entries over 1 .. 300 lost workers -- one and two radix digits of the sort -- with all entries on one worker, dealt round-robin and random, each in the
// three thread orders, checked against a counting sort written here; the two layouts: no column overlaps another or leaves its buffer.
// Built and run by tests/test_lose_oracle.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o lose_core_asan tools/lose_core_asan.cpp && ./lose_core_asan
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../hyperqueue_amd/csrc/lose_core.h"

using namespace hqlose;

static long checks = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

// how 0: every entry on one worker, 1: entry j on worker j % n, 2: random
static void one_case(uint32_t k, uint32_t n, int how, int order) {
    std::unique_ptr<uint64_t[]> id(new uint64_t[k]), prio(new uint64_t[k]), o_id(new uint64_t[k]), o_prio(new uint64_t[k]);
    std::unique_ptr<uint32_t[]> rq(new uint32_t[k]), widx(new uint32_t[k]), o_rq(new uint32_t[k]), off(new uint32_t[(size_t)n + 1]);
    std::unique_ptr<uint8_t[]> kind(new uint8_t[k]), o_kind(new uint8_t[k]);
    const uint32_t one = (uint32_t)(rnd() % n);
    uint64_t next = 0;
    for (uint32_t j = 0; j < k; j++) {
        next += 1 + rnd() % 9; id[j] = next; prio[j] = rnd(); rq[j] = (uint32_t)rnd(); kind[j] = (uint8_t)(rnd() % 5);
        widx[j] = how == 0 ? one : how == 1 ? j % n : (uint32_t)(rnd() % n);
    }
    CHECK(group_on_host(k, n, id.get(), prio.get(), rq.get(), kind.get(), widx.get(), order, off.get(), o_id.get(), o_prio.get(), o_rq.get(), o_kind.get()), "out of memory");
    std::vector<uint32_t> cnt(n, 0), at((size_t)n + 1, 0);
    for (uint32_t j = 0; j < k; j++) cnt[widx[j]]++;
    for (uint32_t w = 0; w < n; w++) at[w + 1] = at[w] + cnt[w];
    for (uint32_t w = 0; w <= n; w++) CHECK(off[w] == at[w], "k=%u n=%u how=%d order=%d: offset %u is %u, not %u", k, n, how, order, w, off[w], at[w]);
    std::vector<uint32_t> fill(at.begin(), at.end() - 1);
    std::vector<uint32_t> src(k);
    for (uint32_t j = 0; j < k; j++) src[fill[widx[j]]++] = j;  // stable: ids ascend inside a worker
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t p = src[j];
        CHECK(o_id[j] == id[p] && o_prio[j] == prio[p] && o_rq[j] == rq[p] && o_kind[j] == kind[p], "k=%u n=%u how=%d order=%d: element %u", k, n, how, order, j);
    }
    cases++;
}

static void layouts(size_t cap, size_t sort_cap, uint32_t n) {
    const DevLayout D = dev_layout(cap, sort_cap, n);
    const size_t sc = hqcancel::scratch_of((uint32_t)cap, n).total * 4;
    std::vector<std::pair<size_t, size_t>> d = {{D.skey, sort_cap * 8}, {D.id, cap * 8}, {D.prio, cap * 8}, {D.sval, sort_cap * 4}, {D.rq, cap * 4}, {D.widx, cap * 4}, {D.lost, (size_t)n * 4},
                                                {D.lost_idx, (size_t)n * 4}, {D.call, (size_t)n * 4}, {D.scratch, sc}, {D.kind, cap}};
    const PinLayout P = pin_layout(cap, n);
    std::vector<std::pair<size_t, size_t>> p = {{P.in, (size_t)n * 12}, {P.f_id, cap * 8}, {P.f_prio, cap * 8}, {P.c_id, cap * 8}, {P.c_prio, cap * 8}, {P.m_task, (size_t)n * 8}, {P.f_rq, cap * 4},
                                                {P.c_rq, cap * 4}, {P.off, ((size_t)n + 1) * 4}, {P.m_root, (size_t)n * 4}, {P.c_kind, cap}};
    const size_t align_d[] = {8, 8, 8, 4, 4, 4, 4, 4, 4, 8, 1}, align_p[] = {4, 8, 8, 8, 8, 8, 4, 4, 4, 4, 1};
    for (int which = 0; which < 2; which++) {
        auto &cols = which ? p : d;
        const size_t bytes = which ? P.bytes : D.bytes;
        for (size_t i = 0; i < cols.size(); i++) {
            CHECK(cols[i].first % (which ? align_p[i] : align_d[i]) == 0, "cap=%zu n=%u: column %zu of layout %d is misaligned", cap, n, i, which);
            CHECK(cols[i].first + cols[i].second <= bytes, "cap=%zu n=%u: column %zu of layout %d leaves the buffer", cap, n, i, which);
            for (size_t j = 0; j < i; j++)
                CHECK(cols[j].first + cols[j].second <= cols[i].first || cols[i].first + cols[i].second <= cols[j].first || !cols[i].second || !cols[j].second,
                      "cap=%zu n=%u: columns %zu and %zu of layout %d overlap", cap, n, j, i, which);
        }
    }
    cases++;
}

int main() {
    for (uint32_t cls = 0; cls < 3; cls++)
        for (int run = 0; run < 2; run++)
            for (int red = 0; red < 2; red++) {
                const uint32_t k = settle(kind_of_entry(cls, run != 0), red != 0);
                const uint32_t want = cls == E_MN ? HQ_LOSE_MN_ROOT : cls == E_PF ? HQ_LOSE_PREFILLED : red ? HQ_LOSE_REDIRECT : run ? HQ_LOSE_RUNNING : HQ_LOSE_ASSIGNED;
                CHECK(k == want, "class %u run %d redirect %d: kind %u, not %u", cls, run, red, k, want);
                CHECK(is_running(k) == (k == HQ_LOSE_RUNNING || k == HQ_LOSE_MN_ROOT), "kind %u", k);
            }
    const uint32_t ks[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1030}, ns[] = {1, 2, 5, 64, 255, 256, 257, 300};
    for (uint32_t k : ks)
        for (uint32_t n : ns)
            for (int how = 0; how < 3; how++)
                for (int order = 0; order < 3; order++) one_case(k, n, how, order);
    auto pow2 = [](size_t x) { size_t p = 2; while (p < x) p <<= 1; return p; };
    for (size_t cap : {(size_t)1, (size_t)2, (size_t)3, (size_t)1023, (size_t)1024, (size_t)1025, (size_t)100001})
        for (uint32_t n : {1u, 2u, 3u, 64u, 1000u}) layouts(cap, pow2(cap), n);
    printf("lose_core_asan: %ld cases, %ld checks\n", cases, checks);
    return 0;
}
