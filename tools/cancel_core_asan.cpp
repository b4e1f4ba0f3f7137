// The grouping of a cancel batch (hyperqueue_amd/csrc/cancel_core.h) under AddressSanitizer + UBSan: a stand-alone program, every input and output array in a
// heap block of its exact size (group_on_host allocates its own scratch the same way).  Batches of 0 .. 4097 positions over 1 .. 70000 worker rows -- one, two
// and three radix digits -- with all positions unrouted, all on one row, every row once and random routes, each in the three thread orders, checked against a
// counting sort written here.
// Built and run by tests/test_cancel_core.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o cancel_core_asan tools/cancel_core_asan.cpp && ./cancel_core_asan
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../hyperqueue_amd/csrc/cancel_core.h"

using namespace hqcancel;

static long checks = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

// kind 0: no position routed, 1: all on one row, 2: position i on row i % W (every row once when n == W), 3: random, a third unrouted
static void one_case(uint32_t n, uint32_t W, int kind, int order) {
    std::unique_ptr<uint32_t[]> route(new uint32_t[n]), wid(new uint32_t[W]), out_wid(new uint32_t[W]), out_off(new uint32_t[(size_t)W + 1]);
    std::unique_ptr<uint64_t[]> id(new uint64_t[n]), out_id(new uint64_t[n]);
    for (uint32_t w = 0; w < W; w++) wid[w] = 50 + 3 * w;
    const uint32_t one = W ? (uint32_t)(rnd() % W) : 0;
    for (uint32_t i = 0; i < n; i++) {
        id[i] = rnd() >> 2;
        route[i] = kind == 0 ? NONE : kind == 1 ? one : kind == 2 ? i % W : (rnd() % 3 == 0 ? (rnd() & 1 ? NONE : W + (uint32_t)(rnd() % 5)) : (uint32_t)(rnd() % W));
    }
    uint32_t n_workers = ~0u, n_ids = ~0u;
    CHECK(group_on_host(n, W, route.get(), id.get(), wid.get(), order, &n_workers, &n_ids, out_wid.get(), out_off.get(), out_id.get()), "out of memory");
    // the expected lists: a counting sort, stable in the batch position
    std::vector<uint32_t> cnt(W, 0);
    for (uint32_t i = 0; i < n; i++) if (route[i] < W) cnt[route[i]]++;
    std::vector<uint32_t> e_wid, e_off{0}, first(W, 0);
    uint32_t tot = 0;
    for (uint32_t w = 0; w < W; w++) { first[w] = tot; if (cnt[w]) { e_wid.push_back(wid[w]); tot += cnt[w]; e_off.push_back(tot); } }
    std::vector<uint64_t> e_id(tot);
    for (uint32_t i = 0; i < n; i++) if (route[i] < W) e_id[first[route[i]]++] = id[i];
    CHECK(n_workers == e_wid.size() && n_ids == tot, "n=%u W=%u kind=%d order=%d: %u workers / %u ids, expected %zu / %u", n, W, kind, order, n_workers, n_ids, e_wid.size(), tot);
    for (uint32_t k = 0; k < n_workers; k++) CHECK(out_wid[k] == e_wid[k] && out_off[k] == e_off[k], "n=%u W=%u kind=%d order=%d: list %u", n, W, kind, order, k);
    CHECK(out_off[n_workers] == tot, "closing offset");
    for (uint32_t j = 0; j < tot; j++) CHECK(out_id[j] == e_id[j], "n=%u W=%u kind=%d order=%d: id %u", n, W, kind, order, j);
    cases++;
}

int main() {
    const uint32_t ns[] = {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097}, Ws[] = {1, 2, 255, 256, 257, 70000};
    for (uint32_t n : ns)
        for (uint32_t W : Ws)
            for (int kind = 0; kind < 4; kind++)
                for (int order = 0; order < 3; order++) {
                    if (kind != 3 && order != 0 && n > 300) continue;  // (the orders matter where positions collide: the random case runs all three everywhere)
                    one_case(n, W, kind, order);
                }
    one_case(70000, 70000, 2, 1);  // every row once, three digits, 69 tiles
    printf("cancel_core_asan: %ld cases, %ld checks, passes_of(255 / 256 / 65535 / 65536) = %u %u %u %u\n", cases, checks, passes_of(255), passes_of(256), passes_of(65535), passes_of(65536));
    return 0;
}
