// The pure host pieces of phase A (hyperqueue_amd/csrc/scan_core.h) under AddressSanitizer + UBSan: a stand-alone program, every table in an exact-size heap
// block.  These are the parts of the scan that decide buffer sizes and trust device output: the runs of a dense histogram, the decode of the ordered view's run
// table (with every refusal and its code), the choice of radix passes from the digit histogram, the wave geometry.  Built and run by tests/test_scan_core.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o scan_core_asan tools/scan_core_asan.cpp && ./scan_core_asan
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../hyperqueue_amd/csrc/scan_core.h"

using namespace hqscan;

static long checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

// ---- runs of a histogram against a brute-force count
static void check_runs(uint32_t L, uint32_t Q, uint32_t fill_percent) {
    Table sc; sc.L = L; sc.Q = Q; sc.G = L * Q;
    sc.levels.resize(L); for (uint32_t l = 0; l < L; l++) sc.levels[l] = 1000000 - 7 * l;
    sc.hist.assign((size_t)L * Q, 0); sc.hist.shrink_to_fit();
    for (auto &c : sc.hist) if (rnd() % 100 < fill_percent) c = 1 + (uint32_t)(rnd() % 50);
    runs_from_hist(sc);
    CHECK(!sc.ordered && sc.run_off.size() == (size_t)Q + 1 && sc.run_off[0] == 0, "L %u Q %u", L, Q);
    size_t nonzero = 0; for (uint32_t c : sc.hist) nonzero += c != 0;
    CHECK(sc.run_cnt.size() == nonzero && sc.run_group.size() == nonzero && sc.run_level.size() == nonzero && sc.run_prio.size() == nonzero && sc.run_start.empty(), "L %u Q %u", L, Q);
    CHECK(sc.run_off[Q] == nonzero, "L %u Q %u", L, Q);
    for (uint32_t q = 0; q < Q; q++) {
        uint32_t r = sc.run_off[q];
        for (uint32_t l = 0; l < L; l++) {  // brute force: the nonempty levels of q in table order
            const uint32_t c = sc.hist[(size_t)l * Q + q];
            if (!c) continue;
            CHECK(r < sc.run_off[q + 1] && sc.run_cnt[r] == c && sc.run_group[r] == l * Q + q && sc.run_level[r] == l && sc.run_prio[r] == sc.levels[l], "L %u Q %u q %u l %u", L, Q, q, l);
            r++;
        }
        CHECK(r == sc.run_off[q + 1], "L %u Q %u q %u", L, Q, q);
    }
}

// ---- the view's run table: hand-made tables in a block of exactly order_tab_layout(n).bytes
struct RunTab { uint32_t n, nr, nl; std::vector<uint32_t> rq, start, rank; std::vector<uint64_t> prio; };
static std::unique_ptr<uint8_t[]> encode(const RunTab &t) {
    const OrderTabLayout tl = order_tab_layout(t.n);
    std::unique_ptr<uint8_t[]> b(new uint8_t[tl.bytes]);
    memset(b.get(), 0xEE, tl.bytes);  // (what the kernel did not write is garbage)
    uint32_t head[2] = {t.nr, t.nl};
    memcpy(b.get(), head, 8);
    auto put = [&](size_t off, const void *src, size_t bytes) { if (bytes) memcpy(b.get() + off, src, bytes); };  // (an empty vector's data() may be null)
    put(tl.o_rq, t.rq.data(), t.rq.size() * 4); put(tl.o_st, t.start.data(), t.start.size() * 4); put(tl.o_rk, t.rank.data(), t.rank.size() * 4); put(tl.o_pr, t.prio.data(), t.prio.size() * 8);
    return b;
}
static void check_accepted(const RunTab &t, uint32_t Q) {
    const std::unique_ptr<uint8_t[]> b = encode(t);
    Table sc; const char *why = nullptr;
    const int rc = decode_runs(b.get(), t.n, Q, &sc, &why);
    CHECK(rc == 0 && why == nullptr, "n %u nr %u: %d %s", t.n, t.nr, rc, why ? why : "");
    CHECK(sc.L == t.nl && sc.G == t.nr && sc.run_cnt.size() == t.nr && sc.run_off.size() == (size_t)Q + 1, "n %u nr %u", t.n, t.nr);
    uint64_t total = 0;
    for (uint32_t r = 0; r < t.nr; r++) {
        CHECK(sc.run_start[r] == t.start[r] && sc.run_level[r] == t.rank[r] && sc.run_prio[r] == t.prio[r] && sc.run_group[r] == r, "run %u", r);
        CHECK(sc.run_cnt[r] == (r + 1 < t.nr ? t.start[r + 1] : t.n) - t.start[r], "run %u", r);
        total += sc.run_cnt[r];
    }
    CHECK(total == t.n - t.start[0], "n %u", t.n);
    for (uint32_t q = 0; q < Q; q++) {  // the prefix sum: the runs of q are those whose request id is q, in table order
        uint32_t first = t.nr, cnt = 0;
        for (uint32_t r = 0; r < t.nr; r++) if (t.rq[r] == q) { if (first == t.nr) first = r; cnt++; }
        CHECK(sc.run_off[q + 1] - sc.run_off[q] == cnt && (cnt == 0 || sc.run_off[q] == first), "q %u", q);
    }
}
static void check_refused(const RunTab &t, uint32_t Q, const char *text) {
    const std::unique_ptr<uint8_t[]> b = encode(t);
    Table sc; const char *why = nullptr;
    const int rc = decode_runs(b.get(), t.n, Q, &sc, &why);
    CHECK(rc == HQTICK_E_DEVICE && why && std::string(why) == text, "n %u nr %u nl %u: %d %s", t.n, t.nr, t.nl, rc, why ? why : "(null)");
}

// ---- the pass choice: a digit histogram of n slots in which the digits listed in `varying` take two values and every other digit one
static std::unique_ptr<uint32_t[]> digit_hist(uint32_t n_digits, uint32_t n, const std::vector<uint32_t> &varying) {
    std::unique_ptr<uint32_t[]> gh(new uint32_t[(size_t)n_digits * 256]);
    memset(gh.get(), 0, (size_t)n_digits * 256 * 4);
    for (uint32_t dg = 0; dg < n_digits; dg++) {
        bool v = false; for (uint32_t x : varying) v = v || x == dg;
        if (v) { gh[dg * 256 + 3] = n / 2; gh[dg * 256 + 200] = n - n / 2; } else gh[dg * 256 + (dg * 37) % 256] = n;
    }
    return gh;
}
static void check_passes(const std::vector<uint32_t> &varying, const std::vector<uint32_t> &want, uint32_t want_level_after) {
    const uint32_t D = 12, n = 1001;
    const std::unique_ptr<uint32_t[]> gh = digit_hist(D, n, varying);
    const Passes p = order_passes(gh.get(), D, n);
    CHECK(p.n == want.size() && p.level_after == want_level_after, "passes %u level_after %u", p.n, p.level_after);
    uint32_t mask = 0;
    for (uint32_t i = 0; i < p.n; i++) { CHECK(p.digit[i] == want[i], "pass %u on digit %u", i, p.digit[i]); mask |= 1u << want[i]; }
    CHECK(p.mask() == mask, "mask %x", p.mask());
}

// ---- the geometry
static void check_geometry(uint64_t N, uint32_t G, uint32_t tpw_hint) {
    const Geom g = wave_geometry(N, G, tpw_hint, 2048);
    CHECK((uint64_t)g.n_waves * g.tasks_per_wave >= N && (uint64_t)(g.n_waves - 1) * g.tasks_per_wave < N, "N %llu G %u: %u x %u", (unsigned long long)N, G, g.n_waves, g.tasks_per_wave);
    CHECK(g.tab_stride % 16 == 0 && g.tab_stride >= g.n_waves && g.tab_stride < g.n_waves + 16, "N %llu G %u: stride %u", (unsigned long long)N, G, g.tab_stride);
    const uint32_t start = tpw_hint ? tpw_hint : 256, times = g.tasks_per_wave / start;
    CHECK(g.tasks_per_wave % start == 0 && times >= 1 && (times & (times - 1)) == 0, "N %llu G %u: %u per wave, doubled from %u", (unsigned long long)N, G, g.tasks_per_wave, start);
    CHECK((uint64_t)g.n_waves * G <= (1ull << 24), "N %llu G %u: %llu slices x groups", (unsigned long long)N, G, (unsigned long long)g.n_waves * G);  // the per-slice table under 64 MiB
    if (!tpw_hint) CHECK(g.n_waves <= 32768, "N %llu: %u rows", (unsigned long long)N, g.n_waves);
    CHECK(g.waves_per_block == (G <= 2048 ? 4u : 1u), "G %u: %u waves per block", G, g.waves_per_block);
}

int main() {
    // runs
    for (uint32_t L : {0u, 1u, 2u, 5u, 64u}) for (uint32_t Q : {0u, 1u, 3u, 16u, 100u}) for (uint32_t fill : {0u, 30u, 100u}) check_runs(L, Q, fill);
    for (int i = 0; i < 200; i++) check_runs(1 + (uint32_t)(rnd() % 40), 1 + (uint32_t)(rnd() % 40), (uint32_t)(rnd() % 101));

    // decode, accepted
    check_accepted({10, 1, 1, {2}, {0}, {0}, {77}}, 4);                                                            // one run
    check_accepted({4, 4, 4, {0, 0, 1, 3}, {0, 1, 2, 3}, {0, 1, 2, 3}, {9, 8, 7, 6}}, 4);                          // nr == n: every slot a run of its own
    check_accepted({9, 4, 2, {0, 0, 2, 2}, {0, 3, 5, 6}, {0, 1, 0, 1}, {50, 40, 50, 40}}, 3);                      // a request without a run in the middle
    check_accepted({1, 1, 1, {0}, {0}, {0}, {0}}, 1);
    for (int i = 0; i < 200; i++) {  // random well-formed tables
        const uint32_t Q = 1 + (uint32_t)(rnd() % 9), nr = 1 + (uint32_t)(rnd() % 30);
        RunTab t; t.nr = nr; t.nl = 1 + (uint32_t)(rnd() % nr);
        uint32_t q = 0, pos = 0;
        for (uint32_t r = 0; r < nr; r++) {
            if (rnd() % 3 == 0 && q + 1 < Q) q += 1 + (uint32_t)(rnd() % (Q - 1 - q));
            t.rq.push_back(q); t.start.push_back(pos); t.rank.push_back((uint32_t)(rnd() % t.nl)); t.prio.push_back(rnd());
            pos += 1 + (uint32_t)(rnd() % 5);
        }
        t.n = pos;
        check_accepted(t, Q);
    }
    // decode, refused: each refusal and its code
    const char *INCONSISTENT = "ordered view: inconsistent run table", *ORDER = "ordered view: runs out of request order";
    check_refused({5, 0, 0, {}, {}, {}, {}}, 4, INCONSISTENT);                                                    // nr == 0
    check_refused({5, 0, 1, {}, {}, {}, {}}, 4, INCONSISTENT);
    check_refused({3, 4, 1, {0, 0, 0}, {0, 1, 2}, {0, 0, 0}, {1, 1, 1}}, 4, INCONSISTENT);                        // nr > n: the table holds n entries, none is read
    check_refused({3, 0xFFFFFFFFu, 1, {0, 0, 0}, {0, 1, 2}, {0, 0, 0}, {1, 1, 1}}, 4, INCONSISTENT);
    check_refused({3, 2, 3, {0, 1}, {0, 1}, {0, 1}, {5, 4}}, 4, INCONSISTENT);                                    // nl > nr
    check_refused({3, 2, 0, {0, 1}, {0, 1}, {0, 0}, {5, 4}}, 4, INCONSISTENT);                                    // nl == 0
    check_refused({3, 2, 2, {0, 4}, {0, 1}, {0, 1}, {5, 4}}, 4, ORDER);                                           // a request id >= Q
    check_refused({3, 1, 1, {0xFFFFFFFFu}, {0}, {0}, {5}}, 4, ORDER);
    check_refused({3, 3, 2, {1, 2, 1}, {0, 1, 2}, {0, 1, 1}, {5, 4, 4}}, 4, ORDER);                               // descending request ids
    check_refused({3, 1, 1, {0}, {0}, {0}, {5}}, 0, ORDER);                                                       // no request at all

    // pass choice
    check_passes({}, {0}, 0);                          // all digits constant: one pass still drops the tombstones
    check_passes({8, 9, 11}, {8, 9, 11}, 0);           // only rq digits vary: no priority pass, level ranks after the first pass (one priority, any order)
    check_passes({0, 5, 7}, {0, 5, 7}, 2);             // only priority digits vary: the ranks are read after the last pass
    check_passes({7, 8}, {7, 8}, 0);                   // digits 7 and 8: the ranks after the pass on 7, in front of the pass on rq
    check_passes({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 7);
    {   // a digit whose one value holds all n slots but one is NOT constant
        const uint32_t D = 12, n = 500;
        std::unique_ptr<uint32_t[]> gh = digit_hist(D, n, {});
        gh[4 * 256 + (4 * 37) % 256] = n - 1; gh[4 * 256 + 255] = 1;
        const Passes p = order_passes(gh.get(), D, n);
        CHECK(p.n == 1 && p.digit[0] == 4 && p.level_after == 0, "passes %u digit %u", p.n, p.digit[0]);
    }

    // geometry
    const uint64_t Ns[] = {1, 255, 256, 257, 32768ull * 256, 32768ull * 256 + 1};
    for (uint64_t N : Ns) for (uint32_t G : {1u, 8u, 64u, 2048u, 2049u, 16384u}) for (uint32_t hint : {0u, 256u, 1024u}) check_geometry(N, G, hint);
    CHECK(wave_geometry(256, 8, 0, 2048).n_waves == 1 && wave_geometry(257, 8, 0, 2048).n_waves == 2, "slices of 256");
    CHECK(wave_geometry(32768ull * 256, 1, 0, 2048).tasks_per_wave == 256 && wave_geometry(32768ull * 256 + 1, 1, 0, 2048).tasks_per_wave == 512, "the 32768-row rule");
    // N x G across 2^24 slices x groups: 4096 slices of 256 x 4096 groups is the cap exactly, one slot more doubles the slice — with a hint too, which lifts only the row rule
    CHECK(wave_geometry(4096ull * 256, 4096, 0, 2048).tasks_per_wave == 256 && wave_geometry(4096ull * 256 + 1, 4096, 0, 2048).tasks_per_wave == 512, "the 2^24 rule");
    CHECK(wave_geometry(4096ull * 256, 4096, 256, 2048).tasks_per_wave == 256 && wave_geometry(4096ull * 256 + 1, 4096, 256, 2048).tasks_per_wave == 512, "the 2^24 rule with a hint");
    CHECK(wave_geometry(40000ull * 256, 1, 256, 2048).n_waves == 40000, "a hint lifts the row rule");
    for (uint64_t N : {4096ull * 256, 4096ull * 256 + 1, 1ull << 26, (1ull << 32) - 16}) for (uint32_t G : {4096u, 16384u}) for (uint32_t hint : {0u, 256u, 2048u}) check_geometry(N, G, hint);

    printf("%ld checks ok\n", checks);
    return 0;
}
