// The placement's solvers without HIP (hyperqueue_amd/csrc/solve_core.h) under AddressSanitizer + UBSan: a stand-alone program.
//   layout     a few hundred random small launches (1-8 columns, 1-4 resources, 0-3 entries per column, 0-9 classes): every offset on 8 bytes, the class tables on 16,
//              the regions in order and exactly as long as their tables, the sizes equal to the closed form; the image packed into an exact-size heap block and read
//              back through the views
//   emulation  EmulatedBlocks (even classes on the packed column table, odd ones on the caller's tables) and solve_block on the whole packed image give the x, status
//              and steps of solve_block on the caller's tables read in place
//   deal       ShardedBlocks over EmulatedBlocks on 1, 2, 3 and 5 ranks — threads over an in-process all-gather — against the unsharded answer, byte for byte; the
//              pass below min_classes; one rank's failed solver; a failed all-gather; the share arithmetic
//   the three small derivations around a solve on hand-written counts
// Built and run by tests/test_solve_core.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -o solve_core_asan tools/solve_core_asan.cpp && ./solve_core_asan
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../hyperqueue_amd/csrc/solve_core.h"

using namespace hqsolve;

static long checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
template <class T> static std::unique_ptr<T[]> exact(const std::vector<T> &v) {  // a heap block of exactly the vector's bytes (never null: one element for an empty table)
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}
static size_t al8(size_t v) { return (v + 7) & ~(size_t)7; }

// One launch's tables, each in a heap block of its own: a block of the random family of tests/test_block_solve.py at the issue's sizes.
struct Launch {
    uint32_t NC = 0, R = 0, ne = 0, nd = 0;
    std::vector<uint32_t> ent_off, ent_res, weight; std::vector<uint8_t> ent_kind; std::vector<uint64_t> ent_amount, free_, total, elig; std::vector<double> pool;
    std::unique_ptr<uint32_t[]> p_off, p_res, p_w; std::unique_ptr<uint8_t[]> p_kind; std::unique_ptr<uint64_t[]> p_amt, p_free, p_tot, p_elig; std::unique_ptr<double[]> p_pool;
    hqblock::ColTable ct{}; hqblock::ClassTable cl{};
    Launch(uint32_t n_cols, uint32_t n_res, uint32_t n_classes, bool allow_empty_cols) : NC(n_cols), R(n_res), nd(n_classes) {
        static const uint64_t grid[] = {10000, 20000, 40000, 5000, 2500, 80000, 30000, 15000, 70000};
        ent_off.push_back(0);
        for (uint32_t g = 0; g < NC; g++) {
            uint32_t want = allow_empty_cols ? below(4) : 1 + below(3), first = below(R);
            if (want > R) want = R;
            for (uint32_t k = 0; k < want; k++) { ent_res.push_back((first + k) % R); ent_kind.push_back(below(16) == 0 ? 1 : 0); ent_amount.push_back(grid[below(9)]); }
            ent_off.push_back((uint32_t)ent_res.size());
            weight.push_back(below(3) ? 10000 : 1000 + below(30000));
        }
        ne = (uint32_t)ent_res.size();
        for (uint32_t r = 0; r < R; r++) pool.push_back((1 + below(49999)) / 7.0);
        for (uint32_t c = 0; c < nd; c++) {
            for (uint32_t r = 0; r < R; r++) { const uint64_t t = (uint64_t)(1 + below(64)) * 10000; total.push_back(t); free_.push_back(below(5) == 0 ? t : (uint64_t)below((uint32_t)(t / 100) + 1) * 100); }
            uint64_t m = (1ull << NC) - 1;
            if (below(4) == 0) m &= rnd();
            elig.push_back(m);
        }
        p_off = exact(ent_off); p_res = exact(ent_res); p_w = exact(weight); p_kind = exact(ent_kind); p_amt = exact(ent_amount); p_pool = exact(pool);
        p_free = exact(free_); p_tot = exact(total); p_elig = exact(elig);
        ct = hqblock::ColTable{NC, R, p_off.get(), p_res.get(), p_kind.get(), p_amt.get(), p_w.get(), p_pool.get(), nullptr, 0};
        cl = hqblock::ClassTable{nd, p_free.get(), p_tot.get(), p_elig.get()};
    }
};

struct Answer {
    std::vector<uint32_t> x, status, steps;
    Answer(uint32_t nd, uint32_t NC) : x((size_t)nd * NC + 1, 0xABABABABu), status(nd + 1, 0xABABABABu), steps(nd + 1, 0xABABABABu) {}  // (one spare word each: never null)
    hqblock::Output out() { return hqblock::Output{x.data(), status.data(), steps.data(), nullptr}; }
    bool operator==(const Answer &o) const { return x == o.x && status == o.status && steps == o.steps; }
};

static void in_place(const Launch &t, Answer &a, uint32_t budget) {
    static hqblock::Shared *S = new hqblock::Shared();
    hqblock::HostWave wv;
    for (uint32_t c = 0; c < t.nd; c++) hqblock::solve_block(wv, *S, t.ct, t.cl, c, a.out(), budget);
}

// ---------------------------------------------------------------------------------------------- layout and emulation
static void check_layout_and_emulation() {
    for (int it = 0; it < 400; it++) {
        Launch t(1 + below(8), 1 + below(4), below(10), true);
        const size_t NC = t.NC, R = t.R, ne = t.ne, nd = t.nd;
        const BlockLayout L = block_layout(t.NC, t.R, t.ne, t.nd);
        // the closed form
        const size_t o_res = al8((NC + 1) * 4), o_w = al8(o_res + ne * 4), o_kind = al8(o_w + NC * 4), o_amt = al8(o_kind + ne), o_pool = o_amt + ne * 8,
                     o_free = (o_pool + R * 8 + 15) & ~(size_t)15, o_tot = o_free + nd * R * 8, o_elig = o_tot + nd * R * 8, o_x = o_elig + nd * 8, o_st = o_x + al8(nd * NC * 4),
                     o_steps = o_st + al8(nd * 4), end = o_steps + al8(nd * 4);
        CHECK(L.o_off == 0 && L.o_res == o_res && L.o_w == o_w && L.o_kind == o_kind && L.o_amt == o_amt && L.o_pool == o_pool, "column table offsets");
        CHECK(L.o_free == o_free && L.o_tot == o_tot && L.o_elig == o_elig && L.o_x == o_x && L.o_st == o_st && L.o_steps == o_steps && L.end == end, "class table and output offsets");
        CHECK(L.pinned_bytes() == end + 64 && L.device_bytes() == o_x + 64, "buffer sizes");
        // alignment, order, room
        const size_t offs[] = {L.o_off, L.o_res, L.o_w, L.o_kind, L.o_amt, L.o_pool, L.o_free, L.o_tot, L.o_elig, L.o_x, L.o_st, L.o_steps, L.end};
        const size_t lens[] = {(NC + 1) * 4, ne * 4, NC * 4, ne, ne * 8, R * 8, nd * R * 8, nd * R * 8, nd * 8, nd * NC * 4, nd * 4, nd * 4};
        for (int k = 0; k < 13; k++) CHECK(offs[k] % 8 == 0, "offset %d = %zu", k, offs[k]);
        CHECK(L.o_free % 16 == 0, "class tables at %zu", L.o_free);
        for (int k = 0; k < 12; k++) CHECK(offs[k] + lens[k] <= offs[k + 1], "region %d [%zu, +%zu) reaches into the next at %zu", k, offs[k], lens[k], offs[k + 1]);
        CHECK(L.o_free <= hqblock::BLOB_MAX, "column table of %zu bytes", L.o_free);
        // the column table alone, as the emulation stages it: exactly o_free bytes
        {
            const BlockLayout L0 = block_layout(t.NC, t.R, t.ne, 0);
            CHECK(L0.o_free == L.o_free && L0.end == L0.o_free, "layout without classes");
            std::unique_ptr<hqblock::V16[]> blob(new hqblock::V16[L0.o_free / 16]);
            pack_cols(reinterpret_cast<unsigned char *>(blob.get()), t.ct, L0);
        }
        // the whole image in a block of exactly `end` bytes, read back through the views
        std::unique_ptr<hqblock::V16[]> image(new hqblock::V16[(L.end + 15) / 16]);  // (end is a multiple of 8: at most 8 spare bytes, behind the outputs)
        unsigned char *b = reinterpret_cast<unsigned char *>(image.get());
        memset(b, 0xEE, L.end);
        pack_cols(b, t.ct, L); pack_classes(b, t.cl, t.R, L);
        const hqblock::ColTable vt = cols_view(b, t.NC, t.R, L); const hqblock::ClassTable vc = classes_view(b, t.nd, L);
        CHECK(vt.n_cols == t.NC && vt.R == t.R && vt.blob == b && vt.blob_bytes == L.o_free && vc.n_classes == t.nd, "views");
        CHECK(memcmp(vt.ent_off, t.ent_off.data(), (NC + 1) * 4) == 0 && memcmp(vt.weight, t.weight.data(), NC * 4) == 0 && memcmp(vt.pool, t.pool.data(), R * 8) == 0, "ent_off / weight / pool read back");
        if (ne) CHECK(memcmp(vt.ent_res, t.ent_res.data(), ne * 4) == 0 && memcmp(vt.ent_kind, t.ent_kind.data(), ne) == 0 && memcmp(vt.ent_amount, t.ent_amount.data(), ne * 8) == 0, "entries read back");
        if (nd) CHECK(memcmp(vc.free_, t.free_.data(), nd * R * 8) == 0 && memcmp(vc.total, t.total.data(), nd * R * 8) == 0 && memcmp(vc.elig, t.elig.data(), nd * 8) == 0, "class tables read back");
        for (size_t i = L.o_x; i < L.end; i++) CHECK(b[i] == 0xEE, "the packers wrote into the outputs at %zu", i);
        // the emulation: packed and in place alike
        if (!nd) continue;
        const uint32_t budget = it % 7 == 0 ? 3 : 4096;
        Answer want(t.nd, t.NC), emu(t.nd, t.NC), img(t.nd, t.NC);
        in_place(t, want, budget);
        EmulatedBlocks e(budget);
        CHECK(e.solve(t.ct, t.cl, emu.out()), "EmulatedBlocks::solve");
        CHECK(emu == want, "EmulatedBlocks differs from solve_block in place (launch %d)", it);
        {
            static hqblock::Shared *S = new hqblock::Shared();
            hqblock::HostWave wv;
            for (uint32_t c = 0; c < t.nd; c++) hqblock::solve_block(wv, *S, vt, vc, c, img.out(), budget);
        }
        CHECK(img == want, "solve_block on the packed image differs (launch %d)", it);
    }
}

// ---------------------------------------------------------------------------------------------- the sharded deal
struct Gather {  // one all-gather between `world` threads: the last to arrive releases the others
    uint32_t world; bool fail = false;
    std::mutex m; std::condition_variable cv; uint32_t arrived = 0; bool done = false; std::vector<unsigned char> all; int calls = 0;
    explicit Gather(uint32_t w) : world(w) {}
};
struct ThreadExchange : hqprice::Exchange {
    Gather &g;
    ThreadExchange(Gather &gather, uint32_t r) : g(gather) { rank = r; world = gather.world; }
    bool allgather(const void *send, void *recv, size_t bytes) override {
        std::unique_lock<std::mutex> lk(g.m);
        g.calls++;
        if (g.fail) return false;  // at once: nobody waits for anybody
        if (g.all.size() != bytes * world) g.all.assign(bytes * world, 0);
        if (bytes) memcpy(g.all.data() + (size_t)rank * bytes, send, bytes);
        if (++g.arrived == world) { g.done = true; g.cv.notify_all(); }
        else g.cv.wait(lk, [&] { return g.done; });
        if (bytes) memcpy(recv, g.all.data(), bytes * world);
        return true;
    }
};
struct FailingBlocks : hqhost::BlockSolver {  // a launch that does not come about
    bool solve(const hqblock::ColTable &, const hqblock::ClassTable &, const hqblock::Output &) override { return false; }
};

enum Mode { DEAL, PASS, INNER_FAILS, GATHER_FAILS };
static void run_ranks(const Launch &t, uint32_t world, Mode mode, uint32_t failing_rank, const Answer &want) {
    Gather g(world);
    g.fail = mode == GATHER_FAILS;
    std::vector<Answer> got(world, Answer(t.nd, t.NC));
    std::vector<int> ok(world, -1);
    std::vector<std::thread> th;
    for (uint32_t r = 0; r < world; r++)
        th.emplace_back([&, r] {
            ThreadExchange ex(g, r);
            EmulatedBlocks emu(4096); FailingBlocks bad;
            hqhost::BlockSolver &inner = mode == INNER_FAILS && r == failing_rank ? static_cast<hqhost::BlockSolver &>(bad) : emu;
            ShardedBlocks sh(inner, ex, mode == PASS ? t.nd + 1 : 0);
            ok[r] = sh.begin(t.ct, t.cl, got[r].out()) && sh.finish();
        });
    for (auto &x : th) x.join();  // (a rank left waiting in the exchange would hang here: the test's time limit is the check that nobody blocks)
    const bool dealt = world > 1 && mode != PASS;
    for (uint32_t r = 0; r < world; r++) {
        if (mode == GATHER_FAILS && dealt) { CHECK(ok[r] == 0, "rank %u of %u: finish() after a failed all-gather", r, world); continue; }
        CHECK(ok[r] == 1, "rank %u of %u, mode %d", r, world, (int)mode);
        if (mode == INNER_FAILS && dealt) {
            for (uint32_t i = 0; i < t.nd; i++) {
                const uint32_t *x = got[r].x.data() + (size_t)i * t.NC, *wx = want.x.data() + (size_t)i * t.NC;
                if (i % world == failing_rank) {
                    CHECK(got[r].status[i] == (uint32_t)hqblock::ST_UNSUPPORTED, "rank %u: class %u of the failed rank has status %u", r, i, got[r].status[i]);
                    for (uint32_t c = 0; c < t.NC; c++) CHECK(x[c] == 0, "rank %u: class %u of the failed rank has x[%u] = %u", r, i, c, x[c]);
                } else CHECK(memcmp(x, wx, (size_t)t.NC * 4) == 0 && got[r].status[i] == want.status[i] && got[r].steps[i] == want.steps[i], "rank %u: class %u of a sound rank differs", r, i);
            }
        } else CHECK(got[r] == want, "rank %u of %u, mode %d: the answer differs from the unsharded one", r, world, (int)mode);
    }
    CHECK(g.calls == (dealt ? (int)world : 0), "%d exchange calls on %u ranks, mode %d", g.calls, world, (int)mode);
}

static void check_sharded_deal() {
    for (uint32_t world : {1u, 2u, 3u, 5u}) {
        const uint32_t counts[] = {0, 1, world - 1, world, world + 1, 7, 9};
        for (uint32_t nd : counts) {
            // share arithmetic: the shares sum to nd, and class i is rank i % world's
            uint32_t sum = 0; std::vector<int> owner(nd, -1);
            for (uint32_t r = 0; r < world; r++) {
                const uint32_t n = ShardedBlocks::share(nd, r, world);
                sum += n;
                for (uint32_t j = 0; j < n; j++) { const uint32_t i = r + j * world; CHECK(i < nd && owner[i] == -1, "class %u dealt twice or out of range", i); owner[i] = (int)r; }
            }
            CHECK(sum == nd, "shares of %u classes on %u ranks sum to %u", nd, world, sum);
            for (uint32_t i = 0; i < nd; i++) CHECK(owner[i] == (int)(i % world), "class %u is rank %d's", i, owner[i]);
            CHECK(ShardedBlocks::share(nd, 0, world) == (nd + world - 1) / world, "rank 0 holds the largest share");
            for (int rep = 0; rep < 3; rep++) {
                Launch t(1 + below(8), 1 + below(4), nd, false);
                Answer want(t.nd, t.NC);
                EmulatedBlocks whole(4096);
                CHECK(whole.solve(t.ct, t.cl, want.out()), "unsharded solve");
                run_ranks(t, world, DEAL, 0, want);
                run_ranks(t, world, PASS, 0, want);
                if (world > 1) run_ranks(t, world, INNER_FAILS, below(world), want);  // (one rank alone passes its solver's refusal on: the host solver takes the launch)
                run_ranks(t, world, GATHER_FAILS, 0, want);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the small derivations
static void check_small_functions() {
    const uint32_t ids[3] = {100, 101, 105}; const uint64_t totals[6] = {4, 0, 8, 1, 16, 2}; const int64_t rem[3] = {-1, 5, 7}; const float mu[3] = {0.f, 0.5f, 1.f};
    const uint8_t vflags[6] = {7, 0, 7, 7, 0, 0}; const uint32_t vtmc[6] = {1, 0, 2, 3, 0, 0};
    hqtick_query_workers fake{};
    fake.n_workers = 3; fake.worker_id = ids; fake.worker_total = totals; fake.worker_remaining_ns = rem; fake.worker_min_utilization = mu;
    hqhost::WorkerSet fw;
    fw.blocked.assign(7, {{1u, (uint8_t)0}}); fw.flags = vflags; fw.group = ids;  // (left over from another use: all of it goes)
    fake_worker_set(fw, &fake, 2, vflags, vtmc, 2);
    CHECK(fw.n == 3 && fw.R == 2 && fw.id == ids && fw.total == totals && fw.free_ == totals && fw.remaining_ns == rem && fw.min_util == mu, "fake workers: fresh, free == total");
    CHECK(fw.flags == nullptr && fw.group == nullptr && fw.vflags == vflags && fw.vtmc == vtmc && fw.n_variant_slots == 2, "fake workers: flags and K2's output");
    CHECK(fw.blocked.size() == 3 && fw.blocked[0].empty() && fw.blocked[2].empty(), "fake workers: nothing blocked");
    CHECK(fw.is_free(1) && fw.vf(1, 0) == 7 && fw.tmc(1, 1) == 3, "fake workers: accessors");
    fake.n_workers = 0;
    fake_worker_set(fw, &fake, 2, nullptr, nullptr, 0);
    CHECK(fw.n == 0 && fw.blocked.empty(), "no fake workers");

    std::vector<uint8_t> loaded{9, 9};
    hqhost::Counts none;  // nothing placed, optimal: an idle tick
    loaded_flags(none, 4, loaded);
    CHECK(loaded == std::vector<uint8_t>({0, 0, 0, 0}), "empty counts load nobody");
    CHECK(none.empty() && tick_status(none) == HQTICK_DONE, "empty optimal counts: done");
    none.is_optimal = false;
    CHECK(tick_status(none) == HQTICK_NO_PROGRESS, "empty counts, not optimal: no progress");
    hqhost::Counts some;
    some.keys = {{0, 0}, {3, 1}};
    some.per_key = {{{0, 2}, {2, 0}}, {{1, 1}}};  // (a pair with count 0 loads nobody)
    loaded_flags(some, 4, loaded);
    CHECK(loaded == std::vector<uint8_t>({1, 1, 0, 0}), "loaded flags");
    CHECK(!some.empty() && tick_status(some) == HQTICK_DONE, "counts, optimal: done");
    some.is_optimal = false;
    CHECK(tick_status(some) == HQTICK_NEED_MORE_COMPUTE, "counts, not optimal: need more compute");
    hqhost::Counts mn;  // only a multi-node placement
    mn.is_optimal = false; mn.mn_rq = {2}; mn.mn_sets = {{{0, 1}}};
    loaded_flags(mn, 2, loaded);
    CHECK(loaded == std::vector<uint8_t>({0, 0}) && tick_status(mn) == HQTICK_NEED_MORE_COMPUTE, "a multi-node set is progress");
}

int main() {
    check_layout_and_emulation();
    check_sharded_deal();
    check_small_functions();
    printf("%ld checks ok\n", checks);
    return 0;
}
