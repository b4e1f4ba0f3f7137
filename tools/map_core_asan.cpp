// The mapping plan (hyperqueue_amd/csrc/map_core.h) under AddressSanitizer + UBSan: a stand-alone program, every table in an exact-size heap block, the plan's
// storage handed out at exactly plan_head_words + small_words.  A few hundred small random ticks (1-9 workers, 1-5 requests, 1-3 levels; the pair form and the
// by_class form of the counts, one_class included; prefill sets in front of and inside the queues; 0-4 Retracting tasks; the dense and the view form of the
// table; 1 and 3 shards) through the five stages and both packers, with the plan's invariants checked, and each refusal with its code and text.
// Built and run by tests/test_map_core.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o map_core_asan tools/map_core_asan.cpp && ./map_core_asan
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../hyperqueue_amd/csrc/map_core.h"

using namespace hqmap;

static long checks = 0, ticks_ok = 0, ticks_refused = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
template <class T> static void exact(std::vector<T> &v) { v.shrink_to_fit(); }  // (capacity == size: one element past the end is outside the heap block)

static const char *const UNDERFLOW = "solver placed more tasks than the queue holds (reference panics, taskqueue.rs:327)";
static const char *const MN_PREFILL = "multi-node queue with a prefill set";
static const char *const MN_UNDERFLOW = "multi-node placement exceeds its queue";
static const char *const NOT_READY = "a retracting task is not in the ready set";
static const char *const NO_READY_SET = "retracting tasks without a ready set";
static const char *const MN_RETRACTING = "a Retracting task was taken by a multi-node placement";
static const char *const PREFILL_ASSERTS = "a Retracting task reached take_tasks_for_prefill: the reference asserts task.is_waiting() (mapping.rs:221)";

// One tick's inputs, each array in a heap block of its own.
struct Tick {
    uint32_t W = 0, Q = 0, L = 0, R = 1;
    hqscan::Table sc; hqhost::Counts cnt; hqtick_snapshot s{};
    std::vector<hqhost::RequestView> rqs; std::vector<hqhost::VariantView> variants;
    std::vector<uint32_t> ent_res; std::vector<uint8_t> ent_kind; std::vector<uint64_t> ent_amount;
    std::vector<uint32_t> worker_id, prefill_off, prefill_worker, prefilled_off, prefilled_rq, retr_worker, retr_redirect, retr_key, retr_rank, ledger_pf;
    std::vector<uint64_t> worker_free, worker_total, prefill_priority, prefill_task, retr_task;
    std::vector<uint8_t> worker_flags;
    std::vector<uint32_t> q_total;
    std::unique_ptr<uint32_t[]> block; size_t block_words = 0;
    uint32_t reserve = 0, fill_max = 2, flags = 0, shard_index = 0, shard_count = 1; bool sink = false, transpose_on = true;
    static uint32_t *storage(void *user, size_t words) { Tick *t = static_cast<Tick *>(user); t->block.reset(new uint32_t[words]); t->block_words = words; return t->block.get(); }
    PlanIn in() {
        PlanIn p{};
        p.sc = &sc; p.cnt = &cnt; p.s = &s; p.rqs = rqs.data(); p.variants = variants.data();
        p.proactive_filling_reserve = reserve; p.proactive_filling_max = fill_max; p.flags = flags; p.sink = sink; p.shard_index = shard_index; p.shard_count = shard_count;
        p.N = 0; for (uint32_t n : q_total) p.N += n;
        p.retr_key = retr_key.data(); p.retr_rank = retr_rank.data();
        if (!ledger_pf.empty()) { p.ledger_pf = ledger_pf.data(); p.ledger_pf_stride = Q; }
        p.transpose_on = transpose_on; p.storage = storage; p.user = this;
        return p;
    }
};

// the table of a ready set with hist[l * Q + q] tasks per (level, request): the dense form, or the view's run form of the same queues
static void make_table(Tick &t, const std::vector<uint32_t> &hist, bool view) {
    hqscan::Table &sc = t.sc; const uint32_t Q = t.Q, L = t.L;
    sc.L = L; sc.Q = Q; sc.levels.resize(L); for (uint32_t l = 0; l < L; l++) sc.levels[l] = 1000 - 10 * l;
    t.q_total.assign(Q, 0); for (uint32_t l = 0; l < L; l++) for (uint32_t q = 0; q < Q; q++) t.q_total[q] += hist[(size_t)l * Q + q];
    if (!view) { sc.G = L * Q; sc.hist = hist; exact(sc.hist); hqscan::runs_from_hist(sc); }
    else {  // runs in request order, each at its first position in the permutation (request ascending, priority descending)
        sc.ordered = true; sc.run_off.assign(Q + 1, 0);
        uint32_t pos = 0;
        for (uint32_t q = 0; q < Q; q++) {
            for (uint32_t l = 0; l < L; l++) {
                const uint32_t c = hist[(size_t)l * Q + q];
                if (!c) continue;
                sc.run_cnt.push_back(c); sc.run_group.push_back((uint32_t)sc.run_group.size()); sc.run_level.push_back(l); sc.run_start.push_back(pos); sc.run_prio.push_back(sc.levels[l]);
                pos += c;
            }
            sc.run_off[q + 1] = (uint32_t)sc.run_cnt.size();
        }
        sc.G = (uint32_t)sc.run_cnt.size();
    }
    exact(sc.run_off); exact(sc.run_cnt); exact(sc.run_group); exact(sc.run_level); exact(sc.run_start); exact(sc.run_prio); exact(sc.levels);
}

static void make_cluster(Tick &t) {
    const uint32_t W = t.W, Q = t.Q;
    t.worker_id.resize(W); uint32_t id = 1 + below(5); for (uint32_t w = 0; w < W; w++) { t.worker_id[w] = id; id += 1 + below(40); }
    t.worker_free.assign((size_t)W * t.R, 0); t.worker_total.assign((size_t)W * t.R, 0);
    for (uint32_t w = 0; w < W; w++) { t.worker_total[w] = 10000ull * (1 + below(8)); t.worker_free[w] = t.worker_total[w] - 10000ull * below(2); }
    if (below(3) == 0) { t.worker_flags.resize(W); for (uint32_t w = 0; w < W; w++) t.worker_flags[w] = below(6) ? HQ_WORKER_SN : 0; }
    for (uint32_t q = 0; q < Q; q++) {  // 1-2 variants per request, one entry each
        const uint32_t nv = 1 + below(2);
        t.rqs.push_back({(uint32_t)t.ent_res.size(), nv});
        for (uint32_t v = 0; v < nv; v++) { t.ent_res.push_back(0); t.ent_kind.push_back(below(8) ? HQ_ENTRY_AMOUNT : HQ_ENTRY_ALL); t.ent_amount.push_back(10000ull * (1 + below(3))); }
    }
    exact(t.ent_res); exact(t.ent_kind); exact(t.ent_amount); exact(t.rqs);
    for (size_t v = 0; v < t.ent_res.size(); v++) t.variants.push_back({t.ent_res.data() + v, t.ent_kind.data() + v, t.ent_amount.data() + v, 1, 0, 10000, 0});
    exact(t.variants);
    hqtick_snapshot &s = t.s;
    s.n_workers = W; s.n_requests = Q; s.n_resources = t.R; s.worker_id = t.worker_id.data(); s.worker_free = t.worker_free.data(); s.worker_total = t.worker_total.data();
    s.worker_flags = t.worker_flags.empty() ? nullptr : t.worker_flags.data();
}

// the placement: per key (worker, count) pairs in a random order, at most `room[q]` tasks per request unless `overdraw`
static void make_counts(Tick &t, std::vector<uint32_t> room, bool by_class, bool one_class, bool overdraw) {
    hqhost::Counts &c = t.cnt; const uint32_t W = t.W, Q = t.Q;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> pairs;
    for (uint32_t q = 0; q < Q; q++) for (uint32_t v = 0; v < t.rqs[q].n_variants; v++) {
        if (below(3) == 0) continue;
        std::vector<uint32_t> order(W); for (uint32_t w = 0; w < W; w++) order[w] = w;
        for (uint32_t w = W; w > 1; w--) std::swap(order[w - 1], order[below(w)]);
        std::vector<std::pair<uint32_t, uint32_t>> pk;
        const uint32_t same = one_class ? 1 + below(3) : 0;
        for (uint32_t w : order) {
            if (!one_class && below(3) == 0) continue;
            uint32_t n = one_class ? same : 1 + below(3);
            if (!overdraw) { if (one_class) { if (room[q] < n) { pk.clear(); break; } } else n = std::min(n, room[q]); }
            if (!n) continue;
            room[q] -= std::min(room[q], n);
            pk.push_back({w, n});
        }
        if (pk.empty() || (one_class && pk.size() != W)) continue;
        c.keys.push_back({q, (uint8_t)v}); pairs.push_back(pk);
    }
    if (!by_class) { c.per_key = pairs; c.pairs_built = true; for (auto &pk : c.per_key) exact(pk); exact(c.per_key); exact(c.keys); return; }
    // the same placement as classes: every worker a class of its own (one_class: one class for all), the all-zero class behind them
    const uint32_t nk = (uint32_t)c.keys.size(), ncl = one_class ? 1 : W;
    c.by_class = true; c.one_class = one_class; c.pairs_built = false; c.n_cols = nk;
    c.wclass.resize(W); for (uint32_t w = 0; w < W; w++) c.wclass[w] = one_class ? 0 : w;
    c.class_x.assign((size_t)(ncl + 1) * std::max(nk, 1u), 0); c.key_col.resize(nk); c.key_list.resize(nk); c.lists.resize(nk);
    for (uint32_t k = 0; k < nk; k++) {
        c.key_col[k] = k; c.key_list[k] = k;
        for (auto &wc : pairs[k]) { c.class_x[(size_t)c.wclass[wc.first] * nk + k] = wc.second; c.lists[k].widx.push_back(wc.first); }
        exact(c.lists[k].widx);
    }
    exact(c.keys); exact(c.wclass); exact(c.class_x); exact(c.key_col); exact(c.key_list); exact(c.lists);
}

static uint32_t count_of(Tick &t, uint32_t k, uint32_t w) { t.cnt.pairs(); for (auto &wc : t.cnt.per_key[k]) if (wc.first == w) return wc.second; return 0; }

// the five stages; returns the refusing stage's code (0: none), *why its text
static int run_plan(Tick &t, Plan &ps, HostResult &hr, const PlanIn &in, const char **why) {
    int rc;
    if ((rc = plan_keys(ps, hr, in, why))) return rc;
    const hqtick_snapshot &s = t.s; const uint32_t W = t.W, Q = t.Q, nkeys = ps.nkeys;
    size_t n_cnt = 0; for (uint32_t k = 0; k < nkeys; k++) n_cnt += t.cnt.key_size(k);
    CHECK(t.block_words == ps.plan_head_words + small_words(nkeys, n_cnt, Q, W, n_groups(t.sc), s.n_retracting, t.sc.ordered), "storage of %zu words", t.block_words);
    for (uint32_t k = 0; k < nkeys; k++) {
        uint32_t sum = 0; for (uint32_t w = 0; w < W; w++) sum += count_of(t, k, w);
        CHECK(ps.key_sum[k] == sum, "key %u: key_sum %u, counts %u", k, ps.key_sum[k], sum);
        uint32_t n = 0; for (uint32_t w = 0; w < W; w++) { const uint32_t c = count_of(t, k, w); CHECK(ps.wcnt[(size_t)k * W + w] == c && (ps.wpos[(size_t)k * W + w] != NONE) == (c != 0), "key %u worker %u", k, w); n += c != 0; }
        // worker-major only: plain queue, one key of its request at the head of the queue, every worker the same count
        if (ps.key_tr[k]) {
            const uint32_t q = ps.key_rq[k]; uint32_t keys_of_q = 0; for (uint32_t kk = 0; kk < nkeys; kk++) keys_of_q += ps.key_rq[kk] == q;
            CHECK(t.transpose_on && s.n_retracting == 0 && keys_of_q == 1 && ps.key_seg[k] == 0 && ps.pf_n[q] == 0 && n > 0, "key %u is worker-major", k);
            for (uint32_t w = 0; w < W; w++) { const uint32_t c = count_of(t, k, w); CHECK(c == 0 || c == ps.key_tr[k], "key %u worker %u: %u of %u", k, w, c, ps.key_tr[k]); }
        }
    }
    for (uint32_t q = 0; q < Q; q++) CHECK(ps.seq_taken[q] <= ps.q_total[q] + ps.pf_n[q] && ps.q_total[q] == t.q_total[q], "request %u: %u taken of %u + %u", q, ps.seq_taken[q], ps.q_total[q], ps.pf_n[q]);
    {   // the key-table image of the early K5a launch, in a block of exactly sweep_words
        const size_t words = sweep_words(nkeys, ps.ord_cnt.size());
        std::unique_ptr<uint32_t[]> img(new uint32_t[words ? words : 1]);
        if (nkeys) { const SweepTables st = pack_sweep_keys(img.get(), ps); CHECK(st.words <= words && st.o_ord + ps.ord_cnt.size() <= words, "sweep image of %zu words in %zu", st.words, words); }
    }
    if ((rc = plan_redirects(ps, hr, in, why))) return rc;
    if ((rc = plan_prefill(ps, hr, in, why))) return rc;
    if ((rc = plan_outputs(ps, hr, in, why))) return rc;
    uint32_t n_sel = 0;
    for (uint32_t q = 0; q < Q; q++) {
        const uint32_t want = ps.zq_taken[q] + ps.new_pf_total[q];
        n_sel += want;
        if (!t.sc.ordered) {
            uint32_t take = 0; for (uint32_t r = t.sc.run_off[q]; r < t.sc.run_off[q + 1]; r++) take += ps.take_base[t.sc.run_group[r]];
            CHECK(take == std::min(want, t.q_total[q]), "request %u: takes %u, wanted %u of %u", q, take, want, t.q_total[q]);
        }
    }
    CHECK(ps.n_sel == n_sel && ps.rq_sel_base[Q] == n_sel, "n_sel %u, sum %u", ps.n_sel, n_sel);
    uint32_t n_rec = 0;
    for (uint32_t w = 0; w < W; w++) {
        CHECK(ps.out_off[w] <= ps.out_off[w + 1], "out_off at %u", w);
        if (t.shard_count > 1 && hqhb::hash_worker_id(t.worker_id[w]) % t.shard_count != t.shard_index) { CHECK(ps.out_off[w] == ps.out_off[w + 1], "another shard's worker %u", w); continue; }
        uint32_t slots = 0; for (uint32_t pi = 0; pi < ps.n_pfq; pi++) if (ps.pfl_j[(size_t)pi * W + w] != NONE) slots += ps.pfq_size[pi];
        CHECK(ps.out_off[w + 1] - ps.out_off[w] == ps.n_assign[w] + slots, "worker %u", w);
        n_rec += ps.n_assign[w] + slots;
    }
    CHECK(ps.n_rec == n_rec, "n_rec %u, sum %u", ps.n_rec, n_rec);
    assemble_host_part(ps, hr, in);
    CHECK(hr.rec_off.size() == (size_t)W + 1 && hr.retract_off.size() == (size_t)W + 1 && hr.retract_off[W] <= ps.retract_pairs.size() && hr.new_free.size() == (size_t)W * t.R, "host part");
    CHECK(hr.red_task.size() == hr.red_kind.size() && hr.red_task.size() == hr.red_worker.size() && hr.red_task.size() == hr.red_variant.size(), "redirect columns");
    for (int with_pfq_rq = 0; with_pfq_rq < 2; with_pfq_rq++) {  // the small tables behind the big ones: never past what small_words said (the block is exactly that long)
        const SmallTables st = pack_small(t.block.get(), ps, t.sc, with_pfq_rq != 0);
        CHECK(st.words <= t.block_words && st.o_rq == ps.plan_head_words && (st.o_holes & 1) == 0 && st.o_holes + 2 * std::max<size_t>(ps.holes.size(), 1) == st.words, "plan of %zu words in %zu", st.words, t.block_words);
    }
    return 0;
}

static bool known_refusal(int rc, const char *why) {
    const std::string w = why ? why : "";
    return (rc == HQTICK_E_QUEUE_UNDERFLOW && (w == UNDERFLOW || w == MN_UNDERFLOW)) || (rc == HQTICK_E_UNSUPPORTED && (w == MN_PREFILL || w == PREFILL_ASSERTS || w == MN_RETRACTING)) ||
           (rc == HQTICK_E_INVALID && (w == NOT_READY || w == NO_READY_SET));
}

static void random_tick(Plan &ps, HostResult &hr, int i) {
    Tick t;
    t.W = 1 + below(9); t.Q = 1 + below(5); t.L = 1 + below(3);
    const uint32_t W = t.W, Q = t.Q, L = t.L;
    const bool view = i % 2 == 1, by_class = (i / 2) % 3 != 0, one_class = (i / 2) % 3 == 2, overdraw = below(12) == 0;
    t.shard_count = (i / 6) % 2 ? 3 : 1; t.shard_index = t.shard_count > 1 ? below(3) : 0;
    t.reserve = below(2); t.fill_max = below(4); t.flags = below(3) == 0 ? HQTICK_FLAG_COMPACT_RECORDS : 0; t.sink = below(8) == 0; t.transpose_on = below(8) != 0;
    std::vector<uint32_t> hist((size_t)L * Q); for (auto &c : hist) c = below(4) ? below(7) : 0;
    make_table(t, hist, view);
    make_cluster(t);
    hqtick_snapshot &s = t.s;
    std::vector<uint32_t> room = t.q_total;
    if (below(2)) {  // prefill sets: at the queue's top priority (inside the queue, behind its first level) or at one of their own (in front of it)
        t.prefill_off.assign(Q + 1, 0); t.prefill_priority.assign(Q, 0);
        for (uint32_t q = 0; q < Q; q++) {
            const uint32_t n = below(3) ? 0 : 1 + below(3);
            const bool has_runs = t.sc.run_off[q] < t.sc.run_off[q + 1];
            t.prefill_priority[q] = has_runs && below(2) ? t.sc.run_prio[t.sc.run_off[q]] : 2000;
            for (uint32_t j = 0; j < n; j++) { t.prefill_task.push_back(900000 + t.prefill_task.size()); t.prefill_worker.push_back(below(W)); }
            t.prefill_off[q + 1] = (uint32_t)t.prefill_task.size(); room[q] += n;
        }
        exact(t.prefill_task); exact(t.prefill_worker);
        s.prefill_off = t.prefill_off.data(); s.prefill_priority = t.prefill_priority.data(); s.prefill_task = t.prefill_task.data(); s.prefill_worker = t.prefill_worker.data();
        t.prefilled_off.assign(W + 1, 0);  // ... and the workers' side of them
        for (uint32_t w = 0; w < W; w++) { for (uint32_t j = below(3); j > 0; j--) t.prefilled_rq.push_back(below(Q + 1)); t.prefilled_off[w + 1] = (uint32_t)t.prefilled_rq.size(); }
        exact(t.prefilled_rq);
        if (below(2)) { s.prefilled_off = t.prefilled_off.data(); s.prefilled_rq = t.prefilled_rq.data(); }
        else { t.ledger_pf.assign((size_t)W * Q, 0); for (auto &c : t.ledger_pf) c = below(4) == 0; }
    }
    make_counts(t, room, by_class, one_class, overdraw);
    if (below(6) == 0) {  // a multi-node placement at the head of a queue
        const uint32_t q = below(Q), n = 1 + below(2);
        t.cnt.mn_rq.push_back(q); t.cnt.mn_sets.push_back({});
        for (uint32_t j = 0; j < n; j++) { std::vector<uint32_t> set; for (uint32_t w = 0; w < W; w++) if (below(2)) set.push_back(w); if (set.empty()) set.push_back(0); exact(set); t.cnt.mn_sets[0].push_back(set); }
    }
    const uint32_t nr = below(5) * (below(3) != 0);  // Retracting tasks: positions in their queues (now and then one that is not in the ready set)
    uint64_t n_ready = 0; for (uint32_t n : t.q_total) n_ready += n;
    if (nr && (n_ready || below(4) == 0)) {
        for (uint32_t j = 0; j < nr; j++) {
            uint32_t key = 0xFFFFFFFFu, rank = 0;
            if (n_ready && below(10)) {
                uint32_t r = below((uint32_t)t.sc.run_cnt.size());
                uint32_t q = 0; while (t.sc.run_off[q + 1] <= r) q++;
                key = view ? q : t.sc.run_level[r] * Q + q; rank = (view ? t.sc.run_start[r] : 0) + below(t.sc.run_cnt[r]);
                bool taken = false; for (size_t x = 0; x < t.retr_key.size(); x++) taken = taken || (t.retr_key[x] == key && t.retr_rank[x] == rank);
                if (taken) key = 0xFFFFFFFFu;  // (two tasks cannot share a queue position)
            }
            t.retr_key.push_back(key); t.retr_rank.push_back(rank); t.retr_task.push_back(500 + 3 * j); t.retr_worker.push_back(below(W)); t.retr_redirect.push_back(below(2) ? below(W) : HQ_NO_WORKER);
        }
        exact(t.retr_key); exact(t.retr_rank); exact(t.retr_task); exact(t.retr_worker); exact(t.retr_redirect);
        s.n_retracting = nr; s.retracting_task = t.retr_task.data(); s.retracting_worker = t.retr_worker.data();
        if (below(2)) s.retracting_redirect_worker = t.retr_redirect.data();
    }
    const PlanIn in = t.in();
    const char *why = nullptr;
    const int rc = run_plan(t, ps, hr, in, &why);
    if (rc) { CHECK(known_refusal(rc, why), "tick %d: %d %s", i, rc, why ? why : "(null)"); ticks_refused++; } else ticks_ok++;
}

// ---- each refusal on a tick made for it: one worker of 4 cpus, one request, a queue of `n_queue` tasks at one level of which the worker takes `take`
static Tick small_tick(uint32_t n_queue, uint32_t take) {
    Tick t; t.W = 1; t.Q = 1; t.L = 1;
    make_table(t, {n_queue}, false);
    t.worker_id = {7}; t.worker_free = {40000}; t.worker_total = {40000};
    t.rqs = {{0, 1}}; t.ent_res = {0}; t.ent_kind = {HQ_ENTRY_AMOUNT}; t.ent_amount = {10000};
    t.variants = {{t.ent_res.data(), t.ent_kind.data(), t.ent_amount.data(), 1, 0, 10000, 0}};
    t.s.n_workers = 1; t.s.n_requests = 1; t.s.n_resources = 1; t.s.worker_id = t.worker_id.data(); t.s.worker_free = t.worker_free.data(); t.s.worker_total = t.worker_total.data();
    if (take) { t.cnt.keys = {{0, 0}}; t.cnt.per_key = {{{0, take}}}; }
    return t;
}
static void with_retracting(Tick &t, uint32_t key, uint32_t rank) {
    t.retr_key = {key}; t.retr_rank = {rank}; t.retr_task = {501}; t.retr_worker = {0};
    t.s.n_retracting = 1; t.s.retracting_task = t.retr_task.data(); t.s.retracting_worker = t.retr_worker.data();
}
static void with_prefill_set(Tick &t) {
    t.prefill_off = {0, 1}; t.prefill_priority = {2000}; t.prefill_task = {900000}; t.prefill_worker = {0};
    t.s.prefill_off = t.prefill_off.data(); t.s.prefill_priority = t.prefill_priority.data(); t.s.prefill_task = t.prefill_task.data(); t.s.prefill_worker = t.prefill_worker.data();
}
static void check_refused(Tick &t, int code, const char *text) {
    Plan ps; HostResult hr; const PlanIn in = t.in(); const char *why = nullptr;
    const int rc = run_plan(t, ps, hr, in, &why);
    CHECK(rc == code && why && std::string(why) == text, "%d %s, expected %d %s", rc, why ? why : "(null)", code, text);
}

int main() {
    Plan ps; HostResult hr;  // reused from tick to tick, as a context reuses them
    for (int i = 0; i < 600; i++) random_tick(ps, hr, i);
    CHECK(ticks_ok >= 300 && ticks_refused >= 10, "%ld ticks planned, %ld refused", ticks_ok, ticks_refused);

    { Tick t = small_tick(3, 4); check_refused(t, HQTICK_E_QUEUE_UNDERFLOW, UNDERFLOW); }                                       // 4 placed on a queue of 3
    { Tick t = small_tick(3, 0); with_prefill_set(t); t.cnt.mn_rq = {0}; t.cnt.mn_sets = {{{0}}}; check_refused(t, HQTICK_E_UNSUPPORTED, MN_PREFILL); }
    { Tick t = small_tick(1, 0); t.cnt.mn_rq = {0}; t.cnt.mn_sets = {{{0}, {0}}}; check_refused(t, HQTICK_E_QUEUE_UNDERFLOW, MN_UNDERFLOW); }   // two multi-node tasks from a queue of 1
    { Tick t = small_tick(5, 1); with_retracting(t, 0xFFFFFFFFu, 0); check_refused(t, HQTICK_E_INVALID, NOT_READY); }           // k_rank_of did not find it
    { Tick t = small_tick(0, 0); with_retracting(t, 0, 0); check_refused(t, HQTICK_E_INVALID, NO_READY_SET); }
    { Tick t = small_tick(5, 0); t.cnt.mn_rq = {0}; t.cnt.mn_sets = {{{0}}}; with_retracting(t, 0, 0); check_refused(t, HQTICK_E_UNSUPPORTED, MN_RETRACTING); }
    // the worker takes 1 of 5 and is prefilled min(4 / 1, fill_max = 2) more: queue positions 1 and 2 — a Retracting task at position 1 reaches the prefill step
    { Tick t = small_tick(5, 1); with_retracting(t, 0, 1); check_refused(t, HQTICK_E_UNSUPPORTED, PREFILL_ASSERTS); }
    {   // ... at position 3 it stays in its queue, at position 0 it is taken: a redirect to the same worker, a hole, no record
        Tick t = small_tick(5, 1); with_retracting(t, 0, 3);
        Plan p; HostResult h; const PlanIn in = t.in(); const char *why = nullptr;
        CHECK(run_plan(t, p, h, in, &why) == 0 && h.red_task.empty() && p.n_sel == 3 && p.n_rec == 3, "a Retracting task out of reach: %s", why ? why : "");
        Tick u = small_tick(5, 1); with_retracting(u, 0, 0);
        const PlanIn in2 = u.in();
        CHECK(run_plan(u, p, h, in2, &why) == 0 && h.red_task.size() == 1 && h.red_kind[0] == HQ_REDIRECT_SAME_WORKER && p.holes.size() == 1 && p.n_assign[0] == 0, "a Retracting task taken: %s", why ? why : "");
    }
    printf("%ld ticks planned, %ld refused, %ld checks ok\n", ticks_ok, ticks_refused, checks);
    return 0;
}
