// The tick's host stages without HIP (hyperqueue_amd/csrc/tick_core.h) under AddressSanitizer + UBSan: a stand-alone program, every array a snapshot points to in
// an exact-size heap block.
//   validate         one hand-written snapshot per refusal, each refused with its text; the smallest valid snapshot and the empty edges (W = 0, Q = 0, n_ready = 0)
//   table_from_hist, queue_levels   a 3-level x 2-request histogram with a zero cell; a prefill set at the top level's priority (merged) and one at a new
//                    priority (inserted in front)
//   export_batches   batches with 0, 1 and 2 cuts and 0 to 2 blockers: the three offset arrays monotone and ending at their arrays' sizes
//   with_row_check   on a stub pass that records its arguments: nothing pending, pending and passing, pending and failing, an error beside a failing check, a check
//                    the pass settled itself, a discard that fails
//   plan_stages      on a stub `after`: 0, 1, 2, 3 in order; a non-zero answer ends the sequence with its code; a stage's refusal ends it with the stage's text
//   query_tail       two fake workers, one request, a stub solve that loads worker 1
// The header calls three functions that the library defines in host_model.cpp and milp.cpp (group_equal_rows, create_task_batches, run_row_check).  This program
// defines them itself, as recorders: what is checked here is the sequence around them, and tests/test_host_stages.py and tests/test_deferred_row_check.py run the
// real ones through the same header.
// Built and run by tests/test_tick_core.py; CPU only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o tick_core_asan tools/tick_core_asan.cpp && ./tick_core_asan
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../hyperqueue_amd/csrc/tick_core.h"

using namespace hqstages;

static long checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

// ---------------------------------------------------------------------------------------------- the recorders
struct GroupCall { const hqhost::WorkerSet *ws; bool all_solver; };
static std::vector<GroupCall> g_group_calls;
static int g_batch_calls = 0, g_row_checks = 0;
static std::vector<bool> g_verdicts;  // what the next run_row_check calls answer, first to last
namespace hqhost {
void group_equal_rows(WorkerSet &ws, bool all_solver) { g_group_calls.push_back({&ws, all_solver}); ws.rows.valid = true; }
std::vector<TaskBatch> create_task_batches(const Problem &, const std::vector<QueueLevels> &queues) {  // one batch per request, as large as its queue
    g_batch_calls++;
    std::vector<TaskBatch> out;
    for (size_t q = 0; q < queues.size(); q++) { TaskBatch b; b.rq = (uint32_t)q; for (auto &l : queues[q].levels) b.size += l.second; out.push_back(b); }
    return out;
}
}  // namespace hqhost
namespace hqmilp {
bool run_row_check(const Model &, RowCheck &rc) {
    rc.pending = false;
    CHECK((size_t)g_row_checks < g_verdicts.size(), "row check %d was not expected", g_row_checks);
    return g_verdicts[(size_t)g_row_checks++];
}
}  // namespace hqmilp

// ---------------------------------------------------------------------------------------------- snapshots
template <class T> struct Arr {  // a heap block of exactly n elements (null when empty)
    std::unique_ptr<T[]> p; size_t n = 0;
    const T *set(std::initializer_list<T> v) { n = v.size(); p.reset(n ? new T[n] : nullptr); size_t i = 0; for (const T &x : v) p[i++] = x; return p.get(); }
};
// two workers, one request of one variant with one entry, two ready tasks: valid as it stands
struct Snap {
    hqtick_snapshot s{};
    Arr<uint32_t> worker_id, worker_group, blocked_worker, blocked_rq, assigned_off, assigned_rq, prefilled_off, prefilled_rq, rq_variant_off, variant_entry_off, entry_resource,
        task_rq, prefill_off, prefill_worker, retracting_worker, retracting_redirect_worker;
    Arr<uint64_t> worker_total, worker_free, entry_amount, task_id, task_priority, prefill_priority, prefill_task, retracting_task;
    Arr<uint8_t> blocked_variant, assigned_variant, entry_kind;
    Snap() {
        s.n_resources = 1;
        s.n_workers = 2; s.worker_id = worker_id.set({3, 7}); s.worker_total = worker_total.set({40000, 80000}); s.worker_free = worker_free.set({40000, 80000});
        s.n_requests = 1; s.rq_variant_off = rq_variant_off.set({0, 1}); s.variant_entry_off = variant_entry_off.set({0, 1});
        s.entry_resource = entry_resource.set({0}); s.entry_kind = entry_kind.set({HQ_ENTRY_AMOUNT}); s.entry_amount = entry_amount.set({10000});
        s.n_ready = 2; s.task_id = task_id.set({1, 2}); s.task_priority = task_priority.set({5, 5}); s.task_rq = task_rq.set({0, 0});
    }
};
static void refused(const hqtick_snapshot *s, bool need_tasks, const char *text) {
    std::string err = "untouched";
    const int rc = validate(s, need_tasks, err);
    CHECK(rc == HQTICK_E_INVALID && err == text, "expected the refusal \"%s\", got %d \"%s\"", text, rc, err.c_str());
}
static void accepted(const hqtick_snapshot *s, bool need_tasks, const char *what) {
    std::string err = "untouched";
    const int rc = validate(s, need_tasks, err);
    CHECK(rc == 0 && err == "untouched", "%s: refused with %d \"%s\"", what, rc, err.c_str());
}

static void check_validate() {
    refused(nullptr, true, "null snapshot");
    { Snap b; b.s.worker_free = nullptr; refused(&b.s, true, "worker arrays missing"); }
    { Snap b; b.s.worker_id = b.worker_id.set({7, 7}); refused(&b.s, true, "worker ids not ascending"); }
    { Snap b; b.s.variant_entry_off = nullptr; refused(&b.s, true, "request arrays missing"); }
    { Snap b; b.s.rq_variant_off = b.rq_variant_off.set({0, 0}); refused(&b.s, true, "request without variants"); }
    { Snap b; b.s.rq_variant_off = b.rq_variant_off.set({0, 33}); refused(&b.s, true, "more than 32 variants"); }
    { Snap b; b.s.entry_resource = b.entry_resource.set({1}); refused(&b.s, true, "entry resource id out of range"); }
    { Snap b; b.s.entry_amount = b.entry_amount.set({0}); refused(&b.s, true, "zero amount request"); }
    { Snap b; b.s.entry_amount = b.entry_amount.set({0}); b.s.entry_kind = b.entry_kind.set({HQ_ENTRY_ALL}); accepted(&b.s, true, "an ALL entry's amount is ignored"); }
    { Snap b; b.s.task_rq = nullptr; refused(&b.s, true, "ready-set columns missing"); accepted(&b.s, false, "a tick on a resident set reads no columns"); }
    { Snap b; b.s.task_id = b.task_id.set({2, 2}); refused(&b.s, true, "ready set not sorted by task id"); accepted(&b.s, false, "a tick on a resident set reads no ids"); }
    { Snap b; b.s.n_blocked = 1; refused(&b.s, true, "blocked arrays missing"); }
    {
        Snap b; b.s.n_blocked = 1; b.s.blocked_worker = b.blocked_worker.set({2}); b.s.blocked_rq = b.blocked_rq.set({0}); b.s.blocked_variant = b.blocked_variant.set({0});
        refused(&b.s, true, "blocked worker index");
        b.s.blocked_worker = b.blocked_worker.set({1}); b.s.blocked_rq = b.blocked_rq.set({1});
        refused(&b.s, true, "blocked request id out of range");
        b.s.blocked_rq = b.blocked_rq.set({0}); b.s.blocked_variant = b.blocked_variant.set({1});
        refused(&b.s, true, "blocked variant out of range");
        b.s.blocked_variant = b.blocked_variant.set({0});
        accepted(&b.s, true, "one blocked pair");
    }
    { Snap b; b.s.worker_group = b.worker_group.set({0, 1}); refused(&b.s, true, "worker_group >= n_groups"); b.s.n_groups = 2; accepted(&b.s, true, "two groups"); }
    { Snap b; b.s.assigned_off = b.assigned_off.set({0, 2, 1}); refused(&b.s, true, "assigned_off not monotone"); }
    { Snap b; b.s.assigned_off = b.assigned_off.set({0, 1, 1}); b.s.assigned_rq = b.assigned_rq.set({0}); refused(&b.s, true, "assigned arrays missing"); }
    { Snap b; b.s.assigned_off = b.assigned_off.set({0, 0, 0}); accepted(&b.s, true, "an empty assigned CSR needs no arrays"); }
    { Snap b; b.s.prefilled_off = b.prefilled_off.set({0, 2, 1}); refused(&b.s, true, "prefilled_off not monotone"); }
    { Snap b; b.s.prefilled_off = b.prefilled_off.set({0, 1, 1}); refused(&b.s, true, "prefilled_rq missing"); }
    { Snap b; b.s.prefill_off = b.prefill_off.set({1, 0}); refused(&b.s, true, "prefill_off not monotone"); }
    {
        Snap b; b.s.prefill_off = b.prefill_off.set({0, 1}); b.s.prefill_priority = b.prefill_priority.set({9}); b.s.prefill_task = b.prefill_task.set({1});
        refused(&b.s, true, "prefill arrays missing");
        b.s.prefill_worker = b.prefill_worker.set({2});
        refused(&b.s, true, "prefill worker index");
        b.s.prefill_worker = b.prefill_worker.set({1});
        accepted(&b.s, true, "one prefilled task");
    }
    { Snap b; b.s.n_retracting = 1; b.s.retracting_task = b.retracting_task.set({1}); refused(&b.s, true, "retracting arrays missing"); }
    {
        Snap b; b.s.n_retracting = 2; b.s.retracting_task = b.retracting_task.set({1, 2}); b.s.retracting_worker = b.retracting_worker.set({0, 2});
        refused(&b.s, true, "retracting worker index");
        b.s.retracting_worker = b.retracting_worker.set({0, 1}); b.s.retracting_task = b.retracting_task.set({2, 2});
        refused(&b.s, true, "retracting tasks not ascending");
        b.s.retracting_task = b.retracting_task.set({1, 2}); b.s.retracting_redirect_worker = b.retracting_redirect_worker.set({HQ_NO_WORKER, 2});
        refused(&b.s, true, "retracting redirect worker index");
        b.s.retracting_redirect_worker = b.retracting_redirect_worker.set({HQ_NO_WORKER, 0});
        accepted(&b.s, true, "two Retracting tasks, one redirected");
    }
    { Snap b; accepted(&b.s, true, "the base snapshot"); }
    { hqtick_snapshot none{}; accepted(&none, true, "the all-zero snapshot"); }
    { Snap b; b.s.n_workers = 0; b.s.worker_id = nullptr; b.s.worker_total = nullptr; b.s.worker_free = nullptr; accepted(&b.s, true, "W = 0"); }
    { Snap b; b.s.n_requests = 0; b.s.rq_variant_off = nullptr; b.s.variant_entry_off = nullptr; b.s.entry_resource = nullptr; b.s.entry_kind = nullptr; b.s.entry_amount = nullptr; accepted(&b.s, true, "Q = 0"); }
    { Snap b; b.s.n_ready = 0; b.s.task_id = nullptr; b.s.task_priority = nullptr; b.s.task_rq = nullptr; accepted(&b.s, true, "n_ready = 0"); }
}

// ---------------------------------------------------------------------------------------------- the table and the queue levels
typedef std::vector<std::pair<uint64_t, uint32_t>> Levels;
static void check_tables() {
    Arr<uint64_t> levels; Arr<uint32_t> hist;
    levels.set({30, 20, 10}); hist.set({2, 1, 0, 3, 4, 5});  // hist[level * Q + rq]: request 0 has nothing at priority 20
    const Table sc = table_from_hist(3, levels.p.get(), hist.p.get(), 2);
    CHECK(sc.L == 3 && sc.Q == 2 && sc.G == 6 && !sc.ordered && sc.levels == std::vector<uint64_t>({30, 20, 10}) && sc.hist == std::vector<uint32_t>({2, 1, 0, 3, 4, 5}), "the dense form");
    CHECK(sc.run_off == std::vector<uint32_t>({0, 2, 5}) && sc.run_cnt == std::vector<uint32_t>({2, 4, 1, 3, 5}), "runs per request");
    CHECK(sc.run_group == std::vector<uint32_t>({0, 4, 1, 3, 5}) && sc.run_level == std::vector<uint32_t>({0, 2, 0, 1, 2}) && sc.run_prio == std::vector<uint64_t>({30, 10, 30, 20, 10}), "the runs' groups, levels and priorities");
    const Table none = table_from_hist(0, nullptr, nullptr, 2);
    CHECK(none.L == 0 && none.G == 0 && none.run_off == std::vector<uint32_t>({0, 0, 0}) && none.run_cnt.empty(), "no levels");
    const Table noq = table_from_hist(2, levels.p.get(), nullptr, 0);
    CHECK(noq.Q == 0 && noq.G == 0 && noq.run_off == std::vector<uint32_t>({0}) && noq.hist.empty(), "no requests");

    hqtick_snapshot s{};
    s.n_requests = 2;
    std::vector<hqhost::QueueLevels> q = queue_levels(sc, &s);
    CHECK(q.size() == 2 && q[0].levels == Levels({{30, 2}, {10, 4}}) && q[1].levels == Levels({{30, 1}, {20, 3}, {10, 5}}), "queue levels without prefill sets");
    Arr<uint32_t> pf_off; Arr<uint64_t> pf_prio;
    s.prefill_off = pf_off.set({0, 2, 5}); s.prefill_priority = pf_prio.set({30, 40});  // request 0: two tasks at the top level's priority; request 1: three at a new one
    q = queue_levels(sc, &s);
    CHECK(q[0].levels == Levels({{30, 4}, {10, 4}}), "a prefill set at the top level's priority merges into it");
    CHECK(q[1].levels == Levels({{40, 3}, {30, 1}, {20, 3}, {10, 5}}), "a prefill set at a new priority goes in front");
    s.prefill_off = pf_off.set({0, 0, 1}); s.prefill_priority = pf_prio.set({0, 7});
    q = queue_levels(none, &s);
    CHECK(q[0].levels.empty() && q[1].levels == Levels({{7, 1}}), "a prefill set in front of an empty queue");
}

// ---------------------------------------------------------------------------------------------- the batches' export
static void check_csr(const std::vector<uint32_t> &off, size_t rows, size_t end, const char *what) {
    CHECK(off.size() == rows + 1 && off[0] == 0 && off[rows] == end, "%s: %zu offsets for %zu rows, ending at %u of %zu", what, off.size(), rows, off.empty() ? 0u : off.back(), end);
    for (size_t i = 0; i < rows; i++) CHECK(off[i] <= off[i + 1], "%s not monotone at %zu", what, i);
}
static void check_export() {
    std::vector<hqhost::TaskBatch> batches(3);
    batches[0].rq = 0; batches[0].size = 5; batches[0].limit = 7;
    batches[1].rq = 1; batches[1].size = 3; batches[1].limit = 3; batches[1].limit_reached = true; batches[1].is_blocker = true; batches[1].cuts = {{2, {}}};
    batches[2].rq = 2; batches[2].size = 9; batches[2].limit = 9; batches[2].cuts = {{1, {{0, 9}}}, {4, {{1, HQ_BLOCKER_UNBOUNDED}, {2, 6}}}};
    BatchExport x; hqtick_result out{};
    export_batches(batches, x, &out);
    CHECK(out.n_batches == 3 && x.b_rq == std::vector<uint32_t>({0, 1, 2}) && x.b_size == std::vector<uint32_t>({5, 3, 9}) && x.b_limit == std::vector<uint32_t>({7, 3, 9}), "batch columns");
    CHECK(x.b_lr == std::vector<uint8_t>({0, 1, 0}) && x.b_blk == std::vector<uint8_t>({0, 1, 0}), "batch flags");
    CHECK(x.b_cut_off == std::vector<uint32_t>({0, 0, 1, 3}) && x.c_size == std::vector<uint32_t>({2, 1, 4}), "cuts");
    CHECK(x.c_bl_off == std::vector<uint32_t>({0, 0, 1, 3}) && x.bl_rq == std::vector<uint32_t>({0, 1, 2}) && x.bl_size == std::vector<uint32_t>({9, HQ_BLOCKER_UNBOUNDED, 6}), "blockers");
    check_csr(x.b_cut_off, x.b_rq.size(), x.c_size.size(), "batch_cut_off");
    check_csr(x.c_bl_off, x.c_size.size(), x.bl_rq.size(), "cut_blocker_off");
    CHECK(x.bl_rq.size() == x.bl_size.size() && x.b_rq.size() == x.b_lr.size() && x.b_rq.size() == x.b_blk.size(), "column lengths");
    CHECK(out.batch_rq == x.b_rq.data() && out.batch_size == x.b_size.data() && out.batch_limit == x.b_limit.data() && out.batch_limit_reached == x.b_lr.data() &&
          out.batch_is_blocker == x.b_blk.data() && out.batch_cut_off == x.b_cut_off.data() && out.cut_size == x.c_size.data() && out.cut_blocker_off == x.c_bl_off.data() &&
          out.blocker_rq == x.bl_rq.data() && out.blocker_size == x.bl_size.data(), "the result points into the export");
    export_batches({}, x, &out);  // ... and nothing is left of it on the next one
    CHECK(out.n_batches == 0 && x.b_rq.empty() && x.c_size.empty() && x.bl_rq.empty(), "no batches");
    check_csr(x.b_cut_off, 0, 0, "batch_cut_off of nothing");
    check_csr(x.c_bl_off, 0, 0, "cut_blocker_off of nothing");
}

// ---------------------------------------------------------------------------------------------- the row check's retry
struct PassScript { bool pending; bool settles; int rc; };  // what a pass does: leaves a check pending, settles it itself, returns rc
struct Retry {
    hqhost::Counts cnt;
    std::vector<PassScript> script; std::vector<std::string> log; int discard_rc = 0;
    int run(bool defer) {
        size_t n = 0;
        auto pass = [&](bool d, bool classic) -> int {
            CHECK(n < script.size(), "pass %zu was not expected", n);
            log.push_back(std::string("pass ") + (d ? "defer" : "inline") + (classic ? " classic" : " fast") + (cnt.milp_nodes == 77 ? " stale" : " fresh") + (cnt.row_check_failed() ? " failed" : ""));
            const PassScript p = script[n++];
            cnt.milp_nodes = 77;  // (a trace the pass leaves in the counts)
            cnt.row_check.check.pending = p.pending;
            if (p.settles) cnt.settle_row_check();
            return p.rc;
        };
        auto discard = [&]() -> int { log.push_back("discard"); return discard_rc; };
        return with_row_check(cnt, defer, pass, discard);
    }
};
static void expect_retry(Retry &r, bool defer, std::vector<bool> verdicts, int want_rc, int want_checks, std::vector<std::string> want_log, const char *what) {
    g_verdicts = verdicts; g_row_checks = 0;
    const int rc = r.run(defer);
    std::string got; for (auto &l : r.log) got += l + "; ";
    CHECK(rc == want_rc && g_row_checks == want_checks && r.log == want_log, "%s: rc %d, %d checks, log: %s", what, rc, g_row_checks, got.c_str());
}
static void check_retry() {
    { Retry r; r.script = {{false, false, 0}}; expect_retry(r, true, {}, 0, 0, {"pass defer fast fresh"}, "nothing pending"); }
    { Retry r; r.script = {{false, false, 0}}; expect_retry(r, false, {}, 0, 0, {"pass inline fast fresh"}, "not deferred"); }
    { Retry r; r.script = {{false, false, -3}}; expect_retry(r, true, {}, -3, 0, {"pass defer fast fresh"}, "an error, nothing pending"); }
    { Retry r; r.script = {{true, false, 0}}; expect_retry(r, true, {true}, 0, 1, {"pass defer fast fresh"}, "pending and passing"); CHECK(!r.cnt.row_check_pending() && r.cnt.milp_nodes == 77, "the counts stand"); }
    { Retry r; r.script = {{true, false, -4}}; expect_retry(r, true, {true}, -4, 1, {"pass defer fast fresh"}, "an error beside a passing check stands"); }
    { Retry r; r.script = {{true, false, 0}, {false, false, 0}}; expect_retry(r, true, {false}, 0, 1, {"pass defer fast fresh", "discard", "pass inline classic fresh"}, "pending and failing"); }
    { Retry r; r.script = {{true, false, -3}, {false, false, 0}}; expect_retry(r, true, {false}, 0, 1, {"pass defer fast fresh", "discard", "pass inline classic fresh"}, "an error beside a failing check"); }
    { Retry r; r.script = {{true, false, 0}, {false, false, -5}}; expect_retry(r, true, {false}, -5, 1, {"pass defer fast fresh", "discard", "pass inline classic fresh"}, "the classic pass's error"); }
    { Retry r; r.script = {{true, true, 0}}; expect_retry(r, true, {true}, 0, 1, {"pass defer fast fresh"}, "settled by the pass, passing"); }
    { Retry r; r.script = {{true, true, 0}, {false, false, 0}}; expect_retry(r, true, {false}, 0, 1, {"pass defer fast fresh", "discard", "pass inline classic fresh"}, "settled by the pass, failing"); }
    { Retry r; r.discard_rc = -3; r.script = {{true, false, 0}}; expect_retry(r, true, {false}, -3, 1, {"pass defer fast fresh", "discard"}, "a discard that fails"); }
}

// ---------------------------------------------------------------------------------------------- the plan's stages
struct TinyTick {  // one worker, one request with two ready tasks at one priority, `placed` of them placed on the worker
    Snap b; Arr<uint64_t> levels; Arr<uint32_t> hist;
    Table sc; hqhost::Problem pb; hqhost::Counts cnt; hqtick_config cfg{};
    std::unique_ptr<uint32_t[]> block;
    static uint32_t *storage(void *user, size_t words) { TinyTick *t = static_cast<TinyTick *>(user); t->block.reset(new uint32_t[words ? words : 1]); return t->block.get(); }
    explicit TinyTick(uint32_t placed) {
        b.s.n_workers = 1; b.s.worker_id = b.worker_id.set({3}); b.s.worker_total = b.worker_total.set({40000}); b.s.worker_free = b.worker_free.set({40000});
        std::string err;
        CHECK(validate(&b.s, true, err) == 0, "the tiny tick's snapshot: %s", err.c_str());
        cfg.proactive_filling_reserve = 0; cfg.proactive_filling_max = 2;
        fill_problem(pb, &b.s, cfg, WorkerEval{});
        sc = table_from_hist(1, levels.set({5}), hist.set({2}), 1);
        cnt.keys = {{0, 0}}; cnt.per_key = {{{0, placed}}};
    }
    hqmap::PlanIn in() {
        hqmap::PlanIn p = plan_in(sc, cnt, &b.s, pb, cfg, 2, nullptr, nullptr);
        p.storage = storage; p.user = this;
        return p;
    }
};
static void check_plan() {
    {
        TinyTick t(1);
        CHECK(t.pb.R == 1 && t.pb.rqs.size() == 1 && t.pb.rqs[0].first_variant == 0 && t.pb.rqs[0].n_variants == 1 && t.pb.variants.size() == 1 && t.pb.variants[0].n_entries == 1 &&
              t.pb.variants[0].weight == 10000 && t.pb.real.n == 1 && t.pb.real.blocked.size() == 1 && t.pb.real.rows.valid, "fill_problem");
        const hqmap::PlanIn in = t.in();
        CHECK(in.sc == &t.sc && in.cnt == &t.cnt && in.s == &t.b.s && in.rqs == t.pb.rqs.data() && in.variants == t.pb.variants.data() && in.N == 2 && in.proactive_filling_max == 2 &&
              !in.sink && in.shard_index == 0 && in.shard_count == 1 && !in.ledger_pf && in.transpose_on, "plan_in: one scheduler, no sink, no ledger");
        hqmap::Plan ps; hqmap::HostResult hr; const char *why = nullptr; std::vector<int> seen;
        const int rc = plan_stages(ps, hr, in, &why, [&](int i) { seen.push_back(i); return 0; });
        CHECK(rc == 0 && why == nullptr && seen == std::vector<int>({0, 1, 2, 3}), "the four stages, `after` behind each: rc %d, %zu calls", rc, seen.size());
        CHECK(ps.nkeys == 1 && ps.n_assign.size() == 1 && ps.n_assign[0] == 1, "the plan places one task");
    }
    for (int stop = 0; stop < 4; stop++) {  // a non-zero answer ends the sequence with that code
        TinyTick t(1);
        const hqmap::PlanIn in = t.in();
        hqmap::Plan ps; hqmap::HostResult hr; const char *why = nullptr; std::vector<int> seen;
        const int rc = plan_stages(ps, hr, in, &why, [&](int i) { seen.push_back(i); return i == stop ? -70 - i : 0; });
        CHECK(rc == -70 - stop && why == nullptr && (int)seen.size() == stop + 1 && seen.back() == stop, "`after` stops behind stage %d: rc %d, %zu calls", stop, rc, seen.size());
    }
    {   // a stage's refusal ends it with the stage's code and text, and `after` is not asked
        TinyTick t(5);  // five placed of two
        const hqmap::PlanIn in = t.in();
        hqmap::Plan ps; hqmap::HostResult hr; const char *why = nullptr; std::vector<int> seen;
        const int rc = plan_stages(ps, hr, in, &why, [&](int i) { seen.push_back(i); return 0; });
        CHECK(rc == HQTICK_E_QUEUE_UNDERFLOW && why && strstr(why, "more tasks than the queue holds") && seen.empty(), "an overdrawn queue: rc %d, %zu calls", rc, seen.size());
    }
}

// ---------------------------------------------------------------------------------------------- a query's tail
static void check_query() {
    Snap b;
    Arr<uint32_t> fake_id; Arr<uint64_t> fake_total; Arr<int64_t> fake_rem; Arr<uint8_t> fflags; Arr<uint32_t> ftmc, rtmc; Arr<uint8_t> rflags;
    hqtick_query_workers fake{};
    fake.n_workers = 2; fake.worker_id = fake_id.set({100, 101}); fake.worker_total = fake_total.set({40000, 40000}); fake.worker_remaining_ns = fake_rem.set({-1, -1});
    WorkerEval ev_real, ev_fake;
    ev_real.flags = rflags.set({7, 7}); ev_real.tmc = rtmc.set({4, 8}); ev_fake.flags = fflags.set({7, 7}); ev_fake.tmc = ftmc.set({4, 4});
    Arr<uint64_t> levels; Arr<uint32_t> hist;
    const Table sc = table_from_hist(1, levels.set({5}), hist.set({2}), 1);
    hqtick_config cfg{}; cfg.mip_time_limit_s = 2.5;
    std::vector<uint8_t> loaded{9}; hqtick_query_result out{}; std::string err = "untouched";
    g_group_calls.clear(); g_batch_calls = 0;
    int solves = 0;
    auto solve = [&](hqhost::Problem &pb, const std::vector<hqhost::TaskBatch> &batches) {
        solves++;
        CHECK(g_group_calls.size() == 2 && g_group_calls[0].ws == &pb.real && !g_group_calls[0].all_solver && g_group_calls[1].ws == pb.custom && g_group_calls[1].all_solver, "the real rows, then the fake ones as solver workers");
        CHECK(pb.custom && pb.custom->n == 2 && pb.custom->id == fake.worker_id && pb.custom->free_ == fake.worker_total && pb.custom->vflags == ev_fake.flags && pb.custom->n_variant_slots == 1, "the fake workers, fresh");
        CHECK(pb.real.n == 2 && pb.real.vflags == ev_real.flags && pb.real.vtmc == ev_real.tmc && pb.time_limit_s == 2.5, "the real workers and the config");
        CHECK(g_batch_calls == 1 && batches.size() == 1 && batches[0].rq == 0 && batches[0].size == 2, "batches from the table's runs");
        hqhost::Counts c;
        c.keys = {{0, 0}}; c.per_key = {{{1, 2}}};  // both tasks on fake worker 1
        c.is_optimal = true;
        return c;
    };
    int rc = query_tail(cfg, &b.s, &fake, ev_real, ev_fake, sc, solve, loaded, &out, err);
    CHECK(rc == 0 && solves == 1 && err == "untouched", "query_tail: rc %d", rc);
    CHECK(loaded == std::vector<uint8_t>({0, 1}) && out.n_workers == 2 && out.is_loaded == loaded.data() && out.is_optimal == 1, "worker 1 alone is loaded");
    auto refuse = [&](hqhost::Problem &, const std::vector<hqhost::TaskBatch> &) { hqhost::Counts c; c.error = HQTICK_E_UNSUPPORTED; c.errmsg = "no"; return c; };
    rc = query_tail(cfg, &b.s, &fake, ev_real, ev_fake, sc, refuse, loaded, &out, err);
    CHECK(rc == HQTICK_E_UNSUPPORTED && err == "no" && loaded == std::vector<uint8_t>({0, 1}), "a solver's error comes back with its text, the flags untouched");
}

int main() {
    check_validate();
    check_tables();
    check_export();
    check_retry();
    check_plan();
    check_query();
    printf("%ld checks ok\n", checks);
    return 0;
}
