// Host stages: batch merge, placement model, gap cache, decode (see host_model.h).
#include "host_model.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>

#include "hb_order.h"

namespace hqhost {

namespace {

// Iteration order of a Map<WorkerId,_> built from `ids` (hb_order.h), memoised on the id list: every (request, variant) key
// of one tick — and usually consecutive ticks — inserts the same workers.
// 32 entries, found by a hash of the list: a busy C4 cluster has up to 16 distinct lists per tick (one per (request, variant) key), and with the four entries this
// memo started with every tick recomputed all of them — 250 of the tick's 1 370 us.  Lives across ticks (flush_tick_caches() empties it: HQTICK_FLAG_NO_TICK_CACHES).
struct OrderEntry { uint64_t hash = 0; bool used = false; std::vector<uint32_t> ids, order; };
thread_local OrderEntry order_cache[32];
thread_local unsigned order_next = 0;
const std::vector<uint32_t> &cached_worker_order(const std::vector<uint32_t> &ids) {
    typedef OrderEntry Entry;
    Entry (&cache)[32] = order_cache;
    unsigned &next = order_next;
    uint64_t h = 0x9E3779B97F4A7C15ull ^ ids.size();
    for (uint32_t v : ids) { h ^= v; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 29; }
    for (Entry &e : cache) if (e.used && e.hash == h && e.ids.size() == ids.size() && (ids.empty() || memcmp(e.ids.data(), ids.data(), ids.size() * 4) == 0)) return e.order;
    Entry &e = cache[next++ & 31];
    e.hash = h; e.ids = ids; e.used = true;
    hqhb::insertion_order_u32(ids.data(), (uint32_t)ids.size(), e.order);
    return e.order;
}

double clock_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const double FRACTIONS = 10000.0;
inline double units(uint64_t a) { return (double)a / FRACTIONS; }  // ResourceAmount::as_f64  amount.rs:91-93

// prune_progressive  scheduler/batches.rs:183-217: keep `prefix` cuts, sample the rest quadratically
void prune_cuts(std::vector<PriorityCut> &cuts, size_t prefix, size_t limit) {
    size_t n = cuts.size();
    if (n <= limit) return;
    std::vector<size_t> pick;
    for (size_t i = 0; i < prefix; i++) pick.push_back(i);
    size_t slots = limit - prefix, pool = n - prefix, prev = prefix - 1;
    for (size_t i = 0; i < slots; i++) {
        double t = (double)i / (double)(slots - 1);
        size_t idx = prefix + (size_t)std::round(t * t * (double)(pool - 1));
        if (idx <= prev) idx = prev + 1;
        pick.push_back(idx);
        prev = idx;
    }
    std::vector<PriorityCut> kept;
    kept.reserve(limit);
    for (size_t i = 0; i < limit; i++) kept.push_back(std::move(cuts[pick[i]]));  // pick is strictly increasing: same result as the in-place swaps
    cuts.swap(kept);
}

}  // namespace

void flush_tick_caches() { for (OrderEntry &e : order_cache) e.used = false; }

// ---------------------------------------------------------------------------------------------------------------
// workers with identical rows (host_model.h, WorkerGroups)
// ---------------------------------------------------------------------------------------------------------------
void group_equal_rows(WorkerSet &ws, bool all_solver) {
    WorkerGroups &g = ws.rows;
    const uint32_t n = ws.n, R = ws.R;
    g.of.resize(n); g.rep.clear(); g.count.clear();
    static thread_local std::vector<uint32_t> table;
    size_t cap = 64; while (cap < 2 * (size_t)n + 2) cap <<= 1;
    bool table_ready = false;  // the open-addressing table is only needed once two neighbours differ
    auto same = [&](uint32_t a, uint32_t b) {
        if (ws.remaining_ns && ws.remaining_ns[a] != ws.remaining_ns[b]) return false;
        if (ws.flags && ws.flags[a] != ws.flags[b]) return false;
        if (ws.min_util && memcmp(ws.min_util + a, ws.min_util + b, 4) != 0) return false;
        const uint64_t *fa = ws.free_ + (size_t)a * R, *fb = ws.free_ + (size_t)b * R, *ta = ws.total + (size_t)a * R, *tb = ws.total + (size_t)b * R;
        uint64_t diff = 0;
        for (uint32_t r = 0; r < R; r++) diff |= (fa[r] ^ fb[r]) | (ta[r] ^ tb[r]);  // a handful of words: no call, no branch
        return diff == 0;
    };
    auto hash_row = [&](uint32_t w) {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        auto mix = [&](uint64_t v) { h ^= v; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 32; };
        for (uint32_t r = 0; r < R; r++) { mix(ws.total[(size_t)w * R + r]); mix(ws.free_[(size_t)w * R + r]); }
        if (ws.remaining_ns) mix((uint64_t)ws.remaining_ns[w]);
        if (ws.min_util) { uint32_t b; memcpy(&b, ws.min_util + w, 4); mix(b); }
        if (ws.flags) mix(ws.flags[w]);
        return h;
    };
    long prev = -1;  // previous worker without a blocked request: neighbours usually agree
    for (uint32_t w = 0; w < n; w++) {
        if (!ws.blocked.empty() && !ws.blocked[w].empty()) {  // a blocked (request, variant) changes the worker's eligibility: a group of its own
            g.of[w] = (uint32_t)g.rep.size(); g.rep.push_back(w); g.count.push_back(1);
            continue;
        }
        if (prev >= 0 && same(w, (uint32_t)prev)) { const uint32_t id = g.of[prev]; g.of[w] = id; g.count[id]++; prev = w; continue; }
        if (!table_ready) {
            table.assign(cap, UINT32_MAX); table_ready = true;
            if (prev >= 0) table[(size_t)hash_row((uint32_t)prev) & (cap - 1)] = g.of[prev];  // everything so far is one group (or blocked singletons)
        }
        prev = w;
        size_t slot = (size_t)hash_row(w) & (cap - 1);
        uint32_t id = UINT32_MAX;
        while (table[slot] != UINT32_MAX) {
            if (same(w, g.rep[table[slot]])) { id = table[slot]; break; }
            slot = (slot + 1) & (cap - 1);
        }
        if (id == UINT32_MAX) { id = (uint32_t)g.rep.size(); table[slot] = id; g.rep.push_back(w); g.count.push_back(0); }
        g.of[w] = id; g.count[id]++;
    }
    g.solver_workers.clear(); g.solver_workers.reserve(n);
    for (uint32_t w = 0; w < n; w++) if (all_solver || ws.is_sn(w)) g.solver_workers.push_back(w);
    g.pool.assign(R, 0.0);
    for (uint32_t w : g.solver_workers) for (uint32_t r = 0; r < R; r++) { const uint64_t c = ws.free_[(size_t)w * R + r]; g.pool[r] += c == HQ_AMOUNT_MAX ? 1.0 : units(c); }
    g.valid = true;
}

// ---------------------------------------------------------------------------------------------------------------
// create_task_batches  scheduler/batches.rs:42-181
// ---------------------------------------------------------------------------------------------------------------
const BlockMemo::Entry *BlockMemo::find(const hqmilp::Model &m) {
    auto &k = scratch; k.clear();
    auto put_bytes = [&](const void *p, size_t n) { const unsigned char *b = static_cast<const unsigned char *>(p); k.insert(k.end(), b, b + n); };
    auto put_vec = [&](const auto &v) { const uint64_t n = v.size(); put_bytes(&n, 8); if (n) put_bytes(v.data(), n * sizeof(v[0])); };
    put_vec(m.obj); put_vec(m.kind); put_vec(m.rtype); put_vec(m.rhs); put_vec(m.roff); put_vec(m.rcol); put_vec(m.rcoef); put_vec(m.start); put_vec(m.col_group); put_vec(m.row_implied);
    uint64_t h = 0x9E3779B97F4A7C15ull;
    size_t i = 0;
    for (; i + 8 <= k.size(); i += 8) { uint64_t w; memcpy(&w, k.data() + i, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    for (; i < k.size(); i++) { h = (h ^ k[i]) * 0x100000001B3ull; }
    scratch_hash = h;
    for (const Entry &e : entries) if (e.hash == h && e.key.size() == k.size() && memcmp(e.key.data(), k.data(), k.size()) == 0) return &e;
    return nullptr;
}

void BlockMemo::put(const hqmilp::Result &r) {
    const size_t slot = entries.size() < CAP ? (entries.emplace_back(), entries.size() - 1) : (next++ % CAP);   // (the index before the table is full: its last slot too)
    Entry &e = entries[slot];
    e.hash = scratch_hash; e.key = scratch; e.x = r.x; e.nodes = r.nodes; e.n_components = r.n_components;
}

std::vector<TaskBatch> create_task_batches(const Problem &pb, const std::vector<QueueLevels> &queues) {
    std::vector<uint32_t> live;  // non-empty queues, in rq order
    for (uint32_t q = 0; q < queues.size(); q++) if (!queues[q].levels.empty()) live.push_back(q);
    std::vector<TaskBatch> batches(live.size());
    if (live.empty()) return batches;
    const WorkerSet &lim_ws = pb.custom ? *pb.custom : pb.real;
    // limits  :65-92.  Single-node requests: one pass over the workers (K2's per-(worker, variant) rows are worker-major: the rq-major loop of the
    // reference walks them with a stride of one row per step), accumulating every live request's limit at once.
    std::vector<uint32_t> sn_limit(live.size(), 0);
    {
        std::vector<uint32_t> sn_b;  // live single-node requests
        for (size_t b = 0; b < live.size(); b++) if (!pb.rq_multi_node(live[b])) sn_b.push_back((uint32_t)b);
        auto add_worker = [&](uint32_t w, uint32_t times) {  // `times` workers with the rows of w
            const bool sn = lim_ws.is_sn(w);
            for (uint32_t b : sn_b) {
                const uint32_t rq = live[b];
                if (!pb.capable_rqv(lim_ws, w, rq)) continue;
                uint32_t runnable = 0;
                if (sn) for (uint32_t v = 0; v < pb.rqs[rq].n_variants; v++) runnable += lim_ws.tmc(w, pb.rqs[rq].first_variant + v);
                sn_limit[b] += (runnable > 0 ? runnable : 1) * times;  // u32 arithmetic wraps like the repeated addition would
            }
        };
        if (sn_b.empty()) {}
        else if (lim_ws.rows.valid) for (size_t g = 0; g < lim_ws.rows.rep.size(); g++) add_worker(lim_ws.rows.rep[g], lim_ws.rows.count[g]);
        else for (uint32_t w = 0; w < lim_ws.n; w++) add_worker(w, 1);
    }
    for (size_t b = 0; b < live.size(); b++) {
        uint32_t rq = live[b];
        uint32_t limit = sn_limit[b];
        if (pb.rq_multi_node(rq)) {  // :65-78
            uint32_t frees = 0;
            for (uint32_t w = 0; w < pb.real.n; w++) frees += pb.real.is_free(w) ? 1 : 0;
            limit = frees / pb.variants[pb.rqs[rq].first_variant].n_nodes;
        }
        batches[b].rq = rq;
        batches[b].limit = limit;
    }
    // k-way merge of the queues' (priority, size) streams  :97-171
    size_t nb = live.size();
    std::vector<size_t> cursor(nb, 0);
    std::vector<char> open(nb, 1);
    auto cur_prio = [&](size_t b) { return queues[live[b]].levels[cursor[b]].first; };
    auto absorb = [&](size_t b) {
        TaskBatch &tb = batches[b];
        tb.size += queues[live[b]].levels[cursor[b]].second;
        if (tb.size > tb.limit) { tb.size = tb.limit; tb.limit_reached = true; open[b] = 0; }
        else if (++cursor[b] >= queues[live[b]].levels.size()) open[b] = 0;
    };
    long last_single = -1;
    std::vector<size_t> top;
    for (;;) {
        top.clear();
        uint64_t best = 0;
        for (size_t b = 0; b < nb; b++) {
            if (!open[b]) continue;
            uint64_t p = cur_prio(b);
            if (p > best) { best = p; top.clear(); top.push_back(b); }
            else if (p == best) top.push_back(b);
        }
        if (top.empty()) break;
        if (top.size() == 1 && last_single == (long)top[0]) { absorb(top[0]); continue; }
        for (size_t b : top) {
            PriorityCut cut;
            cut.size = batches[b].size;
            for (size_t o = 0; o < nb; o++) {
                if (o == b) continue;
                TaskBatch &ob = batches[o];
                if (ob.size > 0 || ob.limit_reached) {
                    ob.is_blocker = true;
                    cut.blockers.push_back({ob.rq, ob.limit_reached ? HQ_BLOCKER_UNBOUNDED : ob.size});
                }
            }
            if (!cut.blockers.empty()) batches[b].cuts.push_back(std::move(cut));
        }
        for (size_t b : top) absorb(b);
        last_single = top.size() == 1 ? (long)top[0] : -1;
    }
    std::vector<TaskBatch> out;
    for (auto &tb : batches) {
        prune_cuts(tb.cuts, 4, 32);
        if (tb.size > 0) out.push_back(std::move(tb));
    }
    return out;
}

// ---------------------------------------------------------------------------------------------------------------
// gap  scheduler/gap.rs
// ---------------------------------------------------------------------------------------------------------------
namespace {

struct Amounts {
    std::vector<uint64_t> a;
    uint64_t get(uint32_t r) const { return r < a.size() ? a[r] : 0; }
};

uint32_t max_count(const Amounts &have, const VariantView &rq) {  // task_max_count_for_request  workerload.rs:121-145
    bool any = false; uint64_t best = 0;
    for (uint32_t e = 0; e < rq.n_entries; e++) {
        uint64_t c = rq.kind[e] == HQ_ENTRY_ALL ? (have.get(rq.res[e]) ? 1 : 0) : std::min<uint64_t>(have.get(rq.res[e]) / rq.amount[e], HQ_MAX_TASK_PER_WORKER);
        if (!any || c < best) best = c;
        any = true;
    }
    return any ? (uint32_t)best : 0;
}
// the same two on a worker's row of R amounts where it lies (every resource index of a validated snapshot is below R): no vector per (blocker, worker) pair
inline uint32_t max_count_row(const uint64_t *have, uint32_t R, const VariantView &rq) {
    bool any = false; uint64_t best = 0;
    for (uint32_t e = 0; e < rq.n_entries; e++) {
        const uint64_t h = rq.res[e] < R ? have[rq.res[e]] : 0;
        const uint64_t c = rq.kind[e] == HQ_ENTRY_ALL ? (h ? 1 : 0) : std::min<uint64_t>(h / rq.amount[e], HQ_MAX_TASK_PER_WORKER);
        if (!any || c < best) best = c;
        any = true;
    }
    return any ? (uint32_t)best : 0;
}
inline void take_away_row(uint64_t *have, uint32_t R, const VariantView &rq, uint64_t times) {
    for (uint32_t e = 0; e < rq.n_entries; e++) {
        const uint32_t r = rq.res[e];
        if (r >= R) continue;
        if (rq.kind[e] == HQ_ENTRY_ALL) have[r] = 0;
        else { const uint64_t d = rq.amount[e] * times; have[r] = have[r] > d ? have[r] - d : 0; }
    }
}
void take_away(Amounts &have, const VariantView &rq, uint64_t times) {  // remove / remove_multiple  workerload.rs:156-177
    for (uint32_t e = 0; e < rq.n_entries; e++) {
        uint32_t r = rq.res[e];
        if (r >= have.a.size()) have.a.resize(r + 1, 0);
        if (rq.kind[e] == HQ_ENTRY_ALL) have.a[r] = 0;
        else { uint64_t d = rq.amount[e] * times; have.a[r] = have.a[r] > d ? have.a[r] - d : 0; }
    }
}

struct GapCache {
    std::map<std::pair<uint32_t, std::vector<uint64_t>>, Amounts> memo;  // (rq, WorkerResources) -> leftover   gap.rs:14-35
    const Problem &pb;
    explicit GapCache(const Problem &p) : pb(p) {}

    // compute_gap_resources  gap.rs:95-147: per non-zero resource, how much of it the blocker's variants can use at most
    Amounts leftover_multi_variant(uint32_t rq, const Amounts &total) {
        const RequestView &rv = pb.rqs[rq];
        long top = -1;
        for (uint32_t v = 0; v < rv.n_variants; v++) { const VariantView &vv = pb.variants[rv.first_variant + v]; for (uint32_t e = 0; e < vv.n_entries; e++) top = std::max<long>(top, vv.res[e]); }
        Amounts out;
        if (top < 0) return out;
        for (uint32_t r = 0; r < total.a.size(); r++) {
            uint64_t have = total.a[r];
            if (have == 0) continue;  // iter_pairs skips zero amounts; the result keeps one slot per visited pair
            hqmilp::Model m;
            for (uint32_t v = 0; v < rv.n_variants; v++) {
                const VariantView &vv = pb.variants[rv.first_variant + v];
                double w = 0.0;
                for (uint32_t e = 0; e < vv.n_entries; e++) if (vv.res[e] == r) w = vv.kind[e] == HQ_ENTRY_ALL ? units(total.get(r)) : units(vv.amount[e]);
                m.add_col(w, hqmilp::COL_NAT);
            }
            for (long rr = 0; rr <= top; rr++) {
                m.begin_row(hqmilp::ROW_MAX, units(total.get((uint32_t)rr)));
                for (uint32_t v = 0; v < rv.n_variants; v++) {
                    const VariantView &vv = pb.variants[rv.first_variant + v];
                    for (uint32_t e = 0; e < vv.n_entries; e++) if (vv.res[e] == (uint32_t)rr) m.term((int)v, vv.kind[e] == HQ_ENTRY_ALL ? units(total.get(r)) : units(vv.amount[e]));
                }
                m.end_row();
            }
            hqmilp::Result s = hqmilp::solve(m, 1e9, false);
            if (!s.feasible || !s.optimal) { out.a.push_back(0); continue; }
            uint64_t used = (uint64_t)std::ceil((float)std::round(s.objective) * 10000.0f);  // ResourceAmount::from_float(v.round() as f32)
            out.a.push_back(have - used);
        }
        return out;
    }

    // What the blocker leaves of a worker (gap.rs:44-84): the worker's total minus as many blocker tasks as fit, minus what runs there (other requests only).
    // asg_cnt (optional): the running tasks given as DISTINCT (rq, variant) pairs with their multiplicities — saturating subtractions commute, so
    // taking a pair away `count` times at once is the same as the reference's one-by-one loop (gap.rs:79-84).  false: the gap is 0 whatever the batch.
    bool leftover(uint32_t high_rq, const Amounts &total, const uint32_t *asg_rq, const uint8_t *asg_variant, uint32_t n_asg, const uint32_t *asg_cnt, Amounts &left) {
        if (pb.rq_multi_node(high_rq)) return false;
        const RequestView &h = pb.rqs[high_rq];
        if (h.n_variants == 1) {
            const VariantView &hv = pb.variants[h.first_variant];
            for (uint32_t e = 0; e < hv.n_entries; e++) if (hv.kind[e] == HQ_ENTRY_ALL) return false;
            left = total;
            take_away(left, hv, max_count(total, hv));
        } else {
            auto key = std::make_pair(high_rq, total.a);
            auto it = memo.find(key);
            if (it == memo.end()) it = memo.emplace(key, leftover_multi_variant(high_rq, total)).first;
            left = it->second;
        }
        for (uint32_t i = 0; i < n_asg; i++) if (asg_rq[i] != high_rq) take_away(left, pb.variants[pb.rqs[asg_rq[i]].first_variant + asg_variant[i]], asg_cnt ? asg_cnt[i] : 1);
        return true;
    }
    // the common blocker — one variant, no `all` entry — on the worker's row itself: true and the leftover in left[0..R), or false: not this shape (the caller takes
    // leftover() above, which also knows the gap-is-0 rules)
    bool leftover_row(uint32_t high_rq, const uint64_t *total, uint32_t R, const uint32_t *asg_rq, const uint8_t *asg_variant, uint32_t n_asg, const uint32_t *asg_cnt, uint64_t *left) {
        if (pb.rq_multi_node(high_rq)) return false;
        const RequestView &h = pb.rqs[high_rq];
        if (h.n_variants != 1) return false;
        const VariantView &hv = pb.variants[h.first_variant];
        for (uint32_t e = 0; e < hv.n_entries; e++) if (hv.kind[e] == HQ_ENTRY_ALL || hv.res[e] >= R) return false;
        for (uint32_t r = 0; r < R; r++) left[r] = total[r];
        take_away_row(left, R, hv, max_count_row(total, R, hv));
        for (uint32_t i = 0; i < n_asg; i++) if (asg_rq[i] != high_rq) take_away_row(left, R, pb.variants[pb.rqs[asg_rq[i]].first_variant + asg_variant[i]], asg_cnt ? asg_cnt[i] : 1);
        return true;
    }
    uint32_t fit_row(uint32_t low_rq, const uint64_t *left, uint32_t R) {
        if (pb.rq_multi_node(low_rq)) return 0;
        const RequestView &l = pb.rqs[low_rq];
        uint32_t best = 0;
        for (uint32_t v = 0; v < l.n_variants; v++) { const uint32_t c = max_count_row(left, R, pb.variants[l.first_variant + v]); if (v == 0 || c < best) best = c; }
        return best;
    }
    // how many tasks of the batch fit into what is left (gap.rs:86-92)
    uint32_t fit(uint32_t low_rq, const Amounts &left) {
        if (pb.rq_multi_node(low_rq)) return 0;
        const RequestView &l = pb.rqs[low_rq];
        uint32_t best = 0;
        for (uint32_t v = 0; v < l.n_variants; v++) { uint32_t c = max_count(left, pb.variants[l.first_variant + v]); if (v == 0 || c < best) best = c; }
        return best;
    }
    uint32_t gap(uint32_t high_rq, uint32_t low_rq, const Amounts &total, const uint32_t *asg_rq, const uint8_t *asg_variant, uint32_t n_asg, const uint32_t *asg_cnt = nullptr) {
        if (pb.rq_multi_node(high_rq) || pb.rq_multi_node(low_rq)) return 0;
        Amounts left;
        if (!leftover(high_rq, total, asg_rq, asg_variant, n_asg, asg_cnt, left)) return 0;
        return fit(low_rq, left);
    }
};

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// run_scheduling_solver  scheduler/solver.rs:36-483
// ---------------------------------------------------------------------------------------------------------------
Counts run_scheduling_solver(const Problem &pb, const std::vector<TaskBatch> &batches) {
    Counts out;
    const double t_enter = clock_us();
    if (pb.rqs.empty()) return out;  // :53-55
    const WorkerSet &ws = pb.custom ? *pb.custom : pb.real;
    const uint32_t R = pb.R;
    std::vector<uint32_t> own_workers; std::vector<double> own_pool;
    if (!ws.rows.valid) {  // (the tick forms these while the GPU runs phase A: group_equal_rows)
        for (uint32_t w = 0; w < ws.n; w++) if (pb.custom || ws.is_sn(w)) own_workers.push_back(w);
        own_pool.assign(R, 0.0);
        for (uint32_t w : own_workers) for (uint32_t r = 0; r < R; r++) { uint64_t c = ws.free_[(size_t)w * R + r]; own_pool[r] += c == HQ_AMOUNT_MAX ? 1.0 : units(c); }
    }
    const std::vector<uint32_t> &solver_workers = ws.rows.valid ? ws.rows.solver_workers : own_workers;  // SN workers, ascending id (the worker arrays are already sorted)  :57-66
    const size_t nw = solver_workers.size();
    const std::vector<double> &pool = ws.rows.valid ? ws.rows.pool : own_pool;  // resource_sums  :56,68-82

    auto is_blocked = [&](uint32_t w, uint32_t rq, uint8_t v) {
        if (pb.custom) return false;
        for (auto &b : ws.blocked[w]) if (b.first == rq && b.second == v) return true;
        return false;
    };

    // ---- separable instances: no multi-node batch, no priority cut ------------------------------------------------
    // Then the only rows of solver.rs:95-271 that span two workers are the batch-size rows `sum_w x <= size_b` of the batches that are
    // not saturated.  Without them the model is one independent block per worker, and workers with the same (free, total,
    // eligibility, min_utilization) have the same block up to the positive factor (W - idx)/W of the objective: solve one block per
    // such worker class instead of building W of them.  The size rows are treated as lazy constraints: if the block optima respect
    // them, that point is optimal for the full model too (it is optimal for a relaxation and feasible) and it is the canonical one
    // (the optimal set of the full model is the product of the block-optimal sets cut by the size rows; the per-block lexicographic
    // minima form the lexicographic minimum of the product, hence of any subset that contains it).  If a size row is violated the
    // general path below takes over.
    struct SeqStart { uint32_t w, batch; uint8_t variant; uint32_t count; };
    std::vector<SeqStart> seq_start;  // starting point handed to the coupled solve when the lazy size rows fail
    // Per worker: the integer optimum of its OWN block (its resource rows alone) in base costs, known when the tick went through the separable section first.
    // The coupled model gets one row per worker from it, "this worker's part of the objective cannot exceed what the worker can hold": the LP of a bin-packing-like
    // tick (a 7-cpu worker, requests of 2 / 3 / 5 cpus that also compete for 2 gpus) fills every worker fractionally to 100 % and sits 20 % above the optimum.
    std::vector<double> block_z;
    std::vector<uint8_t> worker_off;  // workers that are empty in EVERY optimum of the coupled model (see below): their columns are not created
    bool separable = true;
    for (const TaskBatch &b : batches) if (pb.rq_multi_node(b.rq) || !b.cuts.empty() || b.is_blocker) separable = false;
    if (separable && !batches.empty()) {
        struct ColRef { uint32_t batch; uint8_t variant; };
        const double t_sep0 = clock_us();
        const size_t nb = batches.size();
        // the tick's (batch, variant) columns, in the order of solver.rs:95-192: column g of batch b, variant v is voff[b] + v
        std::vector<uint32_t> voff(nb + 1, 0);
        for (size_t b = 0; b < nb; b++) voff[b + 1] = voff[b] + pb.rqs[batches[b].rq].n_variants;
        const uint32_t NC = voff[nb];
        std::vector<uint32_t> col_slot(NC), col_rq(NC), col_batch(NC); std::vector<uint8_t> col_v(NC);
        for (size_t b = 0; b < nb; b++) {
            const RequestView &rv = pb.rqs[batches[b].rq];
            for (uint8_t v = 0; v < rv.n_variants; v++) { const uint32_t g = voff[b] + v; col_slot[g] = rv.first_variant + v; col_rq[g] = batches[b].rq; col_batch[g] = (uint32_t)b; col_v[g] = v; }
        }
        // ---- worker classes: same (total, free, min_utilization, eligibility bits) => same block ----
        const uint32_t EW = (NC + 63) / 64, SW = 2 * R + 1 + EW;  // signature words
        std::vector<uint64_t> sigs; std::vector<uint32_t> rep;     // per class: signature, first worker
        std::vector<uint32_t> wclass(ws.n, 0);
        std::vector<uint64_t> n_in_class;                          // solver workers per class
        {
            size_t cap = 64; while (cap < 2 * nw + 2) cap <<= 1;
            std::vector<uint32_t> table(cap, UINT32_MAX);
            std::vector<uint64_t> tmp(SW);
            { const size_t expect = ws.rows.valid ? ws.rows.rep.size() : 64; sigs.reserve(expect * SW); rep.reserve(expect); n_in_class.reserve(expect); }
            // class of the workers whose rows equal those of w: signature from w's rows and K2's answer for w
            auto class_of = [&](uint32_t w) {
                const uint64_t *tot = ws.total + (size_t)w * R, *fre = ws.free_ + (size_t)w * R;
                const float mu = ws.min_util ? ws.min_util[w] : 0.0f;
                memcpy(tmp.data(), tot, (size_t)R * 8); memcpy(tmp.data() + R, fre, (size_t)R * 8);
                uint32_t mubits; memcpy(&mubits, &mu, 4); tmp[2 * R] = mubits;
                for (uint32_t e = 0; e < EW; e++) tmp[2 * R + 1 + e] = 0;
                const bool any_blocked = !pb.custom && !ws.blocked[w].empty();
                for (uint32_t g = 0; g < NC; g++) {
                    const uint8_t f = ws.vf(w, col_slot[g]);
                    if ((f & 4) && (f & 1) && !(any_blocked && is_blocked(w, col_rq[g], col_v[g]))) tmp[2 * R + 1 + g / 64] |= 1ull << (g % 64);
                }
                uint64_t h = 0x9E3779B97F4A7C15ull;
                for (uint32_t i = 0; i < SW; i++) { h ^= tmp[i]; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
                size_t slot = (size_t)h & (cap - 1);
                uint32_t cid = UINT32_MAX;
                while (table[slot] != UINT32_MAX) {
                    if (memcmp(sigs.data() + (size_t)table[slot] * SW, tmp.data(), (size_t)SW * 8) == 0) { cid = table[slot]; break; }
                    slot = (slot + 1) & (cap - 1);
                }
                if (cid == UINT32_MAX) { cid = (uint32_t)rep.size(); table[slot] = cid; rep.push_back(w); n_in_class.push_back(0); sigs.insert(sigs.end(), tmp.begin(), tmp.end()); }
                return cid;
            };
            if (ws.rows.valid) {  // one signature per group of workers with equal rows (formed while the GPU ran phase A); groups come in the order of their first worker,
                                  // so the classes are numbered as a pass over the workers would number them
                const WorkerGroups &gr = ws.rows;
                std::vector<uint32_t> gclass(gr.rep.size(), UINT32_MAX);
                for (size_t g = 0; g < gr.rep.size(); g++) {
                    if (!(pb.custom || ws.is_sn(gr.rep[g]))) continue;  // the flags byte is part of the group key: all of the group or none
                    gclass[g] = class_of(gr.rep[g]); n_in_class[gclass[g]] += gr.count[g];
                }
                for (uint32_t w : solver_workers) wclass[w] = gclass[gr.of[w]];
            } else {
                for (uint32_t w : solver_workers) { wclass[w] = class_of(w); n_in_class[wclass[w]]++; }
            }
        }
        const uint32_t ncls = (uint32_t)rep.size();
        const double t_sep1 = clock_us();
        auto elig = [&](uint32_t c, uint32_t g) { return (sigs[(size_t)c * SW + 2 * R + 1 + g / 64] >> (g % 64)) & 1; };
        auto class_mu_flag = [&](uint32_t c) {  // does add_min_utilization create its on/off column?  solver.rs:501-521
            const uint32_t w = rep[c];
            const float mu = ws.min_util ? ws.min_util[w] : 0.0f;
            const uint64_t *tot = ws.total + (size_t)w * R, *fre = ws.free_ + (size_t)w * R;
            if (!(mu > 0.001f && tot[0] != HQ_AMOUNT_MAX)) return false;
            const double need = units(tot[0]) * ((double)mu - 1.0) + units(fre[0]);
            return !(need < 0.0001);
        };
        // the block of one class as a model for the exact host solver: columns and rows in the order of solver.rs:95-192
        auto build_class_model = [&](uint32_t c, hqmilp::Model &m, std::vector<ColRef> &cols) {
            const uint32_t w = rep[c];
            const uint64_t *tot = ws.total + (size_t)w * R, *fre = ws.free_ + (size_t)w * R;
            const float mu = ws.min_util ? ws.min_util[w] : 0.0f;
            std::vector<std::vector<std::pair<int, double>>> rt(R);
            std::vector<std::pair<int, double>> cpu;
            for (uint32_t g = 0; g < NC; g++) {
                if (!elig(c, g)) continue;
                const VariantView &vv = pb.variants[col_slot[g]];
                double sc = 0.0;
                for (uint32_t e = 0; e < vv.n_entries; e++) {
                    double gp = pool[vv.res[e]];
                    sc += gp < 0.000001 ? 0.0 : units(vv.kind[e] == HQ_ENTRY_ALL ? tot[vv.res[e]] : vv.amount[e]) / gp;
                }
                int col = m.add_col(sc * ((double)vv.weight / FRACTIONS), hqmilp::COL_NAT);
                cols.push_back({col_batch[g], col_v[g]});
                for (uint32_t e = 0; e < vv.n_entries; e++) {
                    double a = units(vv.kind[e] == HQ_ENTRY_ALL ? tot[vv.res[e]] : vv.amount[e]);
                    rt[vv.res[e]].push_back({col, a});
                    if (vv.res[e] == 0) cpu.push_back({col, a});
                }
            }
            if (class_mu_flag(c)) {
                const double all_cpus = units(tot[0]), need = all_cpus * ((double)mu - 1.0) + units(fre[0]);
                int col = m.add_col(0.0, hqmilp::COL_BOOL);
                cols.push_back({UINT32_MAX, 0});
                cpu.push_back({col, -need}); m.begin_row(hqmilp::ROW_MIN, 0.0); for (auto &t : cpu) m.term(t.first, t.second); m.end_row(); cpu.pop_back();
                cpu.push_back({col, -all_cpus}); m.begin_row(hqmilp::ROW_MAX, 0.0); for (auto &t : cpu) m.term(t.first, t.second); m.end_row(); cpu.pop_back();
            }
            for (uint32_t r = 0; r < R; r++) {
                if (fre[r] == HQ_AMOUNT_MAX) continue;
                if (!rt[r].empty()) { m.begin_row(hqmilp::ROW_MAX, units(fre[r])); for (auto &t : rt[r]) m.term(t.first, t.second); m.end_row(); }
            }
        };
        // MAX-amount rows leak into the next worker in the reference (solver.rs:183-185): such a tick takes the general path
        for (uint32_t c = 0; c < ncls && separable; c++) {
            const uint64_t *fre = ws.free_ + (size_t)rep[c] * R;
            bool any_max = false;
            for (uint32_t r = 0; r < R; r++) if (fre[r] == HQ_AMOUNT_MAX) any_max = true;
            if (!any_max) continue;
            for (uint32_t g = 0; g < NC && separable; g++) {
                if (!elig(c, g)) continue;
                const VariantView &vv = pb.variants[col_slot[g]];
                for (uint32_t e = 0; e < vv.n_entries; e++) if (fre[vv.res[e]] == HQ_AMOUNT_MAX) separable = false;
            }
        }
        // ---- solve one block per class: on the device (one wavefront per class, csrc/block_core.h) where the block qualifies, else here ----
        std::vector<uint32_t> X((size_t)ncls * NC, 0);  // canonical optimum of every class, by tick column
        std::vector<uint8_t> solved(ncls, 0), class_has_flag(ncls, 0);
        bool blocks_exact = true;  // every class block solved to its EXACT optimum (device blocks are; a host block that came back with a gap certificate only is not)
        if (separable) {
            for (uint32_t c = 0; c < ncls; c++) class_has_flag[c] = class_mu_flag(c) ? 1 : 0;
            // one class block through the host's exact solver; -1: infeasible (the reference's `None`)
            auto solve_class_on_host = [&](uint32_t c) -> int {
                hqmilp::Model m; std::vector<ColRef> cols;
                build_class_model(c, m, cols);
                out.blocks_host++; out.milp_cols += m.ncols(); out.milp_rows += m.nrows();
                if (const BlockMemo::Entry *hit = pb.memo ? pb.memo->find(m) : nullptr) {  // this very block, solved to its canonical optimum by an earlier tick
                    out.blocks_memo++; out.milp_nodes += hit->nodes; out.milp_components += hit->n_components;
                    for (size_t k = 0; k < cols.size(); k++) if (cols[k].batch != UINT32_MAX) X[(size_t)c * NC + voff[cols[k].batch] + cols[k].variant] = (uint32_t)std::round(hit->x[k]);
                    solved[c] = 1;
                    return 0;
                }
                hqmilp::Result sol = hqmilp::solve(m, pb.time_limit_s, true);
                out.milp_nodes += sol.nodes; out.milp_components += sol.n_components;
                if (pb.memo && sol.feasible && sol.optimal && sol.canonical) pb.memo->put(sol);
                if (!sol.feasible) return -1;
                if (!sol.optimal) out.is_optimal = false;
                if (!sol.canonical) { out.is_canonical = false; blocks_exact = false; }  // certificate only: the incumbent may sit up to rel_gap below the block's optimum
                for (size_t k = 0; k < cols.size(); k++) if (cols[k].batch != UINT32_MAX) X[(size_t)c * NC + voff[cols[k].batch] + cols[k].variant] = (uint32_t)std::round(sol.x[k]);
                solved[c] = 1;
                return 0;
            };
            std::vector<uint32_t> dev_cls;
            if (pb.blocks && NC <= (uint32_t)hqblock::GCOLS) for (uint32_t c = 0; c < ncls; c++) if (!class_has_flag[c]) dev_cls.push_back(c);
            if (pb.blocks && dev_cls.size() >= pb.block_min_classes) {
                std::vector<uint32_t> ent_off(NC + 1, 0), ent_res, weight(NC); std::vector<uint8_t> ent_kind; std::vector<uint64_t> ent_amount;
                for (uint32_t g = 0; g < NC; g++) {
                    const VariantView &vv = pb.variants[col_slot[g]];
                    for (uint32_t e = 0; e < vv.n_entries; e++) { ent_res.push_back(vv.res[e]); ent_kind.push_back(vv.kind[e]); ent_amount.push_back(vv.amount[e]); }
                    ent_off[g + 1] = (uint32_t)ent_res.size(); weight[g] = vv.weight;
                }
                uint32_t nd = (uint32_t)dev_cls.size();
                std::vector<uint32_t> held;  // classes the host solves itself while the kernel runs (below)
                if (nd > 1024) {
                    // The launch's span is its start spread (more classes than the 1024 blocks the chip holds at once: a busy C4 cluster has ~3000) plus its slowest block,
                    // and the slow blocks are the classes with the most room (the more fits, the deeper the search).  Longest first: classes by descending free share of
                    // resource 0, a 256-bucket counting sort (stable: equal shares keep their order) — k_block_solve 824 -> 620 us on the 3050-class C4 steady state.
                    // And the very hardest ones are not launched at all: the host solves them with its own solver WHILE the kernel runs — a wavefront takes 400-600 us
                    // for what the host does in tens (tools/block_profile.py: the 16 slowest classes of that launch are its first 16 in this order).
                    static const bool ordered = !(getenv("HQTICK_BLOCK_ORDER") && atoi(getenv("HQTICK_BLOCK_ORDER")) == 0);
                    if (ordered) {
                        std::vector<uint32_t> cnt(257, 0), sorted_cls(nd); std::vector<uint8_t> bk(nd);
                        for (uint32_t i = 0; i < nd; i++) {
                            const uint64_t *tot = sigs.data() + (size_t)dev_cls[i] * SW, *fre = tot + R;
                            const uint64_t t0 = tot[0], f0 = fre[0] < t0 ? fre[0] : t0;
                            bk[i] = (t0 && t0 != HQ_AMOUNT_MAX) ? (uint8_t)(255 - (uint32_t)((unsigned __int128)f0 * 255 / t0)) : (uint8_t)255;  // bucket 0 = everything free
                            cnt[bk[i] + 1]++;
                        }
                        for (int b = 0; b < 256; b++) cnt[b + 1] += cnt[b];
                        for (uint32_t i = 0; i < nd; i++) sorted_cls[cnt[bk[i]]++] = dev_cls[i];
                        dev_cls.swap(sorted_cls);
                        static const int hold = getenv("HQTICK_BLOCK_HOLD") ? atoi(getenv("HQTICK_BLOCK_HOLD")) : 24;  // (3050-class C4 steady state: 0 -> 619 us kernel / 1.53 ms tick, 16 -> 491 / 1.42, 32 -> 467 / 1.40;
                                                                                                                      // on a 929-class c3 launch, all resident, the order predicts nothing and holding back costs 20 us)
                        const uint32_t k = pb.blocks->overlaps() ? std::min<uint32_t>((uint32_t)std::max(0, hold), nd / 64) : 0;
                        if (k) { held.assign(dev_cls.begin(), dev_cls.begin() + k); dev_cls.erase(dev_cls.begin(), dev_cls.begin() + k); nd -= k; }
                    }
                }
                std::vector<uint64_t> cfree((size_t)nd * R), ctot((size_t)nd * R), celig(nd);
                for (uint32_t i = 0; i < nd; i++) {
                    const uint32_t c = dev_cls[i];
                    memcpy(ctot.data() + (size_t)i * R, sigs.data() + (size_t)c * SW, (size_t)R * 8);
                    memcpy(cfree.data() + (size_t)i * R, sigs.data() + (size_t)c * SW + R, (size_t)R * 8);
                    celig[i] = sigs[(size_t)c * SW + 2 * R + 1];
                }
                std::vector<uint32_t> dx((size_t)nd * NC, 0), dstatus(nd, hqblock::ST_UNSUPPORTED), dsteps(nd, 0);
                hqblock::ColTable ct{NC, R, ent_off.data(), ent_res.data(), ent_kind.data(), ent_amount.data(), weight.data(), pool.data(), nullptr, 0};
                hqblock::ClassTable cl{nd, cfree.data(), ctot.data(), celig.data()};
                hqblock::Output bo{dx.data(), dstatus.data(), dsteps.data(), nullptr};
                bool dev_ok = pb.blocks->begin(ct, cl, bo);
                for (uint32_t c : held) {  // (the kernel is running)
                    const int hr = solve_class_on_host(c);
                    if (hr < 0) { if (dev_ok) pb.blocks->finish(); out.keys.clear(); out.per_key.clear(); return out; }
                }
                // The device's answers are not taken on trust (ADVICE r02 #5 / VERDICT r03 next 3).  While the kernel runs the host has nothing to do: it solves a
                // SAMPLE of the launched classes with its own exact solver (block_verify of them, a window that moves with the tick counter so that a steady-state
                // cluster is covered class by class over the ticks; the same window on every replica) and compares the canonical answers afterwards, column by
                // column.  One mismatch distrusts the launch: every class of it goes to the host solver.  And EVERY answer is checked for what can be checked in
                // O(columns): it fits the rows (exact integers), and it is maximal — every cost is positive, so an answer that leaves room for one more task
                // of any eligible column is not an optimum.
                std::vector<uint32_t> probe;  // launch positions of the sampled classes
                if (dev_ok && pb.block_verify && nd) {
                    const uint32_t k = std::min<uint32_t>(pb.block_verify, nd), first = (uint32_t)(((uint64_t)pb.tick_seq * k) % nd);
                    for (uint32_t j = 0; j < k; j++) probe.push_back((first + j) % nd);
                }
                std::vector<uint32_t> probe_x((size_t)probe.size() * NC, 0); std::vector<uint8_t> probe_exact(probe.size(), 0);
                for (size_t pi = 0; pi < probe.size(); pi++) {
                    const uint32_t c = dev_cls[probe[pi]];
                    const bool exact_so_far = blocks_exact; blocks_exact = true;
                    if (solve_class_on_host(c) < 0) { pb.blocks->finish(); out.keys.clear(); out.per_key.clear(); return out; }
                    probe_exact[pi] = blocks_exact ? 1 : 0; blocks_exact = blocks_exact && exact_so_far;
                    memcpy(probe_x.data() + pi * NC, X.data() + (size_t)c * NC, (size_t)NC * 4);
                    out.blocks_host--; out.blocks_verified++;  // (a check, not a fallback)
                }
                dev_ok = dev_ok && pb.blocks->finish();
                if (dev_ok) {
                    for (size_t pi = 0; pi < probe.size() && dev_ok; pi++) {
                        const uint32_t i = probe[pi];
                        if (dstatus[i] != hqblock::ST_OK || !probe_exact[pi]) continue;  // (the device gave up on it, or the host's own answer is not the exact canonical one: nothing to compare)
                        if (memcmp(probe_x.data() + pi * NC, dx.data() + (size_t)i * NC, (size_t)NC * 4) != 0) { out.blocks_mismatch++; dev_ok = false; }
                        else { out.blocks_device++; out.block_steps_max = std::max(out.block_steps_max, dsteps[i]); }  // the device's answer, confirmed
                    }
                }
                if (dev_ok) {
                    std::vector<unsigned __int128> used;
                    for (uint32_t i = 0; i < nd; i++) {
                        if (dstatus[i] != hqblock::ST_OK) continue;
                        const uint32_t c = dev_cls[i];
                        if (solved[c]) continue;  // (a sampled class: the host's answer is in place, and equal)
                        // the answer must fit the worker's rows (exact integer check; anything else is solved again here)
                        bool fits = true;
                        used.assign(R, 0);
                        for (uint32_t g = 0; g < NC && fits; g++) {
                            const uint32_t xv = dx[(size_t)i * NC + g];
                            if (!xv) continue;
                            if (!elig(c, g)) { fits = false; break; }
                            const VariantView &vv = pb.variants[col_slot[g]];
                            for (uint32_t e = 0; e < vv.n_entries; e++) used[vv.res[e]] += (unsigned __int128)(vv.kind[e] == HQ_ENTRY_ALL ? ctot[(size_t)i * R + vv.res[e]] : vv.amount[e]) * xv;
                        }
                        for (uint32_t r = 0; r < R && fits; r++) if (used[r] > cfree[(size_t)i * R + r]) fits = false;
                        // ... and be maximal: no eligible column has room for one more task
                        for (uint32_t g = 0; g < NC && fits; g++) {
                            if (!elig(c, g)) continue;
                            const VariantView &vv = pb.variants[col_slot[g]];
                            bool room = vv.n_entries > 0, gains = false;  // gains: the column's objective coefficient is positive (solver.rs:550-568: weight x sum of amount / pool)
                            for (uint32_t e = 0; e < vv.n_entries && room; e++) {
                                const uint64_t a = vv.kind[e] == HQ_ENTRY_ALL ? ctot[(size_t)i * R + vv.res[e]] : vv.amount[e];
                                if (a && vv.weight && pool[vv.res[e]] >= 0.000001) gains = true;
                                if (used[vv.res[e]] + a > cfree[(size_t)i * R + vv.res[e]]) room = false;
                            }
                            if (room && gains && dx[(size_t)i * NC + g] < (uint32_t)hqblock::UB_LIMIT) fits = false;
                        }
                        if (!fits) { out.blocks_rejected++; continue; }
                        memcpy(X.data() + (size_t)c * NC, dx.data() + (size_t)i * NC, (size_t)NC * 4);
                        solved[c] = 1; out.blocks_device++;
                        out.block_steps_max = std::max(out.block_steps_max, dsteps[i]);
                    }
                } else if (out.blocks_mismatch) {
                    for (uint32_t i = 0; i < nd; i++) solved[dev_cls[i]] = 0;  // the launch is distrusted as a whole: every class of it is solved here
                    out.blocks_device = 0;
                }
            }
            for (uint32_t c = 0; c < ncls; c++) {
                if (solved[c]) continue;
                if (solve_class_on_host(c) < 0) { out.keys.clear(); out.per_key.clear(); return out; }  // `None` => empty solution  solver.rs:433-437
            }
        }
        const double t_sep2 = clock_us();
        if (separable) {
            bool sizes_hold = true;  // the lazy batch-size rows  solver.rs:264-271
            {
                for (size_t b = 0; b < nb && sizes_hold; b++) {
                    if (batches[b].limit_reached) continue;
                    uint64_t placed = 0;
                    for (uint32_t c = 0; c < ncls; c++) for (uint32_t v = voff[b]; v < voff[b + 1]; v++) placed += n_in_class[c] * X[(size_t)c * NC + v];
                    if (placed > batches[b].size) sizes_hold = false;
                }
            }
            if (!sizes_hold) {
                separable = false;
                std::vector<hqmilp::Model> class_model(ncls);
                std::vector<std::vector<ColRef>> class_cols(ncls);
                for (uint32_t c = 0; c < ncls; c++) build_class_model(c, class_model[c], class_cols[c]);
                if (out.is_optimal && blocks_exact) {  // every class block was solved to its EXACT optimum above: only then is "share <= block optimum" valid for every integer point
                    std::vector<double> zc(ncls, -1.0);
                    for (uint32_t c = 0; c < ncls; c++) {
                        if (class_has_flag[c]) continue;
                        double z = 0.0;
                        for (size_t k = 0; k < class_cols[c].size(); k++) if (class_cols[c][k].batch != UINT32_MAX) z += class_model[c].obj[k] * (double)X[(size_t)c * NC + voff[class_cols[c][k].batch] + class_cols[c][k].variant];
                        zc[c] = z;
                    }
                    block_z.assign(ws.n, -1.0);
                    for (uint32_t w : solver_workers) block_z[w] = zc[wclass[w]];
                }
                // Workers that no optimum uses.  Without cuts, blockers and multi-node batches two workers of one class (same free, total, eligibility, no
                // min_utilization) can exchange their whole contents, and a single task can move to any worker that has room for it; both moves keep every
                // row satisfied and, as the objective factor (W - idx)/W falls strictly with the index while every cost is positive, moving towards the
                // lower index strictly improves.  So in EVERY optimal solution (a) the non-empty workers of a class are its first k ones, (b) no task of the
                // k-th one fits into the room left on an earlier one: each earlier worker uses more than free_e - dmax_e of some resource e (dmax_e = the
                // largest single request), and at most (D_e - 1) / (free_e - dmax_e) workers can do that with a total demand of D_e.  Hence
                //     k <= min(#tasks, 1 + sum_e (D_e - 1) / (free_e - dmax_e)),
                // and dropping the class's later workers removes no optimal solution: the canonical optimum is unchanged.  This is what keeps "a few ready
                // tasks, a thousand idle workers" — the everyday case between bursts — a small model.
                worker_off.assign(ws.n, 0);
                {
                    std::vector<uint32_t> seen(class_cols.size(), 0), keep(class_cols.size(), UINT32_MAX);
                    for (size_t c = 0; c < class_cols.size(); c++) {
                        if (class_has_flag[c]) continue;
                        const uint64_t *fre = ws.free_ + (size_t)rep[c] * R, *tot = ws.total + (size_t)rep[c] * R;
                        bool ok = true;
                        uint64_t n_tasks = 0;
                        std::vector<uint64_t> dmax(R, 0);
                        std::vector<long double> D(R, 0.0L);
                        std::vector<uint8_t> batch_seen(nb, 0);
                        std::vector<std::vector<uint64_t>> bmax(nb, std::vector<uint64_t>(R, 0));  // per batch: largest amount over its eligible variants
                        for (const ColRef &cr : class_cols[c]) {
                            if (cr.batch == UINT32_MAX) { ok = false; break; }
                            const uint32_t slot = pb.rqs[batches[cr.batch].rq].first_variant + cr.variant;
                            const VariantView &vv = pb.variants[slot];
                            if (class_model[c].obj.empty()) { ok = false; break; }
                            if (!batch_seen[cr.batch]) { batch_seen[cr.batch] = 1; n_tasks += batches[cr.batch].size; }
                            for (uint32_t e = 0; e < vv.n_entries; e++) {
                                const uint64_t a = vv.kind[e] == HQ_ENTRY_ALL ? tot[vv.res[e]] : vv.amount[e];
                                bmax[cr.batch][vv.res[e]] = std::max(bmax[cr.batch][vv.res[e]], a);
                                dmax[vv.res[e]] = std::max(dmax[vv.res[e]], a);
                            }
                        }
                        for (double cj : class_model[c].obj) if (!(cj > 0.0)) ok = false;  // the exchange argument needs strictly positive costs
                        if (!ok) continue;
                        for (size_t b = 0; b < nb; b++) if (batch_seen[b]) for (uint32_t r = 0; r < R; r++) D[r] += (long double)bmax[b][r] * (long double)batches[b].size;
                        long double k = 1.0L; bool bounded = true;
                        for (uint32_t r = 0; r < R && bounded; r++) {
                            if (dmax[r] == 0 || D[r] <= 0.0L) continue;
                            if (fre[r] == HQ_AMOUNT_MAX || fre[r] <= dmax[r]) { bounded = false; break; }
                            k += std::floor((D[r] - 1.0L) / (long double)(fre[r] - dmax[r]));
                        }
                        uint64_t kk = n_tasks;
                        if (bounded && k < (long double)kk) kk = (uint64_t)k;
                        if (kk < n_in_class[c]) keep[c] = (uint32_t)kk;
                    }
                    for (uint32_t w : solver_workers) { const uint32_t c = wclass[w]; if (seen[c]++ >= keep[c]) worker_off[w] = 1; }
                }
                // Starting point for the coupled model below: workers in objective order (the (W - idx)/W factor prefers the low indices), each one
                // takes the optimum of ITS block given what the earlier ones left of every unsaturated batch.  Not optimal in general, but it fills
                // the early workers exactly — the part the LP-rounding heuristics of the solver are weakest at.
                bool usable = true;
                for (uint8_t fl : class_has_flag) if (fl) usable = false;  // min_utilization flags are not part of the hint
                size_t kept = 0; for (uint32_t w : solver_workers) if (!worker_off[w]) kept++;
                if (usable && pb.pricer && kept * NC >= 2 * (size_t)pb.pricer->min_cols) usable = false;  // the price sweeps build their own incumbent: the W sequential block solves would cost more than they do
                // (a solve that stops at its certificate finds the point of a small model faster than these block solves run: 213 -> 142 us on an 80-column tick)
                if (usable && pb.certificate_only && kept * NC <= 512) usable = false;
                if (usable) {
                    std::vector<double> rem(nb);
                    for (size_t b = 0; b < nb; b++) rem[b] = batches[b].limit_reached ? 1e18 : (double)batches[b].size;
                    std::vector<std::vector<uint32_t>> last_x(class_cols.size());  // last solution per class: still optimal while it fits into `rem`
                    for (uint32_t w : solver_workers) {
                        const uint32_t c = wclass[w];
                        const auto &cols = class_cols[c];
                        bool reuse = !last_x[c].empty();
                        if (reuse) {
                            std::vector<double> need(nb, 0.0);
                            for (size_t k = 0; k < cols.size(); k++) need[cols[k].batch] += last_x[c][k];
                            for (size_t b = 0; b < nb; b++) if (need[b] > rem[b]) reuse = false;
                        }
                        if (!reuse) {
                            hqmilp::Model bm = class_model[c];
                            for (size_t b = 0; b < nb; b++) {
                                if (rem[b] >= 1e17) continue;
                                bool any = false;
                                for (size_t k = 0; k < cols.size(); k++) if (cols[k].batch == b) any = true;
                                if (!any) continue;
                                bm.begin_row(hqmilp::ROW_MAX, rem[b]);
                                for (size_t k = 0; k < cols.size(); k++) if (cols[k].batch == b) bm.term((int)k, 1.0);
                                bm.end_row();
                            }
                            hqmilp::Result bs = hqmilp::solve(bm, std::min(0.05, pb.time_limit_s), false);
                            if (!bs.feasible) { seq_start.clear(); usable = false; break; }
                            last_x[c].assign(cols.size(), 0);
                            for (size_t k = 0; k < cols.size(); k++) last_x[c][k] = (uint32_t)std::round(bs.x[k]);
                        }
                        for (size_t k = 0; k < cols.size(); k++) {
                            const uint32_t cnt = last_x[c][k];
                            if (!cnt) continue;
                            seq_start.push_back({w, cols[k].batch, cols[k].variant, cnt});
                            if (rem[cols[k].batch] < 1e17) rem[cols[k].batch] -= cnt;
                        }
                    }
                }
            }
        }
        if (separable) {
            std::vector<uint64_t> key_hash; std::vector<std::pair<uint32_t, uint8_t>> key_list; std::vector<std::vector<std::pair<uint32_t, uint32_t>>> key_counts;
            // The workers of a key are those whose class places something in its column: keys with the same set of classes share the id list and its Map
            // order (a cold tick has one class: one list for all keys).
            struct WorkerList { std::vector<uint8_t> mask; std::vector<uint32_t> widx, order; };  // order: a copy — the memo behind cached_worker_order recycles its entries
            std::vector<WorkerList> lists; lists.reserve((size_t)NC + 1);  // (pointers into it are kept below)
            std::vector<uint32_t> key_g, key_l;
            std::vector<uint8_t> mask(ncls);
            std::vector<uint32_t> ids, ord;
            for (size_t b = 0; b < nb; b++) {
                for (uint8_t v = 0; v < pb.rqs[batches[b].rq].n_variants; v++) {
                    const uint32_t g = voff[b] + v;
                    bool any = false;
                    for (uint32_t c = 0; c < ncls; c++) { mask[c] = X[(size_t)c * NC + g] != 0; any = any || mask[c]; }
                    if (!any) continue;
                    const WorkerList *wl = nullptr;
                    for (const WorkerList &l : lists) if (memcmp(l.mask.data(), mask.data(), ncls) == 0) { wl = &l; break; }
                    if (!wl) {
                        lists.emplace_back();
                        WorkerList &l = lists.back();
                        l.mask = mask;
                        {   // the key's workers, in solver order: written unconditionally, kept by advancing the cursor (no push_back, no branch on the class mask)
                            const size_t nsw = solver_workers.size();
                            ids.resize(nsw + 1); l.widx.resize(nsw + 1);
                            uint32_t *idp = ids.data(), *wxp = l.widx.data(); size_t nk = 0;
                            const uint8_t *mk = mask.data(); const uint32_t *wc = wclass.data(), *wid = ws.id;
                            for (size_t i = 0; i < nsw; i++) { const uint32_t w = solver_workers[i]; idp[nk] = wid[w]; wxp[nk] = w; nk += mk[wc[w]]; }
                            ids.resize(nk); l.widx.resize(nk);
                        }
                        l.order = cached_worker_order(ids);
                        wl = &l;
                    }
                    std::vector<std::pair<uint32_t, uint32_t>> ordered;
                    if (pb.custom) {  // (the tick's own results carry the per-class form instead and build pairs on demand: Counts::pairs)
                        ordered.resize(wl->order.size());
                        const uint32_t *word = wl->order.data(), *widx = wl->widx.data(), *xg = X.data() + g;
                        std::pair<uint32_t, uint32_t> *o = ordered.data();
                        for (size_t k = 0, e = ordered.size(); k < e; k++) { const uint32_t w = widx[word[k]]; o[k] = {w, xg[(size_t)wclass[w] * NC]}; }
                    }
                    key_hash.push_back(hqhb::hash_rq_variant(batches[b].rq, v)); key_list.push_back({batches[b].rq, v}); key_counts.push_back(std::move(ordered));
                    key_g.push_back(g); key_l.push_back((uint32_t)(wl - lists.data()));
                }
            }
            hqhb::insertion_order(key_hash.data(), (uint32_t)key_hash.size(), ord);
            for (uint32_t k : ord) { out.keys.push_back(key_list[k]); out.per_key.push_back(std::move(key_counts[k])); out.key_col.push_back(key_g[k]); out.key_list.push_back(key_l[k]); }
            if (!pb.custom) {  // the per-class form of the same counts, for the mapping plan (host_model.h)
                out.by_class = true; out.pairs_built = false; out.n_cols = NC; out.one_class = ncls == 1 && solver_workers.size() == ws.n;
                out.class_x = X; out.class_x.resize((size_t)(ncls + 1) * NC, 0);
                out.wclass.assign(ws.n, ncls);
                for (uint32_t w : solver_workers) out.wclass[w] = wclass[w];
                out.lists.resize(lists.size());
                for (size_t i = 0; i < lists.size(); i++) {
                    const WorkerList &l = lists[i];
                    std::vector<uint32_t> &dst = out.lists[i].widx; dst.resize(l.order.size());
                    for (size_t k = 0; k < l.order.size(); k++) dst[k] = l.widx[l.order[k]];
                }
            }
            out.n_classes = ncls; out.t_classify_us = t_sep1 - t_sep0; out.t_blocks_us = t_sep2 - t_sep1; out.t_decode_us = clock_us() - t_sep2;
            return out;
        }
        { const double a_ = t_sep1 - t_sep0, b_ = t_sep2 - t_sep1; out = Counts(); out.t_classify_us = a_; out.t_blocks_us = b_; }  // fall through to the general path (the two times: for the trace below)
    }

    // the gap rows below dereference the snapshot's assigned (rq, variant) lists: a bad index is the caller's error, not a crash
    if (!pb.custom && ws.assigned_off) {
        bool any_cut = false;
        for (const TaskBatch &b : batches) if (!b.cuts.empty()) any_cut = true;
        if (any_cut) for (uint32_t i = 0, e = ws.n ? ws.assigned_off[ws.n] : 0; i < e; i++)
            if (ws.assigned_rq[i] >= pb.rqs.size() || ws.assigned_variant[i] >= pb.rqs[ws.assigned_rq[i]].n_variants) { out.error = HQTICK_E_INVALID; out.errmsg = "assigned (rq, variant) out of range"; return out; }
    }
    hqmilp::Model m;
    const double t_model0 = clock_us();
    // structure hints for the coupled solve (csrc/price.h): a worker's columns form a block, the flags and group sizes belong to the whole model
    auto addc = [&](double w, uint8_t kind, int32_t group) { m.col_group.push_back(group); return m.add_col(w, kind); };
    // (worker, rq, variant) -> column   :88   — a flat table over (worker, variant slot), -1 = no column
    const uint32_t NVS = ws.n_variant_slots;
    std::vector<int> place_col((size_t)ws.n * NVS, -1);
    std::vector<uint32_t> col_ub;  // per column: how often the request fits into the worker's free resources (what its resource rows allow at most)
    auto place_get = [&](uint32_t w, uint32_t rq, uint8_t v) -> int { return place_col[(size_t)w * NVS + pb.rqs[rq].first_variant + v]; };
    std::map<uint32_t, std::vector<int>> count_cols;               // tasks_count_vars   :89
    std::vector<std::vector<std::pair<int, double>>> res_terms(R);
    std::vector<std::pair<int, double>> cpu_terms, block_terms;
    std::vector<uint8_t> res_carry(R, 0);
    // structure hint (milp.h: Model::row_block): the row holds columns of ONE worker's block and nothing else
    auto mark_block = [&](int32_t wi_) { m.row_block.resize((size_t)m.nrows(), -1); m.row_block.back() = wi_; };
    auto emit = [&](uint8_t type, double rhs, const std::vector<std::pair<int, double>> &terms) { m.begin_row(type, rhs); for (auto &t : terms) m.term(t.first, t.second); m.end_row(); };
    // a list of columns with coefficient 1 (the count columns of a request, the columns of the workers a blocker leaves no gap on: a thousand terms each, written many times)
    auto ones = [&](const std::vector<int> &cols) { m.rcol.insert(m.rcol.end(), cols.begin(), cols.end()); m.rcoef.resize(m.rcol.size(), 1.0); };
    auto emit_plus = [&](uint8_t type, double rhs, const std::vector<int> &cols, int extra, double coef) { m.begin_row(type, rhs); ones(cols); m.term(extra, coef); m.end_row(); };
    // WorkerGroup::is_capable_to_run_rq  server/workergroup.rs:35-52 (over the real worker map)
    auto group_can_run = [&](uint32_t g, const VariantView &vv, uint32_t slot) {
        uint32_t need = vv.multi_node() ? vv.n_nodes : 1;
        for (uint32_t w = 0; w < pb.real.n; w++) {
            if ((pb.real.group ? pb.real.group[w] : 0) != g) continue;
            uint8_t f = pb.real.vf(w, slot);
            if ((f & 4) && (vv.multi_node() || (f & 2))) { if (--need == 0) return true; }
        }
        return false;
    };
    auto group_can_run_rq = [&](uint32_t g, uint32_t rq) {
        for (uint32_t v = 0; v < pb.rqs[rq].n_variants; v++) if (group_can_run(g, pb.variants[pb.rqs[rq].first_variant + v], pb.rqs[rq].first_variant + v)) return true;
        return false;
    };

    {   // one allocation per array of the model instead of a doubling series (an upper estimate: every worker takes every variant of every batch)
        size_t nvar = 0; for (const TaskBatch &batch : batches) nvar += pb.rqs[batch.rq].n_variants;
        const size_t est_cols = nw * nvar + 64, est_rows = nw * ((size_t)R + 3) + 4 * batches.size() + 64;
        m.obj.reserve(est_cols); m.kind.reserve(est_cols); m.col_group.reserve(est_cols); col_ub.reserve(est_cols);
        m.rtype.reserve(est_rows); m.rhs.reserve(est_rows); m.roff.reserve(est_rows + 1);
        m.rcol.reserve(est_cols * 4); m.rcoef.reserve(est_cols * 4);
    }
    // A worker whose snapshot rows equal the previous worker's (WorkerGroups: same total / free / remaining time / min_utilization / flags, nothing blocked) gets the
    // same block — the same columns, bounds and rows — up to the objective's factor (W - idx): the block of the group's first worker is kept as a TEMPLATE (the slices
    // of the model it wrote, column numbers relative to its first column) and stamped out for the rest.  A cold cluster is one group; a cluster mid-run has about one
    // group per worker and builds every block as before.  Only plain blocks are templates: single-node placement columns and `<=` rows over them, nothing carried.
    struct BlockTemplate {
        uint32_t group = UINT32_MAX; bool ok = false;
        std::vector<double> s, wq; std::vector<uint32_t> slot, rq, ub;          // per column: cost without the order factor, weight, variant slot, request, bound
        std::vector<double> rhs; std::vector<uint8_t> implied; std::vector<int> roff{0}, rcol; std::vector<double> rcoef;   // per row (all `<=`, all of this block)
        std::vector<std::vector<int> *> cc;   // per column: its request's list of count columns (a node of count_cols: stays where it is) — not a map walk per column
        int col0 = 0, row0 = 0, term0 = 0; uint32_t worker = 0;   // where the template's own block lies in the model, and whose it is
    } tmpl;
    // Equal-block runs (milp.h: Model::block_runs): the template's block and its stamps lie back to back and differ in `obj` only — said to the flattener, which then
    // works on the first block and copies; and used below, where one worker's answer is the run's.  stamp_first[w]: the worker whose block w's block is a stamp of.
    const bool runs_on = hqmilp::block_runs_on();
    std::vector<uint32_t> stamp_first, run_members; std::vector<int> blk_base;
    if (runs_on) { stamp_first.assign(ws.n, UINT32_MAX); blk_base.assign(ws.n, -1); }
    std::vector<double> rec_s, rec_wq; std::vector<uint32_t> rec_slot, rec_rq;   // what the loop below records per placement column while it builds a block
    for (size_t wi = 0; wi < nw; wi++) {  // :95
        uint32_t w = solver_workers[wi];
        if (!worker_off.empty() && worker_off[w]) continue;  // empty in every optimum (see the separable section): no columns, no rows
        const uint64_t *tot = ws.total + (size_t)w * R, *fre = ws.free_ + (size_t)w * R;
        double order_factor = (double)(nw - wi);
        const uint32_t my_group = (ws.rows.valid && !pb.custom) ? ws.rows.of[w] : UINT32_MAX;
        if (runs_on && tmpl.ok && my_group != UINT32_MAX && my_group == tmpl.group) {   // the template's block for the whole run of workers that follow with its group, in one go
            run_members.clear();
            size_t wj = wi;
            for (; wj < nw; wj++) {   // (a worker that emits nothing does not end the run)
                const uint32_t w2 = solver_workers[wj];
                if (!worker_off.empty() && worker_off[w2]) continue;
                if (ws.rows.of[w2] != tmpl.group) break;
                run_members.push_back((uint32_t)wj);
            }
            const size_t nm = run_members.size(), nc = tmpl.s.size(), nr = tmpl.roff.size() - 1, nt = tmpl.rcol.size();
            const int base0 = m.ncols(), rbase0 = m.nrows(); const size_t tbase0 = m.rcol.size();
            m.obj.resize((size_t)base0 + nm * nc); m.kind.resize((size_t)base0 + nm * nc, hqmilp::COL_NAT); m.col_group.resize((size_t)base0 + nm * nc);
            col_ub.resize((size_t)base0, UINT32_MAX); col_ub.resize((size_t)base0 + nm * nc);
            m.rtype.resize((size_t)rbase0 + nm * nr, hqmilp::ROW_MAX); m.rhs.resize((size_t)rbase0 + nm * nr); m.roff.resize((size_t)rbase0 + 1 + nm * nr);
            m.rcol.resize(tbase0 + nm * nt); m.rcoef.resize(tbase0 + nm * nt);
            m.row_block.resize((size_t)rbase0, -1); m.row_block.resize((size_t)rbase0 + nm * nr);
            bool any_implied = false; for (uint8_t f : tmpl.implied) if (f) any_implied = true;
            if (any_implied) m.row_implied.resize((size_t)rbase0 + nm * nr, 0);
            for (std::vector<int> *cc : tmpl.cc) cc->reserve(cc->size() + nm);
            const double *ts = tmpl.s.data(), *twq = tmpl.wq.data(); const uint32_t *tslot = tmpl.slot.data(), *tub = tmpl.ub.data();
            const int *troff = tmpl.roff.data(), *trcol = tmpl.rcol.data();
            for (size_t i = 0; i < nm; i++) {
                const size_t wi2 = run_members[i]; const uint32_t w2 = solver_workers[wi2];
                const double of2 = (double)(nw - wi2);
                const int base = base0 + (int)(i * nc), rbase = rbase0 + (int)(i * nr); const int tbase = (int)(tbase0 + i * nt);
                double *ob = m.obj.data() + base; int32_t *cg = m.col_group.data() + base; int *pc = place_col.data() + (size_t)w2 * NVS;
                for (size_t k = 0; k < nc; k++) { ob[k] = ts[k] * of2 * twq[k] / (double)nw; cg[k] = (int32_t)wi2; pc[tslot[k]] = base + (int)k; tmpl.cc[k]->push_back(base + (int)k); }
                memcpy(col_ub.data() + base, tub, nc * sizeof(uint32_t));
                memcpy(m.rhs.data() + rbase, tmpl.rhs.data(), nr * sizeof(double));
                int *ro = m.roff.data() + rbase + 1; int32_t *rb = m.row_block.data() + rbase;
                for (size_t r = 0; r < nr; r++) { ro[r] = tbase + troff[r + 1]; rb[r] = (int32_t)wi2; }
                if (any_implied) for (size_t r = 0; r < nr; r++) if (tmpl.implied[r]) m.row_implied[(size_t)rbase + r] = 1;
                int *rc = m.rcol.data() + tbase;
                for (size_t t = 0; t < nt; t++) rc[t] = base + trcol[t];
                memcpy(m.rcoef.data() + tbase, tmpl.rcoef.data(), nt * sizeof(double));
                stamp_first[w2] = tmpl.worker; blk_base[w2] = base;
            }
            blk_base[tmpl.worker] = tmpl.col0;
            m.block_runs.push_back({tmpl.col0, tmpl.row0, tmpl.term0, (int32_t)(1 + nm), (int32_t)nc, (int32_t)nr, (int32_t)nt});
            tmpl.ok = false;   // (the next worker is of another group, or there is none)
            wi = wj - 1;
            continue;
        }
        if (tmpl.ok && my_group != UINT32_MAX && my_group == tmpl.group) {   // (HQMILP_BLOCK_RUNS=0: one worker at a time)
            const int base = m.ncols();
            for (size_t k = 0; k < tmpl.s.size(); k++) {
                const int col = addc(tmpl.s[k] * order_factor * tmpl.wq[k] / (double)nw, hqmilp::COL_NAT, (int32_t)wi);
                place_col[(size_t)w * NVS + tmpl.slot[k]] = col;
                col_ub.resize((size_t)col + 1, UINT32_MAX); col_ub[col] = tmpl.ub[k];
                tmpl.cc[k]->push_back(col);
            }
            for (size_t r = 0; r + 1 < tmpl.roff.size(); r++) {
                m.begin_row(hqmilp::ROW_MAX, tmpl.rhs[r]);
                for (int t = tmpl.roff[r]; t < tmpl.roff[r + 1]; t++) m.term(base + tmpl.rcol[t], tmpl.rcoef[t]);
                m.end_row();
                if (tmpl.implied[r]) { m.row_implied.resize(m.nrows(), 0); m.row_implied.back() = 1; }
                mark_block((int32_t)wi);
            }
            continue;
        }
        const int rec_col0 = m.ncols(), rec_row0 = m.nrows(), rec_term0 = (int)m.rcol.size();
        rec_s.clear(); rec_wq.clear(); rec_slot.clear(); rec_rq.clear();
        bool rec_plain = my_group != UINT32_MAX;   // (stays true while the block is one a template can describe)
        for (uint32_t r = 0; r < R; r++) if (res_carry[r] || !res_terms[r].empty()) rec_plain = false;   // terms carried in from an unbounded resource of an earlier worker
        cpu_terms.clear();
        block_terms.clear();
        for (const TaskBatch &batch : batches) {
            const RequestView &rv = pb.rqs[batch.rq];
            bool any_variant = false;
            for (uint8_t v = 0; v < rv.n_variants; v++) {
                uint32_t slot = rv.first_variant + v;
                const VariantView &vv = pb.variants[slot];
                uint8_t f = ws.vf(w, slot);
                if (vv.multi_node()) {  // :101-122
                    bool free_worker = pb.custom ? true : ws.is_free(w);
                    if (free_worker && pb.custom) { out.error = HQTICK_E_UNSUPPORTED; out.errmsg = "multi-node batch with fake workers: the reference panics (solver.rs:104-106)"; return out; }
                    if (free_worker && group_can_run(ws.group ? ws.group[w] : 0, vv, slot)) {
                        double s = 0.0;  // create_mn_var  :573-597
                        for (uint32_t r = 0; r < R; r++) if (tot[r]) s += pool[r] < 0.000001 ? 0.0 : units(tot[r]) / pool[r];
                        int col = addc(s * order_factor * ((double)vv.weight / FRACTIONS) / (double)nw, hqmilp::COL_BOOL, (int32_t)wi);
                        place_col[(size_t)w * NVS + slot] = col; col_ub.resize((size_t)col + 1, 1); col_ub[col] = 1;
                        for (uint32_t r = 0; r < R; r++) if (tot[r]) res_terms[r].push_back({col, units(tot[r])});
                    }
                } else if (!is_blocked(w, batch.rq, v) && (f & 4) && (f & 1) && (pb.custom || ws.is_sn(w))) {  // :123-126
                    any_variant = true;
                    double s = 0.0;  // create_sn_var  :542-571
                    for (uint32_t e = 0; e < vv.n_entries; e++) {
                        double g = pool[vv.res[e]];
                        s += g < 0.000001 ? 0.0 : units(vv.kind[e] == HQ_ENTRY_ALL ? tot[vv.res[e]] : vv.amount[e]) / g;
                    }
                    int col = addc(s * order_factor * ((double)vv.weight / FRACTIONS) / (double)nw, hqmilp::COL_NAT, (int32_t)wi);
                    place_col[(size_t)w * NVS + slot] = col;
                    rec_s.push_back(s); rec_wq.push_back((double)vv.weight / FRACTIONS); rec_slot.push_back(slot); rec_rq.push_back(batch.rq);
                    {   // the column's own bound: min over its entries of floor(free / amount)
                        uint64_t ubc = UINT32_MAX;
                        for (uint32_t e = 0; e < vv.n_entries; e++) {
                            const uint64_t f = fre[vv.res[e]], am = vv.kind[e] == HQ_ENTRY_ALL ? tot[vv.res[e]] : vv.amount[e];
                            if (f == HQ_AMOUNT_MAX || am == 0) continue;
                            ubc = std::min<uint64_t>(ubc, f / am);
                        }
                        col_ub.resize((size_t)col + 1, UINT32_MAX); col_ub[col] = (uint32_t)ubc;
                    }
                    count_cols[batch.rq].push_back(col);
                    block_terms.push_back({col, s * ((double)vv.weight / FRACTIONS)});
                    for (uint32_t e = 0; e < vv.n_entries; e++) {
                        double a = units(vv.kind[e] == HQ_ENTRY_ALL ? tot[vv.res[e]] : vv.amount[e]);
                        res_terms[vv.res[e]].push_back({col, a});
                        if (vv.res[e] == 0) cpu_terms.push_back({col, a});
                    }
                }
            }
            if (!any_variant && !pb.rq_multi_node(batch.rq) && batch.is_blocker && pb.capable_rqv(ws, w, batch.rq) && (pb.custom || ws.is_sn(w))) {  // :153-169
                int col = addc((double)wi / (double)(nw * 100), hqmilp::COL_BOOL, (int32_t)wi);
                count_cols[batch.rq].push_back(col);
                for (uint32_t r = 0; r < R; r++) if (fre[r]) res_terms[r].push_back({col, units(fre[r])});
            }
        }
        float mu = ws.min_util ? ws.min_util[w] : 0.0f;
        if (mu > 0.001f && tot[0] != HQ_AMOUNT_MAX) {  // add_min_utilization  :501-540
            double all_cpus = units(tot[0]), need = all_cpus * ((double)mu - 1.0) + units(fre[0]);
            if (!(need < 0.0001)) {
                int col = addc(0.0, hqmilp::COL_BOOL, (int32_t)wi);
                cpu_terms.push_back({col, -need}); emit(hqmilp::ROW_MIN, 0.0, cpu_terms); cpu_terms.pop_back(); mark_block((int32_t)wi);
                cpu_terms.push_back({col, -all_cpus}); emit(hqmilp::ROW_MAX, 0.0, cpu_terms); cpu_terms.pop_back(); mark_block((int32_t)wi);
            }
        }
        if (!block_z.empty() && block_z[w] >= 0.0 && block_terms.size() >= 2)  // the worker's block optimum caps its share of the objective (see block_z)
            { emit(hqmilp::ROW_MAX, block_z[w] * (1.0 + 1e-9) + 1e-12, block_terms); m.row_implied.resize(m.nrows(), 0); m.row_implied.back() = 1; mark_block((int32_t)wi); }  // (implied, for integer points, by the worker's resource rows)
        for (uint32_t r = 0; r < R; r++) {  // :177-191 (an unbounded resource keeps its terms for the next worker, as in the reference)
            if (fre[r] == HQ_AMOUNT_MAX) { if (!res_terms[r].empty()) res_carry[r] = 1; continue; }
            if (!res_terms[r].empty()) { emit(hqmilp::ROW_MAX, units(fre[r]), res_terms[r]); mark_block(res_carry[r] ? -1 : (int32_t)wi); }  // (a row that carries an earlier worker's terms is not one block's)
            res_terms[r].clear(); res_carry[r] = 0;
        }
        // this worker's block as the template of the workers of its group that follow — if it is a plain one: placement columns only (every column the loop created was
        // recorded), `<=` rows over them only, nothing carried over to the next worker
        tmpl.ok = false;
        if (rec_plain && (size_t)(m.ncols() - rec_col0) == rec_s.size() && !rec_s.empty()) {
            bool plain = true;
            for (uint32_t r = 0; r < R; r++) if (res_carry[r] || !res_terms[r].empty()) plain = false;
            for (int i = rec_row0; i < m.nrows() && plain; i++) if (m.rtype[i] != hqmilp::ROW_MAX) plain = false;
            for (int t = rec_term0; t < (int)m.rcol.size() && plain; t++) if (m.rcol[t] < rec_col0) plain = false;
            if (plain) {
                tmpl.group = my_group; tmpl.ok = true; tmpl.col0 = rec_col0; tmpl.row0 = rec_row0; tmpl.term0 = rec_term0; tmpl.worker = w;
                tmpl.s = rec_s; tmpl.wq = rec_wq; tmpl.slot = rec_slot; tmpl.rq = rec_rq;
                tmpl.cc.resize(tmpl.rq.size()); for (size_t k = 0; k < tmpl.rq.size(); k++) tmpl.cc[k] = &count_cols[tmpl.rq[k]];
                tmpl.ub.assign(col_ub.begin() + rec_col0, col_ub.begin() + m.ncols());
                tmpl.rhs.assign(m.rhs.begin() + rec_row0, m.rhs.end());
                tmpl.implied.assign((size_t)(m.nrows() - rec_row0), 0);
                for (int i = rec_row0; i < m.nrows(); i++) if ((size_t)i < m.row_implied.size() && m.row_implied[i]) tmpl.implied[(size_t)(i - rec_row0)] = 1;
                tmpl.roff.assign(1, 0); tmpl.rcol.clear(); tmpl.rcoef.clear();
                for (int i = rec_row0; i < m.nrows(); i++) {
                    for (int t = m.roff[i]; t < m.roff[i + 1]; t++) { tmpl.rcol.push_back(m.rcol[t] - rec_col0); tmpl.rcoef.push_back(m.rcoef[t]); }
                    tmpl.roff.push_back((int)tmpl.rcol.size());
                }
            }
        }
    }
    if (hqmilp::g_probe && hqmilp::g_probe->corrupt_runs && m.block_runs.size() >= 2) {   // tests: two neighbouring runs merged into one false claim (the flattener must refuse it)
        m.block_runs[0].n_blocks += m.block_runs[1].n_blocks; m.block_runs.erase(m.block_runs.begin() + 1);
    }
    // multi-node group sizes  :193-227
    std::map<std::pair<uint32_t, uint32_t>, int> group_cols;
    for (const TaskBatch &batch : batches) {
        if (!pb.rq_multi_node(batch.rq)) continue;
        double n_nodes = (double)pb.variants[pb.rqs[batch.rq].first_variant].n_nodes;
        for (uint32_t g = 0; g < pb.n_groups; g++) {
            std::vector<int> members;
            for (uint32_t w = 0; w < pb.real.n; w++) {
                if ((pb.real.group ? pb.real.group[w] : 0) != g) continue;
                const int pc = place_get(w, batch.rq, 0);
                if (pc >= 0) members.push_back(pc);
            }
            if (members.empty()) continue;
            int col = addc(0.0, hqmilp::COL_NAT, -1);
            emit_plus(hqmilp::ROW_EQ, 0.0, members, col, -n_nodes);
            count_cols[batch.rq].push_back(col);
            group_cols[{batch.rq, g}] = col;
        }
    }
    // Structure hint for the coupled solve (milp.h: Model::row_lhs): rows whose leading terms are one and the same list — a request's count columns (its batch-size row
    // and its "blocker short" rows), the columns of the workers on which a blocker leaves no gap (every cut of the batch against that blocker) — carry the list's id.
    int next_lhs_id = 0;
    std::vector<int> count_ids;
    auto count_lhs_id = [&](uint32_t rq) { if (count_ids.size() <= rq) count_ids.resize((size_t)rq + 1, -1); if (count_ids[rq] < 0) count_ids[rq] = next_lhs_id++; return count_ids[rq]; };
    // A row `list (+ extra term)`: the list — a request's count columns, the no-gap columns of a (batch, blocker) pair — is written into the model ONCE, under its id
    // (milp.h: Model::list_off); every row that starts with it names it and stores only what follows.  id < 0 (a multi-node batch's lists): an ordinary row.
    std::vector<int> list_of_id;
    auto list_row = [&](uint8_t type, double rhs, int id, const std::vector<int> &cols, int extra, double coef) {
        m.begin_row(type, rhs);
        if (id < 0) ones(cols);
        if (extra >= 0) m.term(extra, coef);
        m.end_row();
        m.row_lhs.resize((size_t)m.nrows(), -1); m.row_lhs_len.resize((size_t)m.nrows(), 0);
        if (id < 0) return;
        if ((size_t)id >= list_of_id.size()) list_of_id.resize((size_t)id + 1, -1);
        if (list_of_id[(size_t)id] < 0) list_of_id[(size_t)id] = m.add_list(cols.data(), cols.size());
        m.row_lhs.back() = list_of_id[(size_t)id]; m.row_lhs_len.back() = (int32_t)cols.size();
    };
    // priority cuts  :229-430
    std::map<std::pair<uint32_t, uint32_t>, int> short_flags;  // blocked_priority_vars
    auto short_flag = [&](uint32_t rq, uint32_t size) -> int {  // get_bvar  :233-253
        auto it = short_flags.find({rq, size});
        if (it != short_flags.end()) return it->second;
        auto cc = count_cols.find(rq);
        if (cc == count_cols.end()) return -1;
        int col = addc(0.0, hqmilp::COL_BOOL, -1);
        list_row(hqmilp::ROW_MIN, (double)size, count_lhs_id(rq), cc->second, col, (double)size);
        short_flags[{rq, size}] = col;
        return col;
    };
    static const bool trace_model = getenv("HQMILP_TRACE") != nullptr;
    if (trace_model) fprintf(stderr, "[model] model build entered %.3f ms after the solver (worker classes %.3f, class blocks %.3f, lazy rows / empty workers / start %.3f); worker blocks built at %.3f ms\n", (t_model0 - t_enter) / 1e3, out.t_classify_us / 1e3, out.t_blocks_us / 1e3, (t_model0 - t_enter - out.t_classify_us - out.t_blocks_us) / 1e3, (clock_us() - t_model0) / 1e3);
    GapCache gaps(pb);
    // the gap depends on the worker's total resources and on what runs there: workers with the same signature share one computation per (blocker, batch)
    // (signatures: a flat table of hashes over (total row, running kinds) with the first worker of each as its representative — the rows are compared where they lie)
    std::vector<uint32_t> gap_sig, sig_rep, sig_table; std::vector<uint64_t> sig_hash;
    size_t n_sig_cap = (size_t)ws.n + 1;  // signatures are numbered below the worker count (gap_of narrows this to their number: every worker has its signature by then)
    // per (blocker, signature) — blockers numbered as they turn up: 0 not computed, 1 leftover in left_of (the general rule), 2 gap is 0 by rule, 3 leftover in left_row
    std::vector<int32_t> blocker_ord; uint32_t n_blockers_seen = 0;
    std::vector<uint8_t> left_state; std::vector<Amounts> left_of; std::vector<uint64_t> left_row;
    // a worker's running tasks as distinct (rq, variant) pairs with counts (a busy worker runs ~100 tasks of ~8 kinds: the gap of every (blocker, batch) pair walks this list)
    std::vector<uint32_t> agg_off, agg_rq, agg_cnt; std::vector<uint8_t> agg_variant;
    auto build_agg = [&]() {
        agg_off.assign((size_t)ws.n + 1, 0);
        if (!pb.custom && !ws.assigned_off && ws.agg_off) {  // the assignment ledger's counts: the same lists, no pass over the running tasks
            agg_off.assign(ws.agg_off, ws.agg_off + ws.n + 1);
            const uint32_t e = ws.agg_off[ws.n];
            agg_rq.assign(ws.agg_rq, ws.agg_rq + e); agg_variant.assign(ws.agg_variant, ws.agg_variant + e); agg_cnt.assign(ws.agg_cnt, ws.agg_cnt + e);
            return;
        }
        if (pb.custom || !ws.assigned_off) return;
        // (counted per variant slot, not sorted: a busy worker runs a hundred tasks of a handful of kinds — sorting 1024 such lists was a millisecond of a 3 ms tick)
        std::vector<uint32_t> keys, cnt(NVS, 0);
        for (uint32_t w = 0; w < ws.n; w++) {
            keys.clear();
            for (uint32_t i = ws.assigned_off[w]; i < ws.assigned_off[w + 1]; i++) {
                const uint32_t slot = pb.rqs[ws.assigned_rq[i]].first_variant + ws.assigned_variant[i];
                if (cnt[slot]++ == 0) keys.push_back((ws.assigned_rq[i] << 8) | ws.assigned_variant[i]);
            }
            std::sort(keys.begin(), keys.end());  // the distinct kinds only, ascending (rq, variant) as before
            for (uint32_t k : keys) {
                const uint32_t slot = pb.rqs[k >> 8].first_variant + (k & 0xFFu);
                agg_rq.push_back(k >> 8); agg_variant.push_back((uint8_t)(k & 0xFFu)); agg_cnt.push_back(cnt[slot]); cnt[slot] = 0;
            }
            agg_off[w + 1] = (uint32_t)agg_rq.size();
        }
    };
    auto sig_of = [&](uint32_t w) -> uint32_t {
        if (gap_sig.empty()) { gap_sig.assign(ws.n, UINT32_MAX); size_t cap = 64; while (cap < 2 * (size_t)ws.n + 2) cap <<= 1; sig_table.assign(cap, UINT32_MAX); }
        if (gap_sig[w] != UINT32_MAX) return gap_sig[w];
        if (agg_off.empty()) build_agg();
        const uint64_t *tw = ws.total + (size_t)w * R;
        const uint32_t a0 = agg_off[w], na = agg_off[w + 1] - a0;
        uint64_t h = 0x9E3779B97F4A7C15ull ^ na;
        for (uint32_t r = 0; r < R; r++) { h ^= tw[r]; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
        for (uint32_t i = a0; i < a0 + na; i++) { h ^= ((uint64_t)agg_cnt[i] << 32) | ((uint64_t)agg_rq[i] << 8) | agg_variant[i]; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 32; }  // (sorted by (rq, variant): the multiset of running tasks decides — saturating subtractions commute)
        const size_t mask = sig_table.size() - 1;
        for (size_t pos = (size_t)h & mask;; pos = (pos + 1) & mask) {
            const uint32_t id = sig_table[pos];
            if (id == UINT32_MAX) { sig_table[pos] = (uint32_t)sig_rep.size(); sig_rep.push_back(w); sig_hash.push_back(h); return gap_sig[w] = (uint32_t)sig_rep.size() - 1; }
            if (sig_hash[id] != h) continue;
            const uint32_t o = sig_rep[id], b0 = agg_off[o];
            if (agg_off[o + 1] - b0 != na || memcmp(ws.total + (size_t)o * R, tw, (size_t)R * 8) != 0) continue;
            if (na && (memcmp(agg_rq.data() + b0, agg_rq.data() + a0, (size_t)na * 4) != 0 || memcmp(agg_variant.data() + b0, agg_variant.data() + a0, na) != 0 || memcmp(agg_cnt.data() + b0, agg_cnt.data() + a0, (size_t)na * 4) != 0)) continue;
            return gap_sig[w] = id;
        }
    };
    bool sigs_done = false;   // every solver worker has its signature
    // what the blocker leaves of the workers with signature sg (w: one of them), once per (blocker, signature); then how many tasks of the batch fit into that
    auto gap_of = [&](uint32_t brq, uint32_t low_rq, uint32_t sg, uint32_t w) -> uint32_t {
        if (blocker_ord.empty()) { blocker_ord.assign(pb.rqs.size(), -1); if (sigs_done) n_sig_cap = sig_rep.size() + 1; }
        if (blocker_ord[brq] < 0) {
            blocker_ord[brq] = (int32_t)n_blockers_seen++;
            left_state.resize((size_t)n_blockers_seen * n_sig_cap, 0); left_row.resize((size_t)n_blockers_seen * n_sig_cap * R); left_of.resize(left_state.size());
        }
        const size_t li = (size_t)blocker_ord[brq] * n_sig_cap + sg;
        if (left_state[li] == 0) {
            if (agg_off.empty()) build_agg();
            const uint32_t a0 = agg_off[w], na = agg_off[w + 1] - a0;
            const uint32_t *arq = na ? agg_rq.data() + a0 : nullptr, *acnt = na ? agg_cnt.data() + a0 : nullptr; const uint8_t *avar = na ? agg_variant.data() + a0 : nullptr;
            if (gaps.leftover_row(brq, ws.total + (size_t)w * R, R, arq, avar, na, acnt, &left_row[li * R])) left_state[li] = 3;
            else {
                Amounts tot; tot.a.assign(ws.total + (size_t)w * R, ws.total + (size_t)(w + 1) * R);
                left_state[li] = gaps.leftover(brq, tot, arq, avar, na, acnt, left_of[li]) ? 1 : 2;
            }
        }
        return left_state[li] == 3 ? gaps.fit_row(low_rq, &left_row[li * R], R) : (left_state[li] == 1 ? gaps.fit(low_rq, left_of[li]) : 0);
    };
    std::vector<uint32_t> gap_of_sig; uint32_t batch_no = UINT32_MAX;
    std::vector<std::vector<uint8_t>> cap_cache; std::vector<int8_t> all_cap_cache; size_t n_triples = 0, n_decided_once = 0;
    std::vector<uint32_t> bcols_off, bcols_end((size_t)ws.n, 0); std::vector<int> bcols; std::vector<uint64_t> bcols_ub; uint64_t bcols_ub_max = 0; uint32_t bcols_batch = UINT32_MAX;
    for (const TaskBatch &batch : batches) {
        batch_no++;
        auto cc = count_cols.find(batch.rq);
        if (cc == count_cols.end()) continue;
        const RequestView &brv = pb.rqs[batch.rq];
        if (!batch.limit_reached) {  // :264-271
            list_row(hqmilp::ROW_MAX, (double)batch.size, count_lhs_id(batch.rq), cc->second, -1, 0.0);
        }
        double bsize = (double)batch.size;
        std::vector<uint32_t> capped_by;  // blocked_by_unbounded
        // What a blocker leaves of every worker depends on (batch, blocker) alone — not on the cut: the workers' gaps, the columns of the workers without a gap
        // (zero_cond) and the workers with one are worked out ONCE per pair and every cut of the batch against that blocker reads them (c3p at BASELINE size:
        // 91 (cut, blocker) passes over 1024 workers -> 16).  The rows and the flag columns come out in the reference's order all the same.
        // whole: no_gap is the batch's column list as it stands; max_excess: the largest (sum of the columns' bounds - gap) over with_gap — a cut of at least that size emits no row there
        // all_gap: every solver worker carries the gap gap_all (with_gap stays empty: nothing to write down per worker)
        struct PairMemo { bool done = false, whole = false, all_gap = false; uint32_t gap_all = 0; int lhs_id = -1; int64_t max_excess = INT64_MIN; std::vector<int> no_gap; std::vector<std::pair<uint32_t, uint32_t>> with_gap; };  // with_gap: (worker, gap), ascending workers
        std::vector<PairMemo> pair_memo;
        for (const PriorityCut &cut : batch.cuts) {
            for (auto &bl : cut.blockers) {
                uint32_t brq = bl.first; bool bounded = bl.second != HQ_BLOCKER_UNBOUNDED;
                std::vector<int> no_gap_mn;  // zero_cond of a multi-node batch
                const std::vector<int> *no_gap = &no_gap_mn;
                int no_gap_id = -1;
                std::vector<int> cols;
                int fl_cached = -2;
                if (pb.rq_multi_node(batch.rq)) {
                    for (uint32_t g = 0; g < pb.n_groups; g++) {
                        auto it = group_cols.find({batch.rq, g});
                        if (it != group_cols.end() && group_can_run_rq(g, brq)) no_gap_mn.push_back(it->second);
                    }
                } else {
                    if (pair_memo.size() < pb.rqs.size()) pair_memo.resize(pb.rqs.size());
                    PairMemo &pm = pair_memo[brq];
                    if (!pm.done) {
                        pm.done = true;
                        if (cap_cache.size() < pb.rqs.size()) cap_cache.resize(pb.rqs.size());
                        std::vector<uint8_t> &cap_brq = cap_cache[brq];  // can the worker run the blocker at all (Worker::is_capable_to_run_rqv): once per request class, not per (batch, cut, blocker)
                        if (cap_brq.empty()) { cap_brq.assign(ws.n, 0); for (uint32_t w : solver_workers) cap_brq[w] = pb.capable_rqv(ws, w, brq) ? 1 : 0; }
                        if (bcols_batch != batch_no) {  // the batch's placement columns per worker and the sum of their bounds: once per batch
                            bcols_batch = batch_no; bcols_off.assign((size_t)ws.n + 1, 0); bcols.clear(); bcols_ub.assign(ws.n, 0); bcols_ub_max = 0;
                            if (runs_on) bcols.reserve((size_t)m.ncols());
                            for (uint32_t w : solver_workers) {
                                bcols_off[w] = (uint32_t)bcols.size();
                                if (runs_on && stamp_first[w] != UINT32_MAX) {   // a stamp: its run's first block's columns, moved to its own
                                    const uint32_t f = stamp_first[w]; const int d = blk_base[w] - blk_base[f];
                                    for (uint32_t i = bcols_off[f], e = bcols_end[f]; i < e; i++) { const int pc = bcols[i] + d; bcols.push_back(pc); }
                                    bcols_ub[w] = bcols_ub[f];
                                } else
                                for (uint8_t v = 0; v < brv.n_variants; v++) { const int pc = place_get(w, batch.rq, v); if (pc >= 0) { bcols.push_back(pc); bcols_ub[w] += col_ub[(size_t)pc]; } }
                                bcols_end[w] = (uint32_t)bcols.size(); bcols_ub_max = std::max(bcols_ub_max, bcols_ub[w]);
                            }
                        }
                        n_triples++;
                        if (!sigs_done) { for (uint32_t w : solver_workers) sig_of(w); sigs_done = true; }  // (every worker's signature up front: the table below is indexed by it)
                        gap_of_sig.assign(sig_rep.size(), UINT32_MAX);
                        bool all_capable = true;
                        if (runs_on) {   // once per request, like cap_brq itself
                            if (all_cap_cache.size() < pb.rqs.size()) all_cap_cache.resize(pb.rqs.size(), -1);
                            if (all_cap_cache[brq] < 0) { all_cap_cache[brq] = 1; for (uint32_t w : solver_workers) if (!cap_brq[w]) { all_cap_cache[brq] = 0; break; } }
                            all_capable = all_cap_cache[brq] != 0;
                        } else
                        if (sig_rep.size() == 1) for (uint32_t w : solver_workers) if (!cap_brq[w]) { all_capable = false; break; }
                        if (sig_rep.size() == 1 && all_capable && !solver_workers.empty()) {
                            // identical workers (a cold cluster): ONE gap for all of them — either every worker's columns go into the no-gap list (which is then the
                            // batch's column list as it stands) or every worker carries the gap
                            const uint32_t w0 = solver_workers[0];
                            const uint32_t gap = gap_of(brq, batch.rq, gap_sig[w0], w0);
                            if (runs_on) {   // (said, not written out per worker: the list is `bcols` itself, the gap one number)
                                if (gap > 0) { pm.all_gap = true; pm.gap_all = gap; pm.max_excess = (int64_t)bcols_ub_max - (int64_t)gap; } else pm.whole = true;
                            } else
                            if (gap > 0) { pm.with_gap.reserve(solver_workers.size()); for (uint32_t w : solver_workers) pm.with_gap.push_back({w, gap}); }
                            else pm.no_gap.assign(bcols.begin(), bcols.end());
                        } else {
                        pm.no_gap.reserve(bcols.size());
                        for (uint32_t w : solver_workers) {
                            if (!cap_brq[w]) continue;
                            uint32_t gap = gap_of_sig[gap_sig[w]];
                            if (gap == UINT32_MAX) gap = gap_of_sig[gap_sig[w]] = gap_of(brq, batch.rq, gap_sig[w], w);   // once per (batch, blocker, signature)
                            if (gap > 0) pm.with_gap.push_back({w, gap});
                            else pm.no_gap.insert(pm.no_gap.end(), bcols.data() + bcols_off[w], bcols.data() + bcols_end[w]);
                        }
                        }
                        auto list_of = [&](const PairMemo &q) -> const std::vector<int> & { return q.whole ? bcols : q.no_gap; };
                        if (!list_of(pm).empty()) {   // blockers that leave no gap on the same workers give the same list: one id (identical workers: every blocker of the batch)
                            // (two lists that are both the batch's column list as it stands are equal by construction, not by comparison)
                            for (const PairMemo &o : pair_memo) if (&o != &pm && o.lhs_id >= 0 && ((o.whole && pm.whole) || list_of(o) == list_of(pm))) { pm.lhs_id = o.lhs_id; break; }
                            if (pm.lhs_id < 0) pm.lhs_id = next_lhs_id++;
                        }
                        if (runs_on) for (auto &wg : pm.with_gap) pm.max_excess = std::max(pm.max_excess, (int64_t)bcols_ub[wg.first] - (int64_t)wg.second);
                    }
                    no_gap = pm.whole ? &bcols : &pm.no_gap; no_gap_id = pm.lhs_id;
                    // The pass below emits a row for a worker only where the sum of its columns' bounds exceeds cut.size + gap: decided ONCE for the pair where no worker's
                    // does (equal workers share both figures).  The flag column is still created at this moment, as the pass would at its first worker.
                    auto gap_rows = [&](const uint32_t w, const uint32_t gap) {
                        const int *wc = bcols.data() + bcols_off[w]; const size_t nwc = bcols_end[w] - bcols_off[w];
                        const uint64_t cols_ub = bcols_ub[w];
                        // (a row no point within the columns' own bounds can violate is not emitted: with cuts in the thousands and workers that hold
                        // a hundred tasks that is every one of the W x cuts x blockers rows of a large tick — the model's points are the same)
                        // The flag column itself is created as the reference creates it (get_bvar, :233-253: even for a worker without a placement
                        // column) — the model's COLUMNS, and with them the canonical tie-break, stay exactly the reference's.
                        if (bounded && fl_cached == -2) fl_cached = short_flag(brq, bl.second);  // (created at its first use, as get_bvar does; the same flag for every worker of this pair)
                        const int fl = bounded ? fl_cached : -1;
                        if (cols_ub <= (uint64_t)cut.size + gap) return;
                        if (bounded && fl >= 0) { cols.assign(wc, wc + nwc); emit_plus(hqmilp::ROW_MAX, (double)cut.size + bsize + (double)gap, cols, fl, bsize); }
                        else if (!bounded) { m.begin_row(hqmilp::ROW_MAX, (double)cut.size + (double)gap); for (size_t k = 0; k < nwc; k++) m.term(wc[k], 1.0); m.end_row(); }
                    };
                    if (runs_on && (pm.all_gap || !pm.with_gap.empty()) && pm.max_excess <= (int64_t)cut.size) {
                        if (bounded) fl_cached = short_flag(brq, bl.second);
                        n_decided_once++;
                    } else if (pm.all_gap) for (uint32_t w : solver_workers) gap_rows(w, pm.gap_all);
                    else for (auto &wg : pm.with_gap) gap_rows(wg.first, wg.second);
                }
                if (no_gap->empty()) continue;
                int fl;
                if (bounded && (fl = short_flag(brq, bl.second)) >= 0) list_row(hqmilp::ROW_MAX, bsize + (double)cut.size, no_gap_id, *no_gap, fl, bsize);
                else if (!bounded && std::find(capped_by.begin(), capped_by.end(), brq) == capped_by.end()) {
                    capped_by.push_back(brq);
                    list_row(hqmilp::ROW_MAX, (double)cut.size, no_gap_id, *no_gap, -1, 0.0);
                }
            }
        }
    }

    if (!seq_start.empty()) {
        m.start.assign(m.ncols(), 0.0);
        for (const SeqStart &ss : seq_start) {
            const int pc = place_get(ss.w, batches[ss.batch].rq, ss.variant);
            if (pc < 0) { m.start.clear(); break; }
            m.start[pc] = ss.count;
        }
    }
    m.row_implied.resize(m.nrows(), 0);
    m.row_lhs.resize((size_t)m.nrows(), -1); m.row_lhs_len.resize((size_t)m.nrows(), 0); m.row_block.resize((size_t)m.nrows(), -1);
    m.col_ub = col_ub; m.col_ub.resize((size_t)m.ncols(), UINT32_MAX);
    if (hqmilp::g_probe) {   // tests: every array of the model, and what was said about its runs
        using hqmilp::fnv1a_vec;
        uint64_t h = hqmilp::FNV_BASIS;
        h = fnv1a_vec(h, m.obj); h = fnv1a_vec(h, m.kind); h = fnv1a_vec(h, m.rtype); h = fnv1a_vec(h, m.rhs); h = fnv1a_vec(h, m.roff); h = fnv1a_vec(h, m.rcol); h = fnv1a_vec(h, m.rcoef);
        h = fnv1a_vec(h, m.start); h = fnv1a_vec(h, m.col_group); h = fnv1a_vec(h, m.row_implied); h = fnv1a_vec(h, m.row_lhs); h = fnv1a_vec(h, m.row_lhs_len);
        h = fnv1a_vec(h, m.list_off); h = fnv1a_vec(h, m.list_col); h = fnv1a_vec(h, m.row_block); h = fnv1a_vec(h, m.col_ub);
        hqmilp::g_probe->model = h; hqmilp::g_probe->runs = m.block_runs.size(); hqmilp::g_probe->tables = 0; hqmilp::g_probe->covered = 0;
    }
    const double t_model1 = clock_us();
    if (trace_model) {
        size_t run_blocks = 0; for (const auto &br : m.block_runs) run_blocks += (size_t)br.n_blocks;
        fprintf(stderr, "[model] cuts done at %.3f ms: %d columns, %d rows, %zu terms, %zu worker signatures, %zu (batch, cut, blocker) passes over the workers; %zu equal-block runs over %zu blocks, %zu (cut, blocker) passes decided once\n", (t_model1 - t_model0) / 1e3, m.ncols(), m.nrows(), m.rcol.size(), sig_rep.size(), n_triples, m.block_runs.size(), run_blocks, n_decided_once);
    }
    hqmilp::SolveOpts opts; opts.no_fast_path = pb.no_fast_path; opts.defer_row_check = pb.defer_row_check;
    hqmilp::Result sol = hqmilp::solve(m, pb.time_limit_s, !pb.certificate_only, hqmilp::REFERENCE_MIP_REL_GAP, pb.pricer, &opts);  // :432-438
    if (trace_model) fprintf(stderr, "[model] solve done %.3f ms after the model\n", (clock_us() - t_model1) / 1e3);
    out.pre_us = t_model0 - t_enter; out.model_us = t_model1 - t_model0; out.milp_us = clock_us() - t_model1; out.price_sweeps = sol.price_sweeps; out.price_rounds = sol.price_rounds; out.price_us = sol.price_total_us;
    out.milp_nodes = sol.nodes; out.milp_cols = m.ncols(); out.milp_rows = m.nrows(); out.milp_components = sol.n_components;
    if (!sol.feasible) return out;
    out.is_optimal = sol.optimal;
    out.is_canonical = sol.canonical && sol.optimal;

    // decode  :439-481; Map iteration orders via hb_order.h
    std::vector<uint64_t> key_hash; std::vector<std::pair<uint32_t, uint8_t>> key_list; std::vector<std::vector<std::pair<uint32_t, uint32_t>>> key_counts;
    std::vector<uint64_t> mn_hash; std::vector<uint32_t> mn_list; std::vector<std::vector<std::vector<uint32_t>>> mn_sets;
    std::vector<uint32_t> dec_ids, dec_widx, dec_cnt;
    for (const TaskBatch &batch : batches) {
        const RequestView &rv = pb.rqs[batch.rq];
        if (pb.rq_multi_node(batch.rq)) {
            size_t n_nodes = pb.variants[rv.first_variant].n_nodes;
            std::vector<std::vector<uint32_t>> sets;
            for (uint32_t w : solver_workers) {
                const int pc = place_get(w, batch.rq, 0);
                if (pc < 0 || (uint32_t)std::round(sol.x[pc]) == 0) continue;
                if (!sets.empty() && sets.back().size() < n_nodes) sets.back().push_back(w); else sets.push_back({w});
            }
            if (!sets.empty()) { mn_hash.push_back(hqhb::hash_rq_variant(batch.rq, 0)); mn_list.push_back(batch.rq); mn_sets.push_back(sets); }
        } else {
            for (uint8_t v = 0; v < rv.n_variants; v++) {
                // the key's workers with a non-zero count, in solver order: every worker's triple is written, the cursor advances on a non-zero count (no push_back, no
                // libm round per (worker, key) pair — the point is integral to 1e-9 and not negative: x + 0.5 truncated is the same integer)
                const size_t nsw = solver_workers.size();
                dec_ids.resize(nsw + 1); dec_widx.resize(nsw + 1); dec_cnt.resize(nsw + 1);
                uint32_t *idp = dec_ids.data(), *wxp = dec_widx.data(), *cp = dec_cnt.data(); size_t nk = 0;
                const int *pcol = place_col.data() + rv.first_variant + v;
                const double *xs = sol.x.data();
                for (size_t i = 0; i < nsw; i++) {
                    const uint32_t w = solver_workers[i];
                    const int pc = pcol[(size_t)w * NVS];
                    const double xv = pc >= 0 ? xs[pc] : 0.0;
                    const uint32_t c = xv > 0.0 ? (uint32_t)(xv + 0.5) : 0u;
                    idp[nk] = ws.id[w]; wxp[nk] = w; cp[nk] = c; nk += c > 0 ? 1 : 0;
                }
                if (nk == 0) continue;
                dec_ids.resize(nk);
                const std::vector<uint32_t> &ids = dec_ids, &widx = dec_widx, &cnt = dec_cnt;
                const std::vector<uint32_t> &word = cached_worker_order(ids);
                std::vector<std::pair<uint32_t, uint32_t>> ordered; ordered.reserve(word.size());
                for (uint32_t k : word) ordered.push_back({widx[k], cnt[k]});
                key_hash.push_back(hqhb::hash_rq_variant(batch.rq, v)); key_list.push_back({batch.rq, v}); key_counts.push_back(std::move(ordered));
            }
        }
    }
    std::vector<uint32_t> ord;
    hqhb::insertion_order(key_hash.data(), (uint32_t)key_hash.size(), ord);
    for (uint32_t k : ord) { out.keys.push_back(key_list[k]); out.per_key.push_back(std::move(key_counts[k])); }
    hqhb::insertion_order(mn_hash.data(), (uint32_t)mn_hash.size(), ord);
    for (uint32_t k : ord) { out.mn_rq.push_back(mn_list[k]); out.mn_sets.push_back(std::move(mn_sets[k])); }
    if (trace_model) fprintf(stderr, "[model] decoded %.3f ms after the model, %.3f ms after the solver was entered\n", (clock_us() - t_model1) / 1e3, (clock_us() - t_enter) / 1e3);
    if (sol.row_check.pending) { out.row_check.check = std::move(sol.row_check); out.row_check.model = std::move(m); }  // (the check reads the model: it goes along, nothing is copied)
    return out;
}

}  // namespace hqhost
