// The coupled placement solve by price sweeps: host side (see price.h for the method, price_core.h for what one sweep does per block).  The solve itself:
// master, Kelley loop, rounding, branch-and-price — on the problem that price_flatten.cpp leaves (price_prob.h).
#include "price_prob.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>

#include "lp_tab.h"
#include "milp.h"

namespace hqprice {
namespace {

using hqmilp::lp::BASIC;
using hqmilp::lp::INF;
using hqmilp::lp::LP_OPT;
using hqmilp::lp::Rows;
using hqmilp::lp::Tab;

static_assert(UNBOUNDED == INF, "price_prob.h restates lp_tab.h's INF");
constexpr double FIRST_PROPOSAL_SCALE = 1.0 / 16.0;   // kelley(): what is evaluated of the first master's proposal (see there)
constexpr int MAX_ROUNDS = 6;
constexpr int BP_MAX_NODES = 600;   // nodes of the branch-and-price phase (a deterministic count, like every limit in here)
// (per second of the caller's configured time limit: generous — what keeps the phase inside the limit is its wall-clock guard at 70 % of it)
constexpr double BP_MAX_STEPS = 3.0e6;   // ... and search steps of the slowest blocks summed over the sweeps (0.3-1 us each: see Solver::sweep_steps)
constexpr double BP_MAX_WORK = 3.0e9; // ... and tableau elements its masters may touch (lp_tab.h's `ops`: ~1e9 per second): with thousands of cuts in the master a node
                                      // costs milliseconds, and a 10 k-column model spent 8 s here against a 5 s time limit before this cap (deterministic like the counts)

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
thread_local uint32_t g_early_sweeps = 0;   // tests: sweeps launched on the block tables alone (Solver::launch_on_blocks)

struct Cut {
    double cx = 0, bnd = 0; std::vector<long long> act; std::vector<double> pi;
    // the maximisers, one integer pattern per block, in the model's own variables: fetched from the device on demand (the sweep solved in variables shifted by `lo`)
    std::vector<uint16_t> x; bool fetched = false; std::vector<std::pair<uint32_t, int32_t>> lo;
    // the same per part of the model (PARTS contiguous ranges of blocks): the root master keeps one value function per part
    std::vector<double> pcx; std::vector<long long> pact;  // [PARTS], [PARTS * K]
};

// a node of the branch-and-price phase: flags fixed or free, bounds on single block columns
struct BPNode { std::vector<int8_t> flag; std::vector<std::pair<uint32_t, int32_t>> lo, hi; double bound = INF; int depth = 0; };

struct Solver {
    const Request &rq; Sweeper &sw; Prob P;
    std::vector<Cut> cuts;
    double relaxed_bound = INF;   // min over every evaluated pi of the Lagrangian with the flags relaxed to [0, 1]
    std::vector<double> relaxed_pi;
    double theta_scale = 1.0;
    std::vector<double> pmax;
    bool failed = false;
    size_t cut_lo = 0;            // the master works on cuts[cut_lo ..): points evaluated under the column bounds now in force
    double work = 0.0;            // tableau elements touched by the masters so far (Tab::ops)
    // What the sweeps themselves cost, in the kernel's own unit: a sweep lasts as long as its slowest block, ~1 us per search step on top of ~60 us.  Blocks that
    // run out of their step budget return an LP bound instead of their optimum: the total stays a valid bound, but the master's cuts (patterns) and its evaluations
    // (bounds) no longer describe the same function and the cutting-plane loop stops converging — a model whose blocks do that sweep after sweep (16-column blocks of a
    // busy C4 cluster) is not one for this path.
    double sweep_steps = 0.0; int budget_sweeps = 0;
    int max_sweeps = 256;
    // branch-and-price: the node whose bounds the device tables carry right now (empty lo list = the model's own bounds), and what its lower bounds add per sweep
    std::vector<std::pair<uint32_t, int32_t>> node_lo, node_caps; double node_cl = 0.0; std::vector<double> node_Al; bool at_root = true;
    bool base_caps = true;        // the sweeps run under the model's own column bounds (only those bound the relaxed model)
    // The zero-price sweep launched from inside the flattening, on the block tables alone (price.h: Sweeper::begin_blocks; solve_model's hook).
    enum { EARLY_NONE = 0, EARLY_LAUNCHED, EARLY_REFUSED, EARLY_FAILED };
    int early = EARLY_NONE;
    bool early_begun = false;     // begin_blocks took the tables: the sweeper is owed an end()
    bool host_acts = false;       // the sweep in flight ran without the wide rows' entries: its activities are added up here, from its patterns
    double tp0 = 0.0;             // start of the solve (the trace's clock)
    Solver(const Request &r, Sweeper &s) : rq(r), sw(s) {}

    // what a solve sets on its sweeper before the first sweep
    void prepare_sweeper() {
        sw.stat_sweeps = 0; sw.stat_sweep_us = 0;
        sw.guard_s = rq.deadline_s - 0.3 * rq.time_limit_s; sw.time_up = false;  // (first read at the first sweep)
        max_sweeps = (int)std::min<size_t>(4096, std::max<size_t>(256, ((size_t)64 << 20) / ((size_t)P.T.n_cols * 2 + 1)));  // the device keeps every sweep's patterns: at most 64 MB of them
    }
    // The flattener's hook: P.T's block arrays are final (n_blocks, n_cols, blk_off, blk_m, blk_cap, col_cost, col_a, col_cap), nothing else of P is.  At zero prices
    // that is all a sweep needs: it is on the device while the host builds the wide rows' tables.
    void launch_on_blocks() {
        prepare_sweeper();
        const int took = sw.begin_blocks(P.T, (uint32_t)max_sweeps);
        if (took < 0) return;   // (a sweeper without the split: begin() and the launch once the model is flattened)
        if (took == 0) { early = EARLY_REFUSED; return; }
        early_begun = true;
        const double zero = 0.0, t0 = now_us();
        sw.pending_k = 0;
        if (!sw.sweep_launch(&zero)) { early = EARLY_FAILED; return; }
        sw.stat_sweep_us += now_us() - t0;
        early = EARLY_LAUNCHED; host_acts = true; g_early_sweeps++;
        if (rq.trace) fprintf(stderr, "[price] first sweep (prices 0) launched on the block tables at %.3f ms\n", (now_us() - tp0) / 1e3);
    }
    // The activities of a sweep that ran without the wide rows' entries: sum coef . x over its patterns (read where the sweep left them) and the column-wise entries,
    // per part and in total — the integers the device's 64-bit atomics add up, which are exact and order-free.
    bool activities_from_patterns(uint32_t sweep, SweepTotals &tot) {
        const HostTables &T = P.T;
        const uint16_t *x = sw.patterns(sweep, 1);
        if (!x) return false;
        const size_t KG = (size_t)P.KG;
        const uint32_t per = (T.n_blocks + PARTS - 1) / PARTS;
        tot.act.assign(KG, 0); tot.part_act.assign((size_t)PARTS * KG, 0);
        const uint32_t *woff = T.col_woff.data(); const uint16_t *wr = T.w_row.data(); const int32_t *wc = T.w_coef.data();
        for (uint32_t b = 0; b < T.n_blocks; b++) {
            long long *pa = &tot.part_act[(size_t)(b / per) * KG];
            for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) {
                const long long xv = (long long)x[f];
                if (!xv) continue;
                for (uint32_t e = woff[f]; e < woff[f + 1]; e++) pa[wr[e]] += (long long)wc[e] * xv;
            }
        }
        for (int p = 0; p < PARTS; p++) for (size_t k = 0; k < KG; k++) tot.act[k] += tot.part_act[(size_t)p * KG + k];
        return true;
    }

    // one sweep at pi; returns the cut's index or -1.  In two halves for the caller with work to do meanwhile: evaluate_launch(pi), ..., evaluate(pi, true).
    bool evaluate_launch(const std::vector<double> &pi) {
        if ((int)cuts.size() >= max_sweeps) return false;
        std::vector<double> pig(P.KG, 0.0);
        for (int k = 0; k < P.K; k++) pig[P.grp_of[k]] += pi[k];
        const double t0 = now_us();
        sw.pending_k = (uint32_t)P.KG;
        if (!sw.sweep_launch(pig.data())) { failed = true; return false; }
        sw.stat_sweep_us += now_us() - t0;
        return true;
    }
    int evaluate(const std::vector<double> &pi, bool launched = false) {
        if ((int)cuts.size() >= max_sweeps) return -1;
        SweepTotals tot;
        const double t0 = now_us();
        if (launched) {
            if (!sw.sweep_finish(tot)) { failed = true; return -1; }
            if (host_acts) { host_acts = false; if (!activities_from_patterns((uint32_t)cuts.size(), tot)) { failed = true; return -1; } }
        } else {
            std::vector<double> pig(P.KG, 0.0);
            for (int k = 0; k < P.K; k++) pig[P.grp_of[k]] += pi[k];
            if (!sw.sweep(pig.data(), tot)) { failed = true; return -1; }
        }
        sw.stat_sweep_us += now_us() - t0; sw.stat_sweeps++;
        if (!sw.merges_clock() && now_us() * 1e-6 > sw.guard_s) sw.time_up = true;  // (a sharded sweeper has merged the ranks' readings inside sweep(): a local reading here could split the replicas)
        sweep_steps += 64.0 + (double)tot.max_steps;
        if (tot.n_budget > std::max<uint32_t>(4, P.T.n_blocks / 64)) budget_sweeps++;
        Cut c; c.cx = tot.cx; c.bnd = tot.bnd; c.pi = pi;
        c.act.resize(P.K);
        for (int k = 0; k < P.K; k++) c.act[k] = tot.act[P.grp_of[k]];
        if (node_lo.empty() && tot.part_cx.size() == (size_t)PARTS && tot.part_act.size() == (size_t)PARTS * P.KG) {
            c.pcx = tot.part_cx; c.pact.resize((size_t)PARTS * P.K);
            for (int p = 0; p < PARTS; p++) for (int k = 0; k < P.K; k++) c.pact[(size_t)p * P.K + k] = tot.part_act[(size_t)p * P.KG + P.grp_of[k]];
        }
        if (!node_lo.empty()) {  // the sweep ran in variables shifted by the node's lower bounds: back to the model's own (c.l, A.l and the bound's (c - pi A).l)
            c.lo = node_lo; c.cx += node_cl; c.bnd += node_cl;
            for (int k = 0; k < P.K; k++) { c.act[k] += (long long)std::llround(node_Al[k]); c.bnd -= pi[k] * node_Al[k]; }
        }
        cuts.push_back(std::move(c));
        // the model's bound at these prices, flags relaxed: pi.h + sum_w V_w(pi) + sum_g max(0, c_g - pi.A_g)
        double L = cuts.back().bnd;
        for (int k = 0; k < P.K; k++) L += pi[k] * P.h[k];
        for (int g = 0; g < P.G; g++) { double r = P.gcost[g]; for (auto &t : P.g_rows[g]) r -= pi[t.first] * t.second; if (r > 0.0) L += r; }
        if (base_caps && at_root && L < relaxed_bound) { relaxed_bound = L; relaxed_pi = pi; }
        return (int)cuts.size() - 1;
    }
    double fixed_value(const Cut &c, const std::vector<double> &hB, double cB) const {
        double L = c.bnd + cB;
        for (int k = 0; k < P.K; k++) L += c.pi[k] * hB[k];
        return L;
    }

    // Cutting-plane master (Kelley) for the model with its flags fixed: minimise pi.hB + theta over theta + pi.act_k >= cx_k.  Returns false when the
    // configuration cannot beat `cutoff` (or is infeasible); on success `lambda` holds the master's multipliers of the cuts (summing to 1) and pi_out
    // the final prices.
    //
    // The master is DISAGGREGATED over the model's parts: sum_w V_w(pi) is a sum over PARTS contiguous ranges of workers, every sweep returns each part's
    // own c.x and activities, and the master keeps one theta per part — its model of the dual function is the sum of PARTS piecewise-linear models
    // instead of one, which takes a third of the sweeps to the same accuracy (the first wave of the layered config-5 DAG: 61 -> 19-22).  The workers
    // are in objective order (factor (W - idx) / W, solver.rs:542-571), so contiguous ranges are the parts that differ most from one another.
    //
    // `probe` (optional; called after a master round that is within 10 %, at most three times): shown the master's fractional point — the columns' activities in every wide row — and its
    // lower bound; true = the caller goes to another configuration, this walk ends (false is returned).  `no_sweeps`: only what the cuts at hand settle — false as
    // soon as the master would need another sweep.
    // Starting prices from the model AGGREGATED over chunks of its blocks (round 6).  Where the blocks of a part are the same block up to their costs — a cluster of identical
    // workers: every cold tick, every DAG tick on an idle cluster — the part is one block with `count` times the capacities and the mean cost, and the model is an LP of
    // PARTS x (columns of a block) variables under the priced wide rows: a hundred microseconds of dual simplex.  Its duals of the wide rows are where the decomposition's
    // prices end up, up to what integrality and the cost spread inside a part change — a far better first proposal than a fraction of the price caps.  A proposal like any
    // other (the cut it yields is exact); false: the blocks of some part differ, the caller keeps its scaled proposal.
    bool aggregate_prices(const std::vector<double> &hB, const std::vector<int> &lk, std::vector<double> &pi) {
        const HostTables &T = P.T;
        // chunks of blocks = the aggregated model's granularity: as fine as ~256 LP variables allow (the dense dual simplex of lp_tab.h: ~0.1 ms there, milliseconds at 1024) —
        // 32 chunks of eight-column blocks, 16 of sixteen-column ones.  Measured in sweeps (emulated, deterministic): config-5 first wave 10 -> 7, the 20 % probe 15 -> 11,
        // configs[3]'s unsaturated cluster 19 -> 16; with 64 chunks 7 / 10 / 14, at ten times the LP.
        static const int chunks_env = getenv("HQPRICE_AGG_CHUNKS") ? atoi(getenv("HQPRICE_AGG_CHUNKS")) : 0;
        uint32_t widest = 1;
        for (uint32_t b = 0; b < T.n_blocks; b++) widest = std::max(widest, T.blk_off[b + 1] - T.blk_off[b]);
        const int agg_chunks = chunks_env > 0 ? chunks_env : std::min(64, std::max(PARTS, (int)(256u / widest)));
        const uint32_t nb = T.n_blocks, per = (nb + (uint32_t)agg_chunks - 1) / (uint32_t)agg_chunks;
        const int NP = (int)((nb + per - 1) / per), KL = (int)lk.size();
        if (NP < 2 || KL == 0) return false;
        // Only where a sweep is expensive: the aggregated LP (~256 variables through the dense dual simplex) costs ~1 ms on the MI355X box's host — three sweeps of a
        // 4096-block model, a dozen of a 1024-block one.  (Measured with it on everywhere: layered DAG loop 17 -> 14 sweeps but 2.00 -> 2.13 ms per tick; configs[3]'s
        // unsaturated cluster 19 -> 16 sweeps and 8.8 -> 7.6 ms.)
        static const uint64_t min_cols_env = getenv("HQPRICE_AGG_MINCOLS") ? (uint64_t)atoll(getenv("HQPRICE_AGG_MINCOLS")) : 32768;   // (experiments)
        if ((uint64_t)T.n_cols < min_cols_env) return false;
        if (P.G != 0) return false;   // (models with flags: the aggregated duals of one configuration mislead the walk over configurations — c3p 3 -> 4 sweeps, c4p 9 -> 16)
        std::vector<uint32_t> pb0(NP), pcnt(NP), pnc(NP), voff(NP + 1, 0);
        for (int p = 0; p < NP; p++) {
            const uint32_t b0 = (uint32_t)p * per, b1 = std::min(nb, b0 + per);
            pb0[p] = b0; pcnt[p] = b1 - b0; pnc[p] = T.blk_off[b0 + 1] - T.blk_off[b0];
            const uint32_t c0 = T.blk_off[b0], nc = pnc[p];
            for (uint32_t b = b0 + 1; b < b1; b++) {   // the same block? (amounts, bounds, capacities, membership in the wide rows — everything but the costs)
                const uint32_t c = T.blk_off[b];
                if (T.blk_off[b + 1] - c != nc || T.blk_m[b] != T.blk_m[b0]) return false;
                if (memcmp(&T.blk_cap[(size_t)b * MMAX_BLOCK], &T.blk_cap[(size_t)b0 * MMAX_BLOCK], sizeof(double) * MMAX_BLOCK) != 0) return false;
                if (memcmp(&T.col_a[(size_t)c * MMAX_BLOCK], &T.col_a[(size_t)c0 * MMAX_BLOCK], sizeof(double) * MMAX_BLOCK * nc) != 0) return false;
                if (memcmp(&T.col_cap[c], &T.col_cap[c0], sizeof(int32_t) * nc) != 0) return false;
                for (uint32_t q = 0; q < nc; q++) {
                    const uint32_t e0 = T.col_woff[c0 + q], e1 = T.col_woff[c0 + q + 1], f0 = T.col_woff[c + q];
                    if (T.col_woff[c + q + 1] - f0 != e1 - e0) return false;
                    if (e1 > e0 && (memcmp(&T.w_row[f0], &T.w_row[e0], sizeof(uint16_t) * (e1 - e0)) != 0 || memcmp(&T.w_coef[f0], &T.w_coef[e0], sizeof(int32_t) * (e1 - e0)) != 0)) return false;
                }
            }
            voff[p + 1] = voff[p] + nc;
        }
        const int nv = (int)voff[NP];
        if (nv == 0 || nv > 8192) return false;
        Rows A; A.n = nv;
        std::vector<double> ac(nv), alb(nv, 0.0), aub(nv);
        std::vector<std::pair<int, double>> terms;
        for (int p = 0; p < NP; p++) {
            const uint32_t c0 = T.blk_off[pb0[p]], nc = pnc[p];
            for (uint32_t q = 0; q < nc; q++) {
                double sum = 0.0;
                for (uint32_t b = 0; b < pcnt[p]; b++) sum += T.col_cost[T.blk_off[pb0[p] + b] + q];
                ac[voff[p] + q] = sum / (double)pcnt[p] / theta_scale;
                aub[voff[p] + q] = (double)pcnt[p] * (double)T.col_cap[c0 + q];
            }
            for (int r = 0; r < (int)T.blk_m[pb0[p]]; r++) {
                terms.clear(); double sc = 0.0;
                for (uint32_t q = 0; q < nc; q++) { const double a = T.col_a[(size_t)(c0 + q) * MMAX_BLOCK + r]; if (a != 0.0) { terms.push_back({(int)(voff[p] + q), a}); sc = std::max(sc, std::fabs(a)); } }
                if (terms.empty()) continue;
                for (auto &t : terms) t.second /= sc;
                A.add(terms, -INF, (double)pcnt[p] * T.blk_cap[(size_t)pb0[p] * MMAX_BLOCK + r] / sc);
            }
        }
        const int first_wide = A.m;
        std::vector<double> wscale(KL, 1.0);
        for (int i = 0; i < KL; i++) {
            const int g = P.grp_of[lk[i]];
            terms.clear(); double sc = 0.0;
            for (int p = 0; p < NP; p++) {
                const uint32_t c0 = T.blk_off[pb0[p]];
                for (uint32_t q = 0; q < pnc[p]; q++) for (uint32_t e = T.col_woff[c0 + q]; e < T.col_woff[c0 + q + 1]; e++) if ((int)T.w_row[e] == g) { terms.push_back({(int)(voff[p] + q), (double)T.w_coef[e]}); sc = std::max(sc, std::fabs((double)T.w_coef[e])); }
            }
            if (terms.empty()) { A.add({{0, 0.0}}, -INF, INF); continue; }
            for (auto &t : terms) t.second /= sc;
            wscale[i] = sc;
            A.add(terms, -INF, hB[lk[i]] / sc);
        }
        Tab at; at.init(&A, ac, alb, aub);
        if (at.solve(20000) != LP_OPT) return false;
        work += at.ops;
        pi.assign(P.K, 0.0);
        bool any = false;
        for (int i = 0; i < KL; i++) {
            const int a = at.where[first_wide + i];
            if (a < 0 || at.st[A.n + a] == BASIC) continue;
            double y = std::fabs(at.d[A.n + a]) / wscale[i] * theta_scale;   // the row's dual, back in the units of the prices (cost per unit of the row's activity)
            if (!(y > 0.0)) continue;
            pi[lk[i]] = std::min(y, pmax[lk[i]]);
            any = true;
        }
        return any;
    }

    std::function<bool(const std::vector<double> &, double)> probe;
    // what a no_sweeps walk that converged found: the caller goes to that configuration next, whose own walk would solve the same master again
    struct Settled { bool valid = false; std::vector<double> hB, lambda, pi; double cB = 0.0, bound = 0.0; size_t n_cuts = 0, cut_lo = 0; } settled;
    bool kelley(const std::vector<double> &hB, double cB, double cutoff, double tol, std::vector<double> &lambda, std::vector<double> &pi_out, double *bound_out, bool no_sweeps = false) {
        if (!no_sweeps && settled.valid) {
            settled.valid = false;
            if (settled.n_cuts == cuts.size() && settled.cut_lo == cut_lo && settled.cB == cB && settled.hB == hB) {
                if (settled.bound < cutoff) return false;
                lambda = std::move(settled.lambda); pi_out = std::move(settled.pi); *bound_out = settled.bound;
                return true;
            }
        }
        const int K = P.K;
        const uint32_t per = (P.T.n_blocks + PARTS - 1) / PARTS;
        const int NP = (int)((P.T.n_blocks + per - 1) / per);  // parts that hold blocks
        // With the flags fixed, the rows of one group are ONE left-hand side against several right-hand sides: only the tightest can bind, the others get price 0.  The
        // master prices that one row per group (a three-level tick: 16 of 70 rows — a tableau a third as wide, and none of its degenerate ties among identical columns).
        std::vector<int> lk; lk.reserve(P.KG);
        for (int g = 0; g < P.KG; g++) {
            int best = -1;
            for (int q = P.gr_off[g]; q < P.gr_off[g + 1]; q++) { const int k = P.gr_row[q]; if (best < 0 || hB[k] < hB[best]) best = k; }
            if (best >= 0) lk.push_back(best);
        }
        std::sort(lk.begin(), lk.end());
        const int KL = (int)lk.size();
        Rows M; M.n = KL + NP;
        std::vector<double> mc(KL + NP), mlb(KL + NP, 0.0), mub(KL + NP);
        for (int i = 0; i < KL; i++) { mc[i] = -hB[lk[i]] / theta_scale; mub[i] = pmax[lk[i]]; }
        for (int p = 0; p < NP; p++) { mc[KL + p] = -1.0; mub[KL + p] = 4.0; }
        std::vector<double> cut_scale;
        std::vector<std::pair<int, double>> terms;
        size_t in_master = cut_lo;
        auto push_cuts = [&](Tab *mt) {
            for (; in_master < cuts.size(); in_master++) {
                const Cut &c = cuts[in_master];
                for (int p = 0; p < NP; p++) {
                    terms.clear(); double sc = 1.0;
                    for (int i = 0; i < KL; i++) { const long long a = c.pact[(size_t)p * K + lk[i]]; if (a != 0) { const double v = (double)a / theta_scale; terms.push_back({i, v}); sc = std::max(sc, std::fabs(v)); } }
                    terms.push_back({KL + p, 1.0});
                    for (auto &t : terms) t.second /= sc;
                    M.add(terms, c.pcx[p] / theta_scale / sc, INF);
                    cut_scale.push_back(sc);
                    if (mt) mt->where.push_back(-1);
                }
            }
        };
        for (size_t k = cut_lo; k < cuts.size(); k++) if (cuts[k].pcx.empty()) { if (rq.trace) fprintf(stderr, "[price] master: cut %zu without part sums\n", k); return false; }  // (a sweeper without part sums: cannot happen with the two in this tree)
        push_cuts(nullptr);
        Tab mt; mt.init(&M, mc, mlb, mub);
        double ub_best = INF; std::vector<double> pi_best(K, 0.0);
        for (size_t k = cut_lo; k < cuts.size(); k++) { const double L = fixed_value(cuts[k], hB, cB); if (L < ub_best) { ub_best = L; pi_best = cuts[k].pi; } }
        std::vector<double> pi(K, 0.0), pi_prev_master;
        double lb_master = -INF, lp_us = 0.0;
        bool converged = false; int probes = 0;
        // multipliers per (cut, part) of the master as it stands (after a solve): every part's sum to 1
        auto multipliers = [&](std::vector<double> &lambda) {
            lambda.assign(cuts.size() * PARTS, 0.0);
            std::vector<double> lsum(NP, 0.0);
            for (size_t r = 0; r / NP + cut_lo < cuts.size() && r < (size_t)M.m; r++) {
                const int a = mt.where[r];
                if (a < 0 || mt.st[M.n + a] == BASIC) continue;
                const size_t k = r / NP + cut_lo; const int p = (int)(r % NP);
                const double v = std::fabs(mt.d[M.n + a]) / cut_scale[r];
                lambda[k * PARTS + p] = v; lsum[p] += v;
            }
            for (int p = 0; p < NP; p++) if (!(lsum[p] > 0.0)) {
                // no cut of the part binds: its theta sits on its bound 0 — at the final prices the part's workers take nothing (or nothing worth anything).
                // Its point is the pattern of the cut that is worth most at those prices.
                size_t bk = cut_lo; double bv = -INF;
                for (size_t k = cut_lo; k < cuts.size(); k++) {
                    double v = cuts[k].pcx[p];
                    for (int i = 0; i < KL; i++) v -= mt.x[i] * (double)cuts[k].pact[(size_t)p * K + lk[i]];
                    if (v > bv) { bv = v; bk = k; }
                }
                lambda[bk * PARTS + p] = 1.0; lsum[p] = 1.0;
            }
            for (size_t k = cut_lo; k < cuts.size(); k++) for (int p = 0; p < NP; p++) lambda[k * PARTS + p] /= lsum[p];
        };
        for (int it = 0; it < 200; it++) {
            { const double tl0 = now_us(); const int st = mt.solve(200000); lp_us += now_us() - tl0; if (st != LP_OPT) { if (rq.trace) fprintf(stderr, "[price] master LP status %d at iteration %d (%d cuts)\n", st, it, M.m); return false; } }
            lb_master = -mt.objective() * theta_scale + cB;
            if (ub_best < cutoff) { if (rq.trace) fprintf(stderr, "[price] configuration bounded by %.9f, below the incumbent %.9f\n", ub_best, cutoff); return false; }  // even the relaxation of this configuration is below the incumbent
            if (ub_best - lb_master <= tol * std::fabs(ub_best)) { converged = true; break; }
            if (no_sweeps) return false;
            if (probe && probes < 3 && it >= 1 && ub_best - lb_master <= 0.1 * std::fabs(ub_best)) {
                probes++;
                std::vector<double> lam, colact(K, 0.0);
                multipliers(lam);
                for (size_t k = cut_lo; k < cuts.size(); k++) for (int p = 0; p < NP; p++) {
                    const double l = lam[k * PARTS + p];
                    if (l == 0.0) continue;
                    const long long *pa = &cuts[k].pact[(size_t)p * K];
                    for (int r = 0; r < K; r++) colact[r] += l * (double)pa[r];
                }
                auto keep = std::move(probe); probe = nullptr;   // (the probe runs a master of its own: not this one's again)
                const bool go = keep(colact, lb_master);
                probe = std::move(keep);
                if (go) return false;
            }
            bool same = !pi_prev_master.empty();
            for (int i = 0; i < KL && same; i++) same = std::fabs(mt.x[i] - pi_prev_master[i]) <= 1e-15 + 1e-12 * std::fabs(mt.x[i]);
            pi_prev_master.assign(mt.x.begin(), mt.x.begin() + KL);
            const double alpha = (it < 3 || same) ? 0.0 : 0.3;       // in-out: between the best point so far and the master's proposal
            for (int k = 0; k < K; k++) pi[k] = alpha * pi_best[k];
            for (int i = 0; i < KL; i++) pi[lk[i]] += (1.0 - alpha) * mt.x[i];
            // The very first master has one cut (the patterns at pi = 0) and nothing that holds its prices back: its proposal sits on the price caps, where every column
            // of a priced row has stopped paying — far beyond the prices that only have to break ties or shave the marginal tasks.  A sixteenth of it is evaluated
            // instead (a valid point like any other: the cut it yields is exact): the 65 536-column unsaturated tick 22 -> 19 sweeps, 78 fuzz seeds 36 924 -> 34 596.
            if (it == 0 && cut_lo == 0 && cuts.size() == 1) {
                std::vector<double> pa;
                static const bool agg_on = !(getenv("HQPRICE_AGG_START") && atoi(getenv("HQPRICE_AGG_START")) == 0);   // (A/B switch)
                if (agg_on && aggregate_prices(hB, lk, pa)) { pi = pa; if (rq.trace) fprintf(stderr, "[price]   first proposal: the duals of the model aggregated over chunks of blocks\n"); }
                else for (int k = 0; k < K; k++) pi[k] *= FIRST_PROPOSAL_SCALE;
            }
            const int ci = evaluate(pi);
            if (ci < 0) break;
            if (sw.time_up) { if (rq.trace) fprintf(stderr, "[price] 70 %% of the time limit gone inside the master loop\n"); return false; }
            if (budget_sweeps >= 8) { if (rq.trace) fprintf(stderr, "[price] blocks keep running out of their search budget (%d sweeps): not a model for the sweeps\n", budget_sweeps); return false; }
            const double L = fixed_value(cuts[ci], hB, cB);
            if (L < ub_best) { ub_best = L; pi_best = pi; }
            push_cuts(&mt);
        }
        if (!converged) {
            if (mt.solve(200000) != LP_OPT) return false;
            lb_master = -mt.objective() * theta_scale + cB;
            if (ub_best - lb_master > 1e-3 * std::fabs(ub_best)) { if (rq.trace) fprintf(stderr, "[price] master not converged: %.9f vs %.9f\n", ub_best, lb_master); return false; }  // nowhere near: no usable multipliers
        }
        multipliers(lambda);
        if (rq.trace) fprintf(stderr, "[price]   master: %d priced rows + %d parts, %d cut rows, %ld pivots, %.1f us inside the LP (%d active rows)\n", KL, NP, M.m, mt.iters, lp_us, mt.ma);
        pi_out.assign(K, 0.0);
        for (int i = 0; i < KL; i++) pi_out[lk[i]] = mt.x[i];
        *bound_out = ub_best;
        if (no_sweeps) { settled.valid = true; settled.hB = hB; settled.cB = cB; settled.lambda = lambda; settled.pi = pi_out; settled.bound = ub_best; settled.n_cuts = cuts.size(); settled.cut_lo = cut_lo; }
        return true;
    }

    // the patterns of the cuts that have none yet, from the device's ring (one copy for the lot)
    bool fetch_patterns() {
        size_t first = cuts.size();
        for (size_t k = 0; k < cuts.size(); k++) if (!cuts[k].fetched) { first = k; break; }
        if (first == cuts.size()) return true;
        const uint32_t count = (uint32_t)(cuts.size() - first);
        const uint16_t *pat = sw.patterns((uint32_t)first, count);
        if (!pat) { failed = true; return false; }
        const uint32_t nc = P.T.n_cols;
        for (uint32_t i = 0; i < count; i++) {
            Cut &c = cuts[first + i];
            if (c.fetched) continue;
            c.x.assign(pat + (size_t)i * nc, pat + (size_t)(i + 1) * nc);
            for (auto &l : c.lo) c.x[l.first] = (uint16_t)(c.x[l.first] + l.second);
            c.fetched = true;
        }
        return true;
    }

    // One integer pattern per block out of the active cuts' maximisers, by error diffusion over the wide rows' running totals; then the repair.
    // `hB`: right-hand sides with the flags fixed.  Returns the point over the flat columns (empty: no usable point).
    // `usable` (optional): cuts whose patterns may be used at all (branch-and-price: those that respect the node's bounds); `lo_of` (optional): lower
    // bounds of single columns the repair must not go below.
    // `variant`: 0 = the blocks in their own order (worker order: the objective's), 1 = from the last block to the first — another point of the same quality
    // class, for the ticks whose first point misses the gap by a hair.
    std::vector<uint16_t> round_patterns(const std::vector<double> &lambda, const std::vector<double> &pi, const std::vector<double> &hB,
                                         const std::vector<char> *usable = nullptr, const std::vector<int32_t> *lo_of = nullptr, int variant = 0) {
        const int K = P.K; const HostTables &T = P.T;
        const uint32_t S = (uint32_t)cuts.size();
        const double t_r0 = now_us();
        if (!fetch_patterns()) return {};
        auto pat_of = [&](int k) { return cuts[(size_t)k].x.data(); };
        // lambda: [cut * PARTS + part], every part's multipliers summing to 1 (a caller with one multiplier per cut repeats it for every part)
        const uint32_t per = (T.n_blocks + PARTS - 1) / PARTS;
        auto lam = [&](int k, uint32_t p) { return lambda[(size_t)k * PARTS + p]; };
        std::vector<int> active;
        for (uint32_t k = 0; k < S; k++) {
            if (usable && !(*usable)[k]) continue;
            bool any = false; for (uint32_t p = 0; p < (uint32_t)PARTS && !any; p++) any = lam((int)k, p) > 1e-9;
            if (any) active.push_back((int)k);
        }
        if (active.empty()) return {};
        const int Q = (int)active.size();
        // row weights: relative deviation; rows the LP leaves slack count little
        std::vector<double> lpact(K, 0.0), wgt(K);
        for (int k : active) {
            const Cut &c = cuts[k];
            if (c.pact.empty()) { for (int r = 0; r < K; r++) lpact[r] += lam(k, 0) * (double)c.act[r]; continue; }
            for (uint32_t p = 0; p < (uint32_t)PARTS; p++) { const double l = lam(k, p); if (l > 0.0) for (int r = 0; r < K; r++) lpact[r] += l * (double)c.pact[(size_t)p * P.K + r]; }
        }
        for (int r = 0; r < K; r++) {
            const bool tight = pi[r] > 1e-12 || hB[r] - lpact[r] <= 1e-6 * std::max(1.0, std::fabs(hB[r]));
            wgt[r] = (tight ? 1.0 : 0.02) / std::max(1.0, std::fabs(hB[r]));
        }
        auto block_act = [&](uint32_t b, const uint16_t *x, std::vector<double> &out) {  // A_w x of block b for the pattern row x (flat layout)
            // per group (the rows of a group share its left-hand side), then every row its group's value: the sums run over the block's columns in the same order either way
            double ga[KMAX_HOST];
            for (int g = 0; g < P.KG; g++) ga[g] = 0.0;
            for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) { const uint16_t xv = x[f]; if (!xv) continue; for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) ga[T.w_row[e]] += (double)T.w_coef[e] * (double)xv; }
            for (int r = 0; r < K; r++) out[r] = ga[P.grp_of[r]];
        };
        std::vector<uint16_t> x(T.n_cols, 0);
        std::vector<double> cum(K, 0.0);
        std::vector<int> chosen(T.n_blocks, 0);
        {   // The diffusion runs per GROUP of rows with one left-hand side: their running totals, targets and candidates are the same numbers (a row's own part is its
            // right-hand side, which enters through the weight), so the error sum_r |cum_r + cand_r - tgt_r| w_r is sum_g |cum_g + cand_g - tgt_g| W_g with W_g the
            // group's summed weights — a quarter of the terms on a three-level tick (70 rows, 16 left-hand sides).
            const int KG = P.KG;
            std::vector<double> wg(KG, 0.0), cumg(KG, 0.0), tgtg(KG, 0.0), candg((size_t)Q * KG);
            for (int r = 0; r < K; r++) wg[P.grp_of[r]] += wgt[r];
            std::vector<char> on(Q); std::vector<const double *> cgp(Q, nullptr);
            for (uint32_t bi = 0; bi < T.n_blocks; bi++) {
                const uint32_t b = variant == 1 ? T.n_blocks - 1 - bi : bi;
                const uint32_t part = b / per;
                // (three blocks in four carry the SAME pattern in every cut of their part: its activities are worked out once, the targets take the same additions in
                // the same order, and with nothing to choose between the first cut's pattern is the choice — as the comparison below would make it)
                int first = -1; bool all_same = true;
                const size_t blk_bytes = (size_t)(T.blk_off[b + 1] - T.blk_off[b]) * 2;
                for (int q = 0; q < Q; q++) {
                    const double l = lam(active[q], part);
                    on[q] = l > 1e-9;   // (only the cuts the part's LP point is made of: their patterns are optimal at the final prices)
                    if (!on[q]) continue;
                    const uint16_t *px = pat_of(active[q]);
                    if (first >= 0 && memcmp(px + T.blk_off[b], pat_of(active[first]) + T.blk_off[b], blk_bytes) == 0) cgp[q] = cgp[first];
                    else {
                        if (first < 0) first = q; else all_same = false;
                        double *cg = &candg[(size_t)q * KG];
                        for (int g = 0; g < KG; g++) cg[g] = 0.0;
                        for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) { const uint16_t xv = px[f]; if (!xv) continue; for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) cg[T.w_row[e]] += (double)T.w_coef[e] * (double)xv; }
                        cgp[q] = cg;
                    }
                    const double *cg = cgp[q];
                    for (int g = 0; g < KG; g++) tgtg[g] += l * cg[g];
                }
                int bq = -1; double be = INF;
                if (all_same) bq = first;
                else for (int q = 0; q < Q; q++) {
                    if (!on[q]) continue;
                    const double *cg = cgp[q];
                    double e = 0.0;
                    for (int g = 0; g < KG; g++) e += std::fabs(cumg[g] + cg[g] - tgtg[g]) * wg[g];
                    if (e < be - 1e-15) { be = e; bq = q; }
                }
                if (bq < 0) return {};
                const double *cb = cgp[bq];
                for (int g = 0; g < KG; g++) cumg[g] += cb[g];
                chosen[b] = active[bq];
                memcpy(&x[T.blk_off[b]], pat_of(active[bq]) + T.blk_off[b], (size_t)(T.blk_off[b + 1] - T.blk_off[b]) * 2);
            }
            for (int r = 0; r < K; r++) cum[r] = cumg[P.grp_of[r]];
        }
        if (rq.trace) fprintf(stderr, "[price]   rounding: diffusion done at %.3f us, %d active cuts\n", now_us() - t_r0, Q);
        // `>=` rows that came out short: single-block pattern switches (any sweep's pattern of that block) that close the shortfall at the least loss
        auto ge_short = [&](const std::vector<double> &c) { double s = 0.0; for (int r = 0; r < K; r++) if (P.ge[r] && c[r] > hB[r] + 1e-9) s += c[r] - hB[r]; return s; };
        if (ge_short(cum) > 0.0) {
            std::vector<int> pool = active;
            for (int k = (int)S - 1; k >= 0 && (int)pool.size() < Q + 12; k--) if ((!usable || (*usable)[k]) && std::find(pool.begin(), pool.end(), k) == pool.end()) pool.push_back(k);
            std::vector<double> a0(K), a1(K), c2(K);
            double cmax = 0.0; for (double c : T.col_cost) cmax = std::max(cmax, c);
            // Passes: every switch that would help under the current totals is scored once, the list is walked best first and a switch applied if it still
            // helps under the totals as they are by then (one block once per pass) — a pass costs what ONE move of a best-move-at-a-time loop costs.
            struct Cand { double score; uint32_t b; int k; };
            std::vector<Cand> cl; std::vector<double> colshort, coltight;
            auto evaluate_switch = [&](uint32_t b, int k, double v0, double &score) {  // a0 = the block's current activities
                const uint16_t *px = pat_of(k);
                block_act(b, px, a1);
                double gain = 0.0, newviol = 0.0;
                for (int r = 0; r < K; r++) {
                    if (a0[r] == a1[r]) continue;
                    const double c = cum[r] - a0[r] + a1[r];
                    if (P.ge[r]) gain += std::max(0.0, cum[r] - hB[r]) - std::max(0.0, c - hB[r]);
                    else newviol += std::max(0.0, c - hB[r]) - std::max(0.0, cum[r] - hB[r]);
                }
                if (!(gain > 1e-9)) return false;
                double v1 = 0.0; for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) v1 += T.col_cost[f] * (double)px[f];
                score = gain * 10.0 * cmax - (v0 - v1) - std::max(0.0, newviol) * cmax;
                return true;
            };
            auto value_of = [&](uint32_t b) { double v = 0.0; for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) v += T.col_cost[f] * (double)x[f]; return v; };
            for (int pass = 0; pass < 64 && ge_short(cum) > 0.0; pass++) {
                const double base = ge_short(cum);
                cl.clear();
                std::vector<int> short_in(P.KG, 0);   // short `>=` rows per group
                for (int r = 0; r < K; r++) if (P.ge[r] && cum[r] > hB[r] + 1e-9) short_in[P.grp_of[r]]++;
                // what one more task of column f takes off the short rows (its entries in their groups, once per pass instead of once per candidate)
                // ... and what one task LESS of it costs on the `>=` rows that hold with (almost) nothing to spare.  A row with slack s that the switch moves by D is short
                // by max(0, D - s) afterwards; summed over those rows that is at least sum(D) - sum(s), the linear form below: a bound from BELOW on what the full look
                // subtracts, as the gain here is one from above on what it adds — the filter drops no switch the full look would take.  (The three-level C3 tick:
                // 323 full looks at switches that close the short row by emptying its neighbour, before the first one that does not.)
                std::vector<int> tight_in(P.KG, 0);
                double spare = 0.0;
                for (int r = 0; r < K; r++) if (P.ge[r] && cum[r] <= hB[r] + 1e-9 && hB[r] - cum[r] <= 2.0 + 1e-9) { tight_in[P.grp_of[r]]++; spare += std::max(0.0, hB[r] - cum[r]); }
                colshort.assign(T.n_cols, 0.0); coltight.assign(T.n_cols, 0.0);
                for (uint32_t f = 0; f < T.n_cols; f++) for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) {
                    const int ns = short_in[T.w_row[e]], nt = tight_in[T.w_row[e]];
                    if (ns) colshort[f] += (double)ns * (double)T.w_coef[e];
                    if (nt) coltight[f] += (double)nt * (double)T.w_coef[e];
                }
                for (uint32_t b = 0; b < T.n_blocks; b++) {
                    for (int k : pool) {
                        if (k == chosen[b]) continue;
                        const uint16_t *px = pat_of(k);
                        // a cheap score first — what the switch takes off the short rows (its columns' entries in those rows only) against the value it gives
                        // up; the full look (every row, new violations) happens when the switch is about to be applied
                        double gain = 0.0, dv = 0.0, dmg = 0.0; bool differs = false;
                        for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) {
                            const int d = (int)px[f] - (int)x[f];
                            if (!d) continue;
                            differs = true; dv += T.col_cost[f] * (double)d;
                            gain -= colshort[f] * (double)d;  // (integers in f64: exact, whatever the grouping)
                            dmg += coltight[f] * (double)d;
                        }
                        if (!differs || !(gain - std::max(0.0, dmg - spare) > 1e-9)) continue;
                        cl.push_back({std::min(gain, base) * 10.0 * cmax + dv, b, k});
                    }
                }
                if (rq.trace) fprintf(stderr, "[price]     pass %d: short by %.1f, %zu candidate switches, at %.3f us\n", pass, base, cl.size(), now_us() - t_r0);
                if (cl.empty()) break;
                // (the best few hundred are all a pass ever applies: the rest wait for the next pass, which scores them against the totals as they are then)
                const size_t top = std::min<size_t>(cl.size(), 512);
                std::partial_sort(cl.begin(), cl.begin() + (long)top, cl.end(), [](const Cand &p, const Cand &q) { return p.score > q.score || (p.score == q.score && (p.b < q.b || (p.b == q.b && p.k < q.k))); });
                cl.resize(top);
                std::vector<char> moved(T.n_blocks, 0);
                for (const Cand &cd : cl) {
                    if (!(ge_short(cum) > 0.0)) break;
                    if (moved[cd.b]) continue;
                    {   // still worth the full look?  (the rows it was scored on may have been closed by the switches before it)
                        const uint16_t *px = pat_of(cd.k); double gain = 0.0;
                        for (uint32_t f = T.blk_off[cd.b]; f < T.blk_off[cd.b + 1]; f++) {
                            const int d = (int)px[f] - (int)x[f];
                            if (d) for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) { const int g = T.w_row[e]; for (int q = P.gr_off[g]; q < P.gr_off[g + 1]; q++) { const int r = P.gr_row[q]; if (P.ge[r] && cum[r] > hB[r] + 1e-9) gain -= (double)T.w_coef[e] * (double)d; } }
                        }
                        if (!(gain > 1e-9)) continue;
                    }
                    block_act(cd.b, pat_of(chosen[cd.b]), a0);
                    double score;
                    if (!evaluate_switch(cd.b, cd.k, value_of(cd.b), score)) continue;  // (a1 = the new pattern's activities)
                    for (int r = 0; r < K; r++) cum[r] += a1[r] - a0[r];
                    chosen[cd.b] = cd.k; moved[cd.b] = 1;
                    memcpy(&x[T.blk_off[cd.b]], pat_of(cd.k) + T.blk_off[cd.b], (size_t)(T.blk_off[cd.b + 1] - T.blk_off[cd.b]) * 2);
                }
                if (ge_short(cum) >= base - 1e-9) break;
            }
            if (ge_short(cum) > 0.0) return {};
        }
        if (rq.trace) fprintf(stderr, "[price]   rounding: >= repair done at %.3f us\n", now_us() - t_r0);
        // `<=` rows that came out over: take single tasks away, the cheapest first, never pushing a `>=` row short
        for (int r = 0; r < K; r++) {
            if (cum[r] <= hB[r] + 1e-9) continue;
            std::vector<int> cols;
            const int gr = P.grp_of[r];
            for (int k = P.g_off[gr]; k < P.g_off[gr + 1]; k++) if (P.g_coef[k] > 0 && x[P.g_col[k]] > 0) cols.push_back(k);
            std::sort(cols.begin(), cols.end(), [&](int a, int b) { const double ca = T.col_cost[P.g_col[a]] / P.g_coef[a], cb = T.col_cost[P.g_col[b]] / P.g_coef[b]; return ca < cb || (ca == cb && a > b); });
            for (int k : cols) {
                const int f = P.g_col[k];
                while (x[f] > (lo_of ? (uint16_t)(*lo_of)[f] : 0) && cum[r] > hB[r] + 1e-9) {
                    bool ok = true;
                    for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1] && ok; e++) if (T.w_coef[e] < 0) { const int g = T.w_row[e]; for (int q = P.gr_off[g]; q < P.gr_off[g + 1] && ok; q++) if (cum[P.gr_row[q]] - (double)T.w_coef[e] > hB[P.gr_row[q]] + 1e-9) ok = false; }
                    if (!ok) break;
                    x[f]--;
                    for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) { const int g = T.w_row[e]; for (int q = P.gr_off[g]; q < P.gr_off[g + 1]; q++) cum[P.gr_row[q]] -= (double)T.w_coef[e]; }
                }
                if (cum[r] <= hB[r] + 1e-9) break;
            }
            if (cum[r] > hB[r] + 1e-9) return {};
        }
        return x;
    }

    // ------------------------------------------------------------------------------------------------ branch and price
    // What the root leaves open is the integrality of the FLAGS and of the few blocks the wide rows force to mix patterns.  Nodes fix flags (first) or
    // bound one block column (x <= floor / x >= ceil of its value in the node's LP point); a node's bound is the same Lagrangian, its sweeps run with the
    // column caps hi - lo and the block capacities minus what the lower bounds use, in variables shifted by lo; cuts of other nodes are reused wherever
    // their patterns respect the node's bounds.  Depth first, the child nearer to the LP point first; a node is closed when its bound is within rel_gap
    // of the incumbent.  All limits are counts (nodes, sweeps): replicas decide alike.
    struct NodeLP { double bound = INF; bool pruned = false; std::vector<double> lambda, pi, bfrac; };

    bool apply_node(const BPNode &nd, std::vector<int32_t> &lo_arr, std::vector<int32_t> &hi_arr) {
        const HostTables &T = P.T;
        lo_arr.assign(T.n_cols, 0); hi_arr = P.base_cap;
        for (auto &l : nd.lo) lo_arr[l.first] = std::max(lo_arr[l.first], l.second);
        for (auto &h : nd.hi) hi_arr[h.first] = std::min(hi_arr[h.first], h.second);
        node_caps.clear();
        for (const CapRow &cr : P.caps) {  // a conditional bound applies once every flag of its row is fixed (before that the node is relaxed by leaving it out)
            double r = cr.rhs; bool all_fixed = true;
            for (auto &t : cr.g) { if (nd.flag[t.first] < 0) { all_fixed = false; break; } r -= t.second * (double)nd.flag[t.first]; }
            if (!all_fixed) continue;
            const double c = std::floor(r + 1e-9);
            const int32_t cap = c < 0.0 ? 0 : (c > 65535.0 ? 65535 : (int32_t)c);
            if (cap < hi_arr[cr.flat]) { hi_arr[cr.flat] = cap; node_caps.push_back({(uint32_t)cr.flat, cap}); }
        }
        std::vector<int32_t> caps(T.n_cols); std::vector<double> bcap(T.blk_cap);
        node_lo.clear(); node_cl = 0.0; node_Al.assign(P.K, 0.0);
        for (uint32_t f = 0; f < T.n_cols; f++) {
            if (hi_arr[f] < lo_arr[f]) return false;
            caps[f] = hi_arr[f] - lo_arr[f];
            const int32_t l = lo_arr[f];
            if (l <= 0) continue;
            node_lo.push_back({f, l}); node_cl += T.col_cost[f] * (double)l;
            for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) { const int g = T.w_row[e]; for (int q = P.gr_off[g]; q < P.gr_off[g + 1]; q++) node_Al[P.gr_row[q]] += (double)T.w_coef[e] * (double)l; }
            const int b = P.block_of_flat[f];
            for (int r = 0; r < MMAX_BLOCK; r++) bcap[(size_t)b * MMAX_BLOCK + r] -= T.col_a[(size_t)f * MMAX_BLOCK + r] * (double)l;
        }
        for (double v : bcap) if (v < 0.0) return false;  // the lower bounds alone overfill a worker
        if (!sw.set_caps(caps.data()) || !sw.set_block_caps(bcap.data())) { failed = true; return false; }
        at_root = nd.lo.empty() && nd.hi.empty() && node_caps.empty();
        return true;
    }

    void node_master(const BPNode &nd, double cutoff, double tol, NodeLP &out, std::vector<char> &usable) {
        const int K = P.K, G = P.G;
        out = NodeLP(); out.bound = nd.bound;
        if (!fetch_patterns()) return;
        usable.assign(cuts.size(), 1);
        for (size_t k = 0; k < cuts.size(); k++) {
            const std::vector<uint16_t> &x = cuts[k].x;
            for (auto &l : nd.lo) if ((int32_t)x[l.first] < l.second) { usable[k] = 0; break; }
            if (usable[k]) for (auto &h : nd.hi) if ((int32_t)x[h.first] > h.second) { usable[k] = 0; break; }
            if (usable[k]) for (auto &h : node_caps) if ((int32_t)x[h.first] > h.second) { usable[k] = 0; break; }
        }
        std::vector<double> hN(P.h); double cN = 0.0;
        std::vector<int> freeg;
        for (int g = 0; g < G; g++) {
            if (nd.flag[g] < 0) { freeg.push_back(g); continue; }
            cN += P.gcost[g] * (double)nd.flag[g];
            for (auto &t : P.g_rows[g]) hN[t.first] -= t.second * (double)nd.flag[g];
        }
        const int F = (int)freeg.size();
        Rows M; M.n = K + 1 + F;
        std::vector<double> mc(M.n), mlb(M.n, 0.0), mub(M.n);
        for (int k = 0; k < K; k++) { mc[k] = -hN[k] / theta_scale; mub[k] = pmax[k]; }
        mc[K] = -1.0; mub[K] = 4.0;
        for (int i = 0; i < F; i++) { mc[K + 1 + i] = -1.0; mub[K + 1 + i] = 4.0; }
        std::vector<std::pair<int, double>> terms;
        std::vector<double> row_scale; std::vector<int> row_cut;
        for (int i = 0; i < F; i++) {  // mu_g + pi.A_g >= c_g
            const int g = freeg[i];
            terms.clear(); double sc = 1.0;
            for (auto &t : P.g_rows[g]) { const double v = t.second / theta_scale; terms.push_back({t.first, v}); sc = std::max(sc, std::fabs(v)); }
            terms.push_back({K + 1 + i, 1.0});
            for (auto &t : terms) t.second /= sc;
            M.add(terms, P.gcost[g] / theta_scale / sc, INF);
            row_scale.push_back(sc); row_cut.push_back(-1);
        }
        Tab mt;
        auto add_cut = [&](size_t k, bool live) {
            const Cut &c = cuts[k];
            terms.clear(); double sc = 1.0;
            for (int r = 0; r < K; r++) if (c.act[r] != 0) { const double v = (double)c.act[r] / theta_scale; terms.push_back({r, v}); sc = std::max(sc, std::fabs(v)); }
            terms.push_back({K, 1.0});
            for (auto &t : terms) t.second /= sc;
            M.add(terms, c.cx / theta_scale / sc, INF);
            row_scale.push_back(sc); row_cut.push_back((int)k);
            if (live) mt.where.push_back(-1);
        };
        for (size_t k = 0; k < cuts.size(); k++) if (usable[k]) add_cut(k, false);
        mt.init(&M, mc, mlb, mub);
        auto node_value = [&](const Cut &c) {  // the node's Lagrangian at the cut's prices
            double L = c.bnd + cN;
            for (int k = 0; k < K; k++) L += c.pi[k] * hN[k];
            for (int g : freeg) { double r = P.gcost[g]; for (auto &t : P.g_rows[g]) r -= c.pi[t.first] * t.second; if (r > 0.0) L += r; }
            return L;
        };
        std::vector<double> pi(K), pi_best, prev;
        bool ok = false;
        for (int it = 0; it < 80; it++) {
            ok = false;
            if (mt.solve(200000) != LP_OPT) break;
            ok = true;
            const double lbm = -mt.objective() * theta_scale + cN;
            if (out.bound <= cutoff) { out.pruned = true; break; }
            if (out.bound - lbm <= tol * std::fabs(out.bound)) break;
            bool same = !prev.empty();
            for (int k = 0; k < K && same; k++) same = std::fabs(mt.x[k] - prev[k]) <= 1e-15 + 1e-12 * std::fabs(mt.x[k]);
            prev.assign(mt.x.begin(), mt.x.begin() + K);
            const double alpha = (it < 2 || same || pi_best.empty()) ? 0.0 : 0.3;
            for (int k = 0; k < K; k++) pi[k] = (alpha > 0.0 ? alpha * pi_best[k] : 0.0) + (1.0 - alpha) * mt.x[k];
            const int ci = evaluate(pi);
            if (ci < 0) { ok = false; break; }
            usable.push_back(1);
            const double L = node_value(cuts[ci]);
            if (L < out.bound) { out.bound = L; pi_best = pi; }
            add_cut((size_t)ci, true);
        }
        work += mt.ops;
        if (!ok || out.pruned) return;
        out.lambda.assign(cuts.size(), 0.0); out.bfrac.assign(G, 0.0);
        double lsum = 0.0;
        for (int r = 0; r < M.m; r++) {
            const int a = mt.where[r];
            if (a < 0 || mt.st[M.n + a] == BASIC) continue;
            const double v = std::fabs(mt.d[M.n + a]) / row_scale[r];
            if (row_cut[r] >= 0) { out.lambda[row_cut[r]] = v; lsum += v; } else out.bfrac[freeg[r]] = std::min(1.0, v);
        }
        for (int g = 0; g < G; g++) if (nd.flag[g] >= 0) out.bfrac[g] = (double)nd.flag[g];
        if (lsum > 0.0) for (double &l : out.lambda) l /= lsum; else out.lambda.clear();
        out.pi.assign(mt.x.begin(), mt.x.begin() + K);
    }
};

}  // namespace

namespace {
thread_local bool g_capture_cut = false; thread_local std::vector<unsigned char> g_first_cut;
// everything after the model has been flattened into S.P
Answer run_solver(Solver &S, const double tp0) {
    Answer ans;
    const Request &rq = S.rq; Sweeper &sw = S.sw;
    auto tmark = [&](const char *what) { if (rq.trace) fprintf(stderr, "[price] %s at %.3f ms (sweeps so far %.3f ms)\n", what, (now_us() - tp0) / 1e3, sw.stat_sweep_us / 1e3); };
    tmark("model flattened");
    if (rq.trace) fprintf(stderr, "[price]   %d equal-block runs took %d of %u blocks from their first one\n", S.P.n_runs, S.P.run_blocks, S.P.T.n_blocks);
    Prob &P = S.P;
    if (rq.trace) fprintf(stderr, "[price] %u blocks, %u block columns, %d wide rows with %d distinct left-hand sides (%zu / %zu terms), %d flags, %zu conditional bounds\n", P.T.n_blocks, P.T.n_cols, P.K, P.KG, P.row_terms, P.T.w_row.size(), P.G, P.caps.size());
    const int K = P.K, G = P.G;
    struct Ender { Sweeper *s; ~Ender() { if (s) s->end(); } } ender{S.early_begun ? &sw : nullptr};
    std::vector<double> pi0(K, 0.0);
    if (S.early == Solver::EARLY_REFUSED) { ans.why = "sweeper refused the model"; return ans; }
    if (S.early == Solver::EARLY_FAILED) { S.failed = true; ans.why = "sweep failed"; return ans; }
    if (S.early == Solver::EARLY_LAUNCHED) {
        // the first sweep has been on its way since the block tables were final (Solver::launch_on_blocks); the wide rows' tables follow it on the stream
        if (!sw.begin_wide()) { ans.why = "sweeper refused the model"; return ans; }
        tmark("wide tables handed to the sweeper");
    } else {
        S.prepare_sweeper();
        if (!sw.begin(P.T, (uint32_t)S.max_sweeps)) { ans.why = "sweeper refused the model"; return ans; }
        ender.s = &sw;
        tmark("tables handed to the sweeper");
        // the first sweep runs at zero prices: it needs the tables and nothing else, so it is on its way while the host works out the price caps
        if (!S.evaluate_launch(pi0)) { ans.why = "sweep failed"; return ans; }
    }
    // price caps: beyond pmax every column of the row has a negative reduced cost (`<=` rows); for `>=` rows a multiple of the largest cost per unit
    S.pmax.assign(K, 0.0);
    {
        double cmax = 0.0; for (double c : P.T.col_cost) cmax = std::max(cmax, c);
        // (per GROUP: the rows of a group share their left-hand side — one division per term of a list, not one per term of every row that carries it)
        std::vector<double> gp(P.KG, 0.0);
        for (int g = 0; g < P.KG; g++) {
            double p = 0.0; bool neg = false; int32_t amin = INT32_MAX;
            for (int t = P.g_off[g]; t < P.g_off[g + 1]; t++) {
                const int32_t a = P.g_coef[t];
                if (a > 0) p = std::max(p, P.T.col_cost[P.g_col[t]] / (double)a); else { neg = true; amin = std::min(amin, -a); }
            }
            if (neg) p = std::max(p, 64.0 * cmax / (double)std::max<int32_t>(1, amin));
            gp[g] = p;
        }
        for (int k = 0; k < K; k++) S.pmax[k] = gp[P.grp_of[k]];
    }
    tmark("price caps done");
    if (S.evaluate(pi0, true) < 0) { ans.why = "sweep failed"; return ans; }
    tmark("first sweep (prices 0) done");
    if (g_capture_cut) {
        const Cut &c0 = S.cuts[0];
        auto put = [](const void *p, size_t bytes) { const unsigned char *b = (const unsigned char *)p; g_first_cut.insert(g_first_cut.end(), b, b + bytes); };
        g_first_cut.clear();
        put(c0.act.data(), c0.act.size() * sizeof(long long)); put(c0.pact.data(), c0.pact.size() * sizeof(long long));
        put(&c0.cx, sizeof c0.cx); put(&c0.bnd, sizeof c0.bnd); put(c0.pcx.data(), c0.pcx.size() * sizeof(double));
    }
    S.theta_scale = std::max(S.cuts[0].bnd, 1e-9);
    ans.ran = true;
    double best_value = rq.incumbent ? rq.incumbent_value : -INF;
    std::vector<double> hB(K);
    std::vector<int32_t> caps(P.base_cap);
    std::vector<double> final_pi;
    std::vector<std::vector<double>> tried;   // flag configurations already solved
    auto was_tried = [&](const std::vector<double> &B) { for (auto &t : tried) if (t == B) return true; return false; };
    auto certified = [&]() { return best_value > -INF && S.relaxed_bound <= best_value + rq.rel_gap * std::fabs(best_value); };
    // One flag configuration: master to convergence, one pattern per block, repair, the caller's polish.  Returns the point's value (-INF: nothing
    // usable came out) and leaves the point in x.
    std::vector<double> jump_to;   // set by try_config's probe: the configuration to go to instead (try_config returns -INF then)
    auto try_config = [&](const std::vector<double> &B, std::vector<double> &x) -> double {
        tried.push_back(B);
        // (the one clock of this path: read at the sweeps, and — where no other rank depends on the reading — here, so that the host-only stretches between sweeps
        // (master LPs, rounding, polish) cannot carry a tick past its guard either; a sharded sweeper merges the ranks' readings inside its exchange, nowhere else)
        if (!sw.merges_clock() && now_us() * 1e-6 > sw.guard_s) sw.time_up = true;
        if (sw.time_up) return -INF;
        ans.rounds++;
        double cB = 0.0;
        for (int k = 0; k < K; k++) hB[k] = P.h[k];
        for (int g = 0; g < G; g++) { cB += P.gcost[g] * B[g]; for (auto &t : P.g_rows[g]) hB[t.first] -= t.second * B[g]; }
        if (!P.caps.empty()) {  // conditional bounds with the flags fixed
            caps = P.base_cap;
            for (const CapRow &cr : P.caps) { double r = cr.rhs; for (auto &t : cr.g) r -= t.second * B[t.first]; const double c = std::floor(r + 1e-9); if (c < (double)caps[cr.flat]) caps[cr.flat] = c < 0.0 ? 0 : (int32_t)c; }
            if (!sw.set_caps(caps.data())) { S.failed = true; return -INF; }
            // (the cuts of earlier rounds are points of THEIR bounds: a round with other bounds starts a new master)
            S.base_caps = false; S.cut_lo = S.cuts.size();
            if (S.evaluate(pi0) < 0) return -INF;
        }
        std::vector<double> lambda, pi;
        double bound_B = INF;
        const double cutoff = best_value > -INF ? best_value * (1.0 - 1e-12) : -INF;
        const double tol = std::max(1e-6, rq.rel_gap / 50.0);
        // Once this configuration's master is within 10 %: would the flags its fractional point does not need, dropped, give a configuration whose master is ALREADY
        // converged on the cuts at hand, at a bound no worse?  Then that is where the walk goes — this configuration would be left for it anyway after its own
        // convergence, rounding and polish (the three-level C3 tick: 9 sweeps on the incumbent's flags, then a successor that converged without one more; now 3).
        jump_to.clear();
        S.probe = nullptr;
        if (G > 0 && P.caps.empty()) S.probe = [&](const std::vector<double> &colact, double lb_here) -> bool {
            std::vector<double> Bp = B, act = colact;
            for (int g = 0; g < G; g++) if (Bp[g] == 1.0) for (auto &t : P.g_rows[g]) act[t.first] += t.second;
            bool dropped = false;
            for (int g = 0; g < G; g++) {
                if (Bp[g] != 1.0 || P.gcost[g] != 0.0) continue;
                bool ok = true;
                for (auto &t : P.g_rows[g]) if (act[t.first] - t.second > P.h[t.first] + 1e-7 * (1.0 + std::fabs(P.h[t.first]))) ok = false;
                if (!ok) continue;
                Bp[g] = 0.0; dropped = true;
                for (auto &t : P.g_rows[g]) act[t.first] -= t.second;
            }
            if (!dropped || was_tried(Bp)) return false;
            std::vector<double> hBp(K); double cBp = 0.0;
            for (int k = 0; k < K; k++) hBp[k] = P.h[k];
            for (int g = 0; g < G; g++) { cBp += P.gcost[g] * Bp[g]; for (auto &t : P.g_rows[g]) hBp[t.first] -= t.second * Bp[g]; }
            std::vector<double> lam2, pi2; double b2 = INF;
            if (!S.kelley(hBp, cBp, -INF, tol, lam2, pi2, &b2, true) || b2 < lb_here) { S.settled.valid = false; return false; }
            if (rq.trace) fprintf(stderr, "[price] configuration %u left for the one its fractional point names: converged on the %zu cuts at hand, bound %.9f\n", ans.rounds, S.cuts.size(), b2);
            jump_to = Bp;
            return true;
        };
        const bool conv = S.kelley(hB, cB, cutoff, tol, lambda, pi, &bound_B);
        S.probe = nullptr;
        if (!conv) return -INF;
        tmark("master converged");
        final_pi = pi;
        std::vector<uint16_t> xf = S.round_patterns(lambda, pi, hB);
        tmark("patterns rounded");
        if (xf.empty()) return -INF;
        x.assign(rq.n, 0.0);
        for (uint32_t f = 0; f < P.T.n_cols; f++) x[P.model_of[f]] = (double)xf[f];
        for (int g = 0; g < G; g++) x[P.gmodel[g]] = B[g];
        double value = 0.0;
        if (!rq.polish || !rq.polish(x, value)) return -INF;  // the caller's rows say no
        tmark("polished");
        if (rq.trace) fprintf(stderr, "[price] configuration %u: %zu sweeps so far, bound with these flags %.9f, point %.9f, model bound %.9f\n", ans.rounds, S.cuts.size(), bound_B, value, S.relaxed_bound);
        if (value > best_value) { best_value = value; ans.x = x; ans.x_value = value; }
        // not certified by this point although the configuration's bound allows more: the same multipliers rounded in the other block order — a third of a
        // millisecond against the dozens of sweeps branch-and-price would spend on the same question (the layered DAG loop's 57-sweep ticks: 17)
        if (bound_B > best_value * (1.0 + rq.rel_gap)) {
            std::vector<uint16_t> xr = S.round_patterns(lambda, pi, hB, nullptr, nullptr, 1);
            if (!xr.empty()) {
                std::vector<double> x2(rq.n, 0.0);
                for (uint32_t f = 0; f < P.T.n_cols; f++) x2[P.model_of[f]] = (double)xr[f];
                for (int g = 0; g < G; g++) x2[P.gmodel[g]] = B[g];
                double v2 = 0.0;
                if (rq.polish(x2, v2)) {
                    if (rq.trace) fprintf(stderr, "[price] configuration %u, blocks in reverse order: point %.9f\n", ans.rounds, v2);
                    if (v2 > value) { value = v2; x = x2; }
                    if (v2 > best_value) { best_value = v2; ans.x = x2; ans.x_value = v2; }
                }
            }
        }
        return value;
    };
    // flags of x whose rows hold without them are dropped (they only ever restrict): the rule of milp.cpp's sparse_greedy.  True if B changed.
    auto drop_flags = [&](std::vector<double> &B, const std::vector<double> &x) {
        bool dropped = false;
        std::vector<double> act(K, 0.0);
        {
            std::vector<double> ga(P.KG, 0.0);
            for (int g = 0; g < P.KG; g++) for (int t = P.g_off[g]; t < P.g_off[g + 1]; t++) ga[g] += (double)P.g_coef[t] * x[P.model_of[P.g_col[t]]];
            for (int k = 0; k < K; k++) act[k] += ga[P.grp_of[k]];
        }
        for (int g = 0; g < G; g++) for (auto &t : P.g_rows[g]) act[t.first] += t.second * x[P.gmodel[g]];
        for (int g = 0; g < G; g++) {
            if (B[g] != 1.0 || P.gcost[g] != 0.0 || x[P.gmodel[g]] != 1.0) continue;
            bool ok = true;
            for (auto &t : P.g_rows[g]) if (act[t.first] - t.second > P.h[t.first] + 1e-7 * (1.0 + std::fabs(P.h[t.first]))) ok = false;
            if (!ok) continue;
            B[g] = 0.0; dropped = true;
            for (auto &t : P.g_rows[g]) act[t.first] -= t.second;
        }
        return dropped;
    };
    // a configuration and what dropping leads to from there
    auto descend = [&](std::vector<double> B) {
        for (int round = 0; round < MAX_ROUNDS && !S.failed && !was_tried(B); round++) {
            std::vector<double> x;
            const double v = try_config(B, x);
            if (!jump_to.empty()) { B = jump_to; jump_to.clear(); continue; }
            if (v == -INF) break;
            if (certified()) break;
            if (!drop_flags(B, x)) break;
        }
    };
    if (rq.incumbent && G > 0) {  // the caller's incumbent (milp.cpp's sparse_greedy: flags on, raise, drop the flags no longer needed, raise again) names a configuration
        std::vector<double> B(G);
        for (int g = 0; g < G; g++) B[g] = rq.incumbent[P.gmodel[g]] > 0.5 ? 1.0 : 0.0;
        descend(B);
    }
    if (ans.x.empty() && !S.failed) descend(std::vector<double>(G, 1.0));   // every flag on: always feasible for the tick's models (every lower-priority batch capped at its cut)
    if (S.failed) { ans.ran = false; ans.why = "sweep failed"; ans.x.clear(); return ans; }
    // Not certified against the bound seen so far and the model has flags: the master of the RELAXED model (flags in [0, 1]) may still bring the bound
    // down — its cuts are the points already evaluated, the flags enter through one extra variable each (mu_g >= c_g - pi.A_g, mu_g >= 0).  Its
    // multipliers of the flag rows are the flags' LP values: the configuration they round to, and single flags forced off in the order of those
    // values, are tried next ("place every higher-priority task of that class": often worth a little utilisation for what it unlocks).
    std::vector<double> Blp;
    if (G > 0 && best_value > -INF && !certified()) {
        if (!S.base_caps) {  // back to the model's own column bounds: only sweeps under those bound the relaxed model
            if (!sw.set_caps(P.base_cap.data())) { ans.ran = false; ans.why = "sweep failed"; ans.x.clear(); return ans; }
            S.base_caps = true; S.cut_lo = S.cuts.size();
            if (S.evaluate(pi0) < 0) { ans.ran = false; ans.why = "sweep failed"; ans.x.clear(); return ans; }
        }
        Rows M; M.n = K + 1 + G;
        std::vector<double> mc(M.n), mlb(M.n, 0.0), mub(M.n);
        for (int k = 0; k < K; k++) { mc[k] = -P.h[k] / S.theta_scale; mub[k] = S.pmax[k]; }
        mc[K] = -1.0; mub[K] = 4.0;
        for (int g = 0; g < G; g++) { mc[K + 1 + g] = -1.0; mub[K + 1 + g] = 4.0; }
        std::vector<std::pair<int, double>> terms;
        for (int g = 0; g < G; g++) {  // mu_g + pi.A_g >= c_g
            terms.clear(); double sc = 1.0;
            for (auto &t : P.g_rows[g]) { const double v = t.second / S.theta_scale; terms.push_back({t.first, v}); sc = std::max(sc, std::fabs(v)); }
            terms.push_back({K + 1 + g, 1.0});
            for (auto &t : terms) t.second /= sc;
            M.add(terms, P.gcost[g] / S.theta_scale / sc, INF);
        }
        size_t in_master = S.cut_lo;
        Tab mt;
        auto push_cuts = [&](bool live) {
            for (; in_master < S.cuts.size(); in_master++) {
                const Cut &c = S.cuts[in_master];
                terms.clear(); double sc = 1.0;
                for (int k = 0; k < K; k++) if (c.act[k] != 0) { const double v = (double)c.act[k] / S.theta_scale; terms.push_back({k, v}); sc = std::max(sc, std::fabs(v)); }
                terms.push_back({K, 1.0});
                for (auto &t : terms) t.second /= sc;
                M.add(terms, c.cx / S.theta_scale / sc, INF);
                if (live) mt.where.push_back(-1);
            }
        };
        push_cuts(false);
        mt.init(&M, mc, mlb, mub);
        std::vector<double> pi(K), pi_best = S.relaxed_pi.empty() ? std::vector<double>(K, 0.0) : S.relaxed_pi, prev;
        bool master_ok = false;
        for (int it = 0; it < 120; it++) {
            master_ok = false;
            if (mt.solve(200000) != LP_OPT) break;
            master_ok = true;
            const double lb_master = -mt.objective() * S.theta_scale;
            if (S.relaxed_bound <= best_value + rq.rel_gap * std::fabs(best_value)) break;   // certified
            if (S.relaxed_bound - lb_master <= 1e-6 * std::fabs(S.relaxed_bound)) break;      // the bound is what it is
            bool same = !prev.empty();
            for (int k = 0; k < K && same; k++) same = std::fabs(mt.x[k] - prev[k]) <= 1e-15 + 1e-12 * std::fabs(mt.x[k]);
            prev.assign(mt.x.begin(), mt.x.begin() + K);
            const double alpha = (it < 2 || same) ? 0.0 : 0.3;
            for (int k = 0; k < K; k++) pi[k] = alpha * pi_best[k] + (1.0 - alpha) * mt.x[k];
            const double before = S.relaxed_bound;
            if (S.evaluate(pi) < 0) break;
            if (S.relaxed_bound < before) pi_best = pi;
            push_cuts(true);
        }
        if (S.failed) { ans.ran = false; ans.why = "sweep failed"; ans.x.clear(); return ans; }
        if (master_ok || mt.solve(200000) == LP_OPT) {
            Blp.assign(G, 0.0);
            for (int g = 0; g < G; g++) { const int ar = mt.where[g]; if (ar >= 0 && mt.st[M.n + ar] != BASIC) { double sc = 1.0; for (auto &t : P.g_rows[g]) sc = std::max(sc, std::fabs(t.second / S.theta_scale)); Blp[g] = std::min(1.0, std::fabs(mt.d[M.n + ar]) / sc); } }
        }
    }
    if (!Blp.empty() && !certified() && P.caps.empty()) {
        std::vector<double> B(G);
        for (int g = 0; g < G; g++) B[g] = (Blp[g] > 0.5 || P.gcost[g] > 0.0) ? 1.0 : 0.0;
        descend(B);
        // single flags of the best configuration forced off, least LP value first
        for (int trial = 0; trial < 12 && !certified() && !S.failed && !ans.x.empty(); trial++) {
            std::vector<double> cur(G);
            for (int g = 0; g < G; g++) cur[g] = ans.x[P.gmodel[g]];
            int pick = -1; double pv = INF;
            for (int g = 0; g < G; g++) {
                if (cur[g] != 1.0 || P.gcost[g] != 0.0) continue;
                std::vector<double> t = cur; t[g] = 0.0;
                if (was_tried(t)) continue;
                if (Blp[g] < pv) { pv = Blp[g]; pick = g; }
            }
            if (pick < 0) break;
            cur[pick] = 0.0;
            descend(cur);
        }
        if (S.failed) { ans.ran = false; ans.why = "sweep failed"; ans.x.clear(); return ans; }
    }
    // ---- branch and price: what the configurations above leave open, on models small enough for a few hundred more sweeps to be cheap ----
    double bp_bound = INF;
    if (best_value > -INF && !certified() && !S.failed && P.T.n_cols <= 131072 && S.budget_sweeps < 8) {
        S.base_caps = true;  // every node sets its own column bounds from here on
        int col_nodes = 0;  // branching on single columns moves the bound of these models very little (a mixing worker passes its role to the next one): a short leash
        auto closes = [&](double bound) { return bound <= best_value + rq.rel_gap * std::fabs(best_value); };
        std::vector<BPNode> stack;
        { BPNode root; root.flag.assign(G, -1); root.bound = S.relaxed_bound; stack.push_back(std::move(root)); }
        double closed_max = -INF;  // the largest bound among the closed nodes: with the open ones it bounds the model
        int nodes = 0;
        std::vector<int32_t> lo_arr, hi_arr; std::vector<char> usable;
        while (!stack.empty() && nodes < BP_MAX_NODES && (int)S.cuts.size() + 8 < S.max_sweeps && S.work < BP_MAX_WORK * rq.time_limit_s && S.sweep_steps < BP_MAX_STEPS * rq.time_limit_s &&
               !sw.time_up && !S.failed) {
            BPNode nd = std::move(stack.back()); stack.pop_back();
            if (!sw.merges_clock() && now_us() * 1e-6 > sw.guard_s) { sw.time_up = true; stack.push_back(std::move(nd)); break; }
            if (closes(nd.bound)) { closed_max = std::max(closed_max, nd.bound); continue; }
            nodes++;
            if (!S.apply_node(nd, lo_arr, hi_arr)) { if (S.failed) break; continue; }  // empty node
            Solver::NodeLP lp;
            S.node_master(nd, best_value, std::max(2e-6, rq.rel_gap / 20.0), lp, usable);
            if (S.failed) break;
            if (lp.pruned || closes(lp.bound)) { closed_max = std::max(closed_max, std::min(lp.bound, nd.bound)); continue; }
            if (lp.lambda.empty()) { stack.push_back(std::move(nd)); break; }  // no usable multipliers (master trouble): leave the node open
            nd.bound = std::min(nd.bound, lp.bound);
            // flags first: the free flag whose LP value is least decided
            int bg = -1; double bd = 1e-6;
            for (int g = 0; g < G; g++) if (nd.flag[g] < 0) { const double d = std::min(lp.bfrac[g], 1.0 - lp.bfrac[g]); if (d > bd) { bd = d; bg = g; } }
            if (bg < 0) {  // every flag is 0 or 1 in the LP point: the node's patterns make a point
                std::vector<double> Bn(G), hBn(P.h);
                for (int g = 0; g < G; g++) { Bn[g] = lp.bfrac[g] > 0.5 ? 1.0 : 0.0; for (auto &t : P.g_rows[g]) hBn[t.first] -= t.second * Bn[g]; }
                std::vector<double> lam_parts(lp.lambda.size() * PARTS);
                for (size_t k = 0; k < lp.lambda.size(); k++) for (int p = 0; p < PARTS; p++) lam_parts[k * PARTS + p] = lp.lambda[k];
                std::vector<uint16_t> xf = S.round_patterns(lam_parts, lp.pi, hBn, &usable, &lo_arr);
                if (!xf.empty()) {
                    std::vector<double> x(rq.n, 0.0);
                    for (uint32_t f = 0; f < P.T.n_cols; f++) x[P.model_of[f]] = (double)xf[f];
                    for (int g = 0; g < G; g++) x[P.gmodel[g]] = Bn[g];
                    double value = 0.0;
                    if (rq.polish && rq.polish(x, value) && value > best_value) { best_value = value; ans.x = x; ans.x_value = value; }
                }
                if (closes(nd.bound)) { closed_max = std::max(closed_max, nd.bound); continue; }
            }
            BPNode a = nd, b = nd; a.depth = b.depth = nd.depth + 1;
            if (bg >= 0) {
                const int8_t first = lp.bfrac[bg] > 0.5 ? 1 : 0;
                a.flag[bg] = first; b.flag[bg] = (int8_t)(1 - first);
            } else {  // the block column whose LP value is furthest from an integer (cost-weighted)
                if (++col_nodes > 48) { stack.push_back(std::move(nd)); break; }
                int bf = -1; double bs = 1e-7, bv = 0.0;
                std::vector<double> xl(P.T.n_cols, 0.0);
                for (size_t k = 0; k < S.cuts.size(); k++) { const double l = k < lp.lambda.size() ? lp.lambda[k] : 0.0; if (l <= 0.0 || !usable[k]) continue; const uint16_t *px = S.cuts[k].x.data(); for (uint32_t f = 0; f < P.T.n_cols; f++) xl[f] += l * (double)px[f]; }
                for (uint32_t f = 0; f < P.T.n_cols; f++) { const double fr = xl[f] - std::floor(xl[f]); const double sc = std::min(fr, 1.0 - fr) * (P.T.col_cost[f] + 1e-9); if (std::min(fr, 1.0 - fr) > 1e-6 && sc > bs) { bs = sc; bf = (int)f; bv = xl[f]; } }
                if (bf < 0) { closed_max = std::max(closed_max, nd.bound); continue; }  // an integral LP point that still did not close: nothing to branch on (its value IS the bound)
                const int32_t fl = (int32_t)std::floor(bv);
                BPNode dn = nd, up = nd; dn.depth = up.depth = nd.depth + 1;
                dn.hi.push_back({(uint32_t)bf, fl}); up.lo.push_back({(uint32_t)bf, fl + 1});
                if (bv - fl < 0.5) { a = std::move(dn); b = std::move(up); } else { a = std::move(up); b = std::move(dn); }
            }
            stack.push_back(std::move(b)); stack.push_back(std::move(a));  // (a = the child nearer to the LP point: popped first)
        }
        bp_bound = closed_max;
        for (const BPNode &nd : stack) bp_bound = std::max(bp_bound, nd.bound);
        if (rq.trace) fprintf(stderr, "[price] branch and price: %d nodes, %zu left open, %zu sweeps in all, bound %.9f, incumbent %.9f\n", nodes, stack.size(), S.cuts.size(), bp_bound, best_value);
        // back to the model's own bounds (a later caller of this sweeper starts from begin() anyway)
        S.node_lo.clear(); S.at_root = true;
        if (S.failed) { ans.ran = false; ans.why = "sweep failed"; ans.x.clear(); return ans; }
    }
    ans.bound = std::min(S.relaxed_bound, bp_bound > -INF ? bp_bound : INF);
    ans.sweeps = (uint32_t)sw.stat_sweeps;
    // for the host's guided windows: blocks, their values and the reduced costs at the last prices
    // (only what the sweeps leave open goes on to the host's windows: a certified answer needs neither)
    const bool closed = best_value > -INF && ans.bound <= best_value + rq.rel_gap * std::fabs(best_value);
    if (!final_pi.empty() && !closed) {
        ans.block_of.assign(rq.n, -1); ans.rcost.assign(rq.n, 0.0);
        std::vector<std::pair<int, double>> rows;
        for (uint32_t f = 0; f < P.T.n_cols; f++) {
            const int j = P.model_of[f];
            ans.block_of[j] = P.block_of_flat[f];
            double r = P.T.col_cost[f];
            rows.clear();   // the column's rows in ascending order (the order the prices are subtracted in is part of the value's last bits)
            for (uint32_t e = P.T.col_woff[f]; e < P.T.col_woff[f + 1]; e++) { const int g = P.T.w_row[e]; for (int q = P.gr_off[g]; q < P.gr_off[g + 1]; q++) rows.push_back({P.gr_row[q], (double)P.T.w_coef[e]}); }
            std::sort(rows.begin(), rows.end());
            for (auto &t : rows) r -= final_pi[t.first] * t.second;
            ans.rcost[j] = r;
        }
    }
    return ans;
}

thread_local int g_early_sweep = -1;
bool early_sweep_on() {
    static const bool env_on = !(getenv("HQPRICE_EARLY_SWEEP") && atoi(getenv("HQPRICE_EARLY_SWEEP")) == 0);   // (A/B switch)
    return g_early_sweep < 0 ? env_on : g_early_sweep != 0;
}
}  // namespace

Answer solve_model(const ModelView &mv, double rel_gap, double time_limit_s, double deadline_s, bool trace, Sweeper &sw, double *cost_scale) {
    const double tp0 = now_us();
    Request rq;
    rq.n = mv.n; rq.m = mv.m; rq.rel_gap = rel_gap; rq.time_limit_s = time_limit_s; rq.deadline_s = deadline_s; rq.trace = trace;
    Solver S(rq, sw);
    S.tp0 = tp0;
    if (g_capture_cut) g_first_cut.clear();
    std::vector<double> ub, c; double cmax = 1.0;
    const std::function<void()> hook = [&S]() { S.launch_on_blocks(); };
    if (const char *why = flatten(mv, S.P, ub, c, cmax, early_sweep_on() ? &hook : nullptr)) {
        if (S.early_begun) sw.end();   // (refused behind the hook: a sweep may be in flight on tables that S.P owns — end() waits for it)
        Answer ans; ans.why = why; return ans;
    }
    if (cost_scale) *cost_scale = cmax;
    Polisher pol(S.P, mv.n);
    rq.polish = [&pol](std::vector<double> &x, double &value) { return pol.run(x, value); };
    return run_solver(S, tp0);
}

void set_early_sweep(int on) { g_early_sweep = on; g_early_sweeps = 0; }
uint32_t early_sweeps() { return g_early_sweeps; }
void capture_first_cut(bool on) { g_capture_cut = on; g_first_cut.clear(); }
const std::vector<unsigned char> &first_cut_bytes() { return g_first_cut; }

Answer solve(const Request &rq, Sweeper &sw) {
    Solver S(rq, sw);
    const double tp0 = now_us();
    if (const char *why = flatten(rq, S.P)) { Answer ans; ans.why = why; return ans; }
    return run_solver(S, tp0);
}

}  // namespace hqprice
