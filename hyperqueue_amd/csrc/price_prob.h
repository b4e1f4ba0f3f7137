// The coupled solve's flattened problem: what the flatteners (price_flatten.cpp) leave and the solver (price.cpp) reads.  Internal, host-only.
#pragma once
#include "price.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace hqprice {

constexpr int KMAX_HOST = 128;   // == price_core.h's KMAX (not included here: these sources are host-only and also part of libhqalloc.so)
constexpr int NMAX_BLOCK = 32, MMAX_BLOCK = 4;
constexpr double GRID = 10000.0;  // ResourceAmount fractions per unit  common/resources/amount.rs:7
constexpr double UNBOUNDED = 1e300;   // == lp_tab.h's INF (price.cpp, which sees both, asserts it)

struct CapRow { int flat; double rhs; std::vector<std::pair<int, double>> g; };  // x_flat + sum_g coef B_g <= rhs (the column's own coefficient divided out)

struct Prob {
    HostTables T;
    std::vector<int> flat_of, model_of;       // model column <-> flat column (-1: global)
    std::vector<int> gmodel;                   // global columns (model index)
    std::vector<double> gcost;
    int K = 0, G = 0;
    std::vector<double> h;                     // wide rows in <= form
    std::vector<uint8_t> ge;                   // the row was a `>=` row (entered negated)
    std::vector<std::vector<std::pair<int, double>>> g_rows;   // per global column: (wide row, coefficient in <= form)
    // Wide rows with the same left-hand side over the block columns (the cut rows of one batch against its several blockers differ in their flag only) share
    // ONE activity: the device prices and accumulates per GROUP (T.K groups, price of a group = sum of its rows' prices), and the host keeps the left-hand
    // sides per group as well — row-wise here, column-wise in T.col_woff / T.w_row / T.w_coef — and expands to rows where a row's own right-hand side matters
    // (c3p at BASELINE size: 70 wide rows, 16 distinct left-hand sides, 71 680 against 16 384 terms).
    std::vector<int> grp_of;   // [K] row -> group
    int KG = 0;
    std::vector<int> g_off, g_col; std::vector<int32_t> g_coef;   // [KG] the distinct left-hand sides over the flat columns, terms in the model's order
    std::vector<int> gr_off, gr_row;                              // [KG] the rows of a group, ascending
    size_t row_terms = 0;                                         // terms of the K rows as the model wrote them (statistics)
    std::vector<CapRow> caps;
    std::vector<int32_t> base_cap;
    std::vector<int> block_of_flat;
    int n_runs = 0, run_blocks = 0;   // equal-block runs of the model that passed the flattener's comparison, and the blocks they cover (statistics)
};

// round half away from zero without the call into libm (-msse4.1 gives floor / nearbyint as one instruction, not round); |v| < 2^51
inline double round_fast(double v) { return (double)(long long)(v + (v >= 0.0 ? 0.5 : -0.5)); }
inline long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a < 0 ? -a : a; }

// ---- price_flatten.cpp.  Both return nullptr on success, else what keeps the model away from the sweeps.
// The component as CompSolver holds it (scaled rows, given bounds and costs) -> blocks + wide rows.
const char *flatten(const Request &rq, Prob &P);
// The model as its builder wrote it -> the same tables, the same numbering.  ub: the derived column bounds (model columns), c: obj / cmax.  after_blocks (optional) is
// called once, when the block tables — T.n_blocks, T.n_cols, blk_off, blk_m, blk_cap, col_cost, col_a, col_cap — are final: behind the rows loop, the last run's copies
// and the never-binding rows.  What follows builds the wide rows' groups and changes none of the eight.  Also serves mv.run_stats / mv.tables_digest and, under
// set_check_hints, flattens a model with block runs a second time without them and demands the same bytes.
const char *flatten(const ModelView &mv, Prob &P, std::vector<double> &ub, std::vector<double> &c, double &cmax, const std::function<void()> *after_blocks = nullptr);
// FNV-1a over everything the flattening leaves (tests: two ways of getting there must agree in every byte)
uint64_t digest_of(const Prob &P);

// The candidate point of a flag configuration against the flattened model, raised greedily (most valuable columns first) as far as the blocks' rows, the wide rows
// and the conditional bounds allow — what CompSolver::polish_point does on the component's scaled rows.  The integers are exact here: block rows on their own grid,
// wide rows with integer coefficients.  x: the model's columns (in / out).
struct Polisher {
    const Prob &P; int n;
    explicit Polisher(const Prob &p, int n_) : P(p), n(n_) {}
    bool run(std::vector<double> &x, double &value) const {
        const HostTables &T = P.T; const int K = P.K, G = P.G;
        if ((int)x.size() != n) return false;
        std::vector<double> xf(T.n_cols), B(G);
        for (uint32_t f = 0; f < T.n_cols; f++) { const double v = x[P.model_of[f]], rv = round_fast(v); if (v < -1e-9 || v > (double)P.base_cap[f] + 1e-9 || std::fabs(v - rv) > 1e-9) return false; xf[f] = rv; }
        for (int g = 0; g < G; g++) { B[g] = x[P.gmodel[g]]; if (B[g] != 0.0 && B[g] != 1.0) return false; }
        // block rows
        std::vector<double> bact((size_t)T.n_blocks * MMAX_BLOCK, 0.0);
        for (uint32_t b = 0; b < T.n_blocks; b++) {
            double *ba = &bact[(size_t)b * MMAX_BLOCK];
            for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) if (xf[f] != 0.0) for (int r = 0; r < MMAX_BLOCK; r++) ba[r] += T.col_a[(size_t)f * MMAX_BLOCK + r] * xf[f];
            for (int r = 0; r < (int)T.blk_m[b]; r++) if (ba[r] > T.blk_cap[(size_t)b * MMAX_BLOCK + r]) return false;
        }
        // wide rows: activity per group, the flags' part per row
        std::vector<double> ga(P.KG, 0.0), fl(K, 0.0);
        for (int g = 0; g < P.KG; g++) for (int t = P.g_off[g]; t < P.g_off[g + 1]; t++) ga[g] += (double)P.g_coef[t] * xf[P.g_col[t]];
        for (int g = 0; g < G; g++) if (B[g] != 0.0) for (auto &t : P.g_rows[g]) fl[t.first] += t.second * B[g];
        for (int k = 0; k < K; k++) if (ga[P.grp_of[k]] + fl[k] > P.h[k] + 1e-9 * std::max(1.0, std::fabs(P.h[k]))) return false;
        // conditional bounds with these flags
        std::vector<double> cap(T.n_cols);
        for (uint32_t f = 0; f < T.n_cols; f++) cap[f] = (double)P.base_cap[f];
        for (const CapRow &cr : P.caps) { double r = cr.rhs; for (auto &t : cr.g) r -= t.second * B[t.first]; const double cc = std::floor(r + 1e-9); if (xf[cr.flat] > cc) return false; cap[cr.flat] = std::min(cap[cr.flat], cc); }
        // The raise goes through the columns by descending cost (ties: ascending model column — CompSolver::polish_point's order).  Raising only ever uses room up, so
        // a column whose own block has no room for one more of it NOW never gets any: the few that do are found first, and only those are ordered.
        std::vector<int> order;
        // (the same holds for the wide rows: a group whose tightest row has no room for the column's coefficient rules the column out for good — on an unsaturated
        // tick the batch-size rows are tight after the rounding and nearly every worker has room: without this test 60 000 columns were candidates, for nothing)
        std::vector<double> gslack(P.KG, UNBOUNDED);
        for (int k = 0; k < K; k++) { const int g = P.grp_of[k]; gslack[g] = std::min(gslack[g], P.h[k] - (ga[g] + fl[k])); }
        for (uint32_t b = 0; b < T.n_blocks; b++) {
            const double *ba = &bact[(size_t)b * MMAX_BLOCK], *bc = &T.blk_cap[(size_t)b * MMAX_BLOCK];
            const int mb = (int)T.blk_m[b];
            for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) {
                if (!(T.col_cost[f] > 0.0) || cap[f] - xf[f] < 1.0) continue;
                bool room = true;
                for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1] && room; e++) { const double a = (double)T.w_coef[e]; if (a > 0.0 && gslack[T.w_row[e]] < 0.5 * a) room = false; }
                for (int r = 0; r < mb && room; r++) { const double a = T.col_a[(size_t)f * MMAX_BLOCK + r]; if (a > 0.0 && bc[r] - ba[r] < a) room = false; }
                if (room) order.push_back((int)f);
            }
        }
        std::sort(order.begin(), order.end(), [&](int p, int q) { return T.col_cost[p] > T.col_cost[q] || (T.col_cost[p] == T.col_cost[q] && P.model_of[p] < P.model_of[q]); });
        for (int f : order) {
            double step = cap[f] - xf[f];
            if (step < 1.0) continue;
            const uint32_t b = (uint32_t)P.block_of_flat[f];
            const double *ba = &bact[(size_t)b * MMAX_BLOCK];
            for (int r = 0; r < (int)T.blk_m[b] && step >= 1.0; r++) { const double a = T.col_a[(size_t)f * MMAX_BLOCK + r]; if (a > 0.0) { const double room = T.blk_cap[(size_t)b * MMAX_BLOCK + r] - ba[r]; if (room < a) { step = 0.0; break; } step = std::min(step, std::floor(room / a + 1e-9)); } }
            for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1] && step >= 1.0; e++) {
                const double a = (double)T.w_coef[e];
                if (!(a > 0.0)) continue;   // (a `>=` row entered negated: more of the column only helps it)
                const int g = T.w_row[e];
                for (int q = P.gr_off[g]; q < P.gr_off[g + 1]; q++) { const int k = P.gr_row[q]; const double room = P.h[k] - (ga[g] + fl[k]); if (room < 0.5 * a) { step = 0.0; break; } step = std::min(step, std::floor(room / a + 1e-9)); }
            }
            if (step < 1.0) continue;
            xf[f] += step;
            double *bw = &bact[(size_t)b * MMAX_BLOCK];
            for (int r = 0; r < MMAX_BLOCK; r++) bw[r] += T.col_a[(size_t)f * MMAX_BLOCK + r] * step;
            for (uint32_t e = T.col_woff[f]; e < T.col_woff[f + 1]; e++) ga[T.w_row[e]] += (double)T.w_coef[e] * step;
        }
        double z = 0.0;
        for (uint32_t f = 0; f < T.n_cols; f++) { x[P.model_of[f]] = xf[f]; z += T.col_cost[f] * xf[f]; }
        for (int g = 0; g < G; g++) z += P.gcost[g] * B[g];
        value = z;
        return true;
    }
};

}  // namespace hqprice
