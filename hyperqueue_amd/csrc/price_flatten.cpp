// The coupled solve's flatteners: a component (price.h: Request) or the model as its builder wrote it (ModelView) -> blocks + wide rows (price_prob.h: Prob).
// One set of steps for both forms: block numbering, the global 0/1 columns, the flat numbering and the tables' allocation, what becomes of a row
// (Core::place), the never-binding rows, the wide rows' groups.  Where the forms differ, the difference is an argument or a property of the row source
// (RequestRows / ModelRows below) — never a question about who calls.  Host-only: part of both libraries and of libhqalloc.so.
#include "price_prob.h"

#include <cstdio>
#include <cstring>

#include "milp.h"

namespace hqprice {
namespace {

constexpr double INF = UNBOUNDED;
thread_local bool g_check_hints = false; thread_local int g_hint_mismatches = 0;

// What the rows loop calls per row: written out in the loop before there was one set of steps for both forms, and still compiled into it — a row costs no call.
#define HQ_PER_ROW inline __attribute__((always_inline))

typedef std::vector<std::pair<int, int32_t>> Lhs;   // a wide left-hand side over the block columns: (flat column, coefficient), sign applied

// The groups' left-hand sides -> P's row-wise and column-wise tables (P.grp_of, P.KG set; lhs[g] in the model's order)
void finish_groups(Prob &P, const std::vector<Lhs> &lhs) {
    HostTables &T = P.T;
    const int KG = P.KG;
    T.K = (uint32_t)KG;
    size_t tot = 0; for (auto &l : lhs) tot += l.size();
    // (sized once and written through pointers: ~16 k terms per tick on c3p, three passes — a push_back per term was a third of the flattening)
    P.g_off.assign((size_t)KG + 1, 0); P.g_col.resize(tot); P.g_coef.resize(tot);
    std::vector<uint32_t> gcnt(T.n_cols + 1, 0);
    {
        auto *gc = P.g_col.data(); auto *gk = P.g_coef.data(); uint32_t *cnt = gcnt.data() + 1; size_t pos = 0;
        for (int g = 0; g < KG; g++) {
            const std::pair<int, int32_t> *l = lhs[(size_t)g].data();
            for (size_t i = 0, e = lhs[(size_t)g].size(); i < e; i++) { gc[pos] = l[i].first; gk[pos] = l[i].second; cnt[l[i].first]++; pos++; }
            P.g_off[(size_t)g + 1] = (int)pos;
        }
    }
    T.col_woff.assign(T.n_cols + 1, 0);
    for (uint32_t f = 0; f < T.n_cols; f++) T.col_woff[f + 1] = T.col_woff[f] + gcnt[f + 1];
    T.w_row.resize(T.col_woff[T.n_cols]); T.w_coef.resize(T.col_woff[T.n_cols]);
    {
        std::vector<uint32_t> &cur = gcnt;   // (the counts are done with: the cursors take their place)
        for (uint32_t f = 0; f < T.n_cols; f++) cur[f] = T.col_woff[f];
        uint32_t *cp = cur.data(); uint16_t *wr = T.w_row.data(); auto *wc = T.w_coef.data();
        const auto *gc = P.g_col.data(); const auto *gk = P.g_coef.data();
        for (int g = 0; g < KG; g++) for (int e = P.g_off[g], e1 = P.g_off[g + 1]; e < e1; e++) { const uint32_t p = cp[gc[e]]++; wr[p] = (uint16_t)g; wc[p] = gk[e]; }
    }
    // rows of every group, ascending
    P.gr_off.assign((size_t)KG + 1, 0);
    for (int k = 0; k < P.K; k++) P.gr_off[P.grp_of[k] + 1]++;
    for (int g = 0; g < KG; g++) P.gr_off[g + 1] += P.gr_off[g];
    P.gr_row.resize(P.K);
    { std::vector<int> c2(P.gr_off.begin(), P.gr_off.end() - 1); for (int k = 0; k < P.K; k++) P.gr_row[c2[P.grp_of[k]]++] = k; }
}

// what a range of terms looks like to the classification: the block of its block columns (-2 none yet), more than one block, a global column, no negative
// coefficient, the count of block columns, the most the terms reach within the column bounds (summed in term order)
struct Scan { int b0 = -2; bool multi = false, has_g = false, nonneg = true; int n_bcols = 0; double amax = 0.0; };
// A row as its source hands it to Core::place: the stored terms [a, e), its kind and bounds (`<=` hi, `>=` lo; both: a range or an equality), the implied mark,
// the shared list of leading terms it names (-1 none; coefficient 1 each, not among the stored terms) with its length, and what its terms look like.
struct Row { int a = 0, e = 0; bool is_le = false, is_ge = false, implied = false; double lo = 0.0, hi = 0.0; int list = -1, list_len = 0; Scan sc; };
struct WideRow { double h; uint8_t ge; int lhs_key; int own = -1; std::vector<std::pair<int, double>> g; };   // lhs_key: 2 * list + (`>=` row), or -1 with its own list `own`

// A block row's coefficients on the ResourceAmount grid, as integers, and their gcd (0 for no terms).  rnd: the source's rounding.
template <class Rnd> HQ_PER_ROW const char *grid_terms(const double *coef, int nt, double scale, Rnd rnd, long long *vi, long long &g) {
    g = 0;
    for (int k = 0; k < nt; k++) {
        const double v = coef[k] * scale * GRID, rv = rnd(v);
        if (rv < 1.0 || std::fabs(v - rv) > 1e-6 * std::max(1.0, rv) || rv >= 4.0e15) return "block row off the ResourceAmount grid";
        vi[k] = (long long)rv;
        g = gcd_ll(g, vi[k]);
    }
    return nullptr;
}

// The steps both forms go through.  A row source (`Src`) supplies what the forms do not share:
//   sc                     the factor that gives the row's coefficients and bounds their original size back (the Request's row_scale; 1 for the model)
//   rnd(v)                 rounding to the nearest integer.  The Request form rounds with std::round, the model form with round_fast, and this stays a property of
//                          the source: wherever both are defined they lead to the same verdicts (they differ only for |v| one ulp below 0.5, where |v - rv| is 0.5
//                          either way and both tolerance tests refuse with the same text; from 2^52 up round_fast may be one off, and 4.0e15 < 2^52 refuses before
//                          that), but round_fast converts to a 64-bit integer first, which is undefined from 2^63 up and for NaN — values the Request form has
//                          always refused through std::round and never excluded beforehand.
//   grid(row, scaled, g)   the block row's grid integers divided by their gcd g, as doubles, one per stored term
//   fifth_row(row, b0)     called before a block's fifth row is refused (the Request form's trace line)
struct Core {
    Prob &P; HostTables &T;
    const int n; const int32_t *const col_group; const int *const rcol; const double *const rcoef;
    const double *ub = nullptr, *c = nullptr;   // column bounds and costs over the model's columns: given (Request) or derived (model), set before alloc_tables
    int max_group = -1, nb = 0;
    std::vector<int> block_of_group, bsize, blk, gidx;
    std::vector<WideRow> wide;
    std::vector<Lhs> own_lists;   // left-hand sides of the wide rows that name no shared list

    Core(Prob &p, int n_, const int32_t *cg, const int *rc, const double *rv) : P(p), T(p.T), n(n_), col_group(cg), rcol(rc), rcoef(rv) {}

    // blocks in order of their first column (the tick: worker order); the columns outside every block are the global ones
    const char *number_blocks() {
        for (int j = 0; j < n; j++) max_group = std::max(max_group, col_group[j]);
        block_of_group.assign((size_t)max_group + 1, -1); blk.assign(n, -1);
        for (int j = 0; j < n; j++) {
            const int g = col_group[j];
            if (g < 0) { P.gmodel.push_back(j); continue; }
            if (block_of_group[g] < 0) { block_of_group[g] = (int)bsize.size(); bsize.push_back(0); }
            blk[j] = block_of_group[g];
            if (++bsize[blk[j]] > NMAX_BLOCK) return "block with more than 32 columns";
        }
        nb = (int)bsize.size();
        if (nb < 8) return "fewer than 8 blocks";
        return nullptr;
    }
    // the global columns: 0/1 (is01: by their bound or by their kind), no negative cost
    template <class Is01> const char *take_globals(Is01 is01) {
        P.G = (int)P.gmodel.size();
        for (int j : P.gmodel) {
            if (!is01(j)) return "global column that is not 0/1";
            if (c[j] < 0.0) return "global column with negative cost";
            P.gcost.push_back(c[j]);
        }
        gidx.assign(n, -1);
        for (int g = 0; g < P.G; g++) gidx[P.gmodel[g]] = g;
        return nullptr;
    }
    // the flat numbering and the block tables, empty but for costs and caps
    const char *alloc_tables() {
        T.n_blocks = (uint32_t)nb;
        T.blk_off.assign((size_t)nb + 1, 0);
        for (int b = 0; b < nb; b++) T.blk_off[b + 1] = T.blk_off[b] + (uint32_t)bsize[b];
        T.n_cols = T.blk_off[nb];
        P.flat_of.assign(n, -1); P.model_of.assign(T.n_cols, -1); P.block_of_flat.assign(T.n_cols, -1);
        {
            std::vector<uint32_t> cur(T.blk_off.begin(), T.blk_off.end() - 1);
            for (int j = 0; j < n; j++) if (blk[j] >= 0) { const int f = (int)cur[blk[j]]++; P.flat_of[j] = f; P.model_of[f] = j; P.block_of_flat[f] = blk[j]; }
        }
        T.col_cost.assign(T.n_cols, 0.0); T.col_a.assign((size_t)T.n_cols * MMAX_BLOCK, 0.0); T.col_cap.assign(T.n_cols, 0);
        T.blk_m.assign(nb, 0); T.blk_cap.assign((size_t)nb * MMAX_BLOCK, 0.0);
        // every column of a block must be bounded by its block: a cap below 65536; amounts that do not fit even once leave ub 0
        for (uint32_t f = 0; f < T.n_cols; f++) {
            const int j = P.model_of[f];
            if (c[j] < 0.0) return "negative cost";
            if (!(ub[j] <= 65535.0)) return "column bound above 65535";
            T.col_cost[f] = c[j];
            T.col_cap[f] = (int32_t)std::floor(ub[j] + 1e-9);
        }
        return nullptr;
    }
    // the stored terms [a, e) added to what `sc` holds already (a shared list's part, or nothing)
    HQ_PER_ROW void scan(int a, int e, Scan &sc) const {
        for (int k = a; k < e; k++) {
            const int j = rcol[k];
            if (rcoef[k] < 0.0) sc.nonneg = false;
            sc.amax += rcoef[k] * ub[j];
            if (blk[j] < 0) { sc.has_g = true; continue; }
            sc.n_bcols++;
            if (sc.b0 == -2) sc.b0 = blk[j]; else if (blk[j] != sc.b0) sc.multi = true;
        }
    }

    // What becomes of one row.  nullptr: placed or passed over; else the refusal.
    template <class Src> HQ_PER_ROW const char *place(Src &src, const Row &row) {
        const int a = row.a, e = row.e;
        const Scan &sc = row.sc;
        if (row.is_le && row.is_ge) return nullptr;  // no constraint at all
        const bool vacuous = row.is_le && sc.nonneg && sc.amax <= row.hi * (1.0 + 1e-12) + 1e-9;   // a `<=` row no point within the column bounds (which the blocks carry as caps) can violate
        if (!sc.multi && !sc.has_g && sc.b0 >= 0) {  // a row of one block
            if (row.implied) return nullptr;  // implied for integer points by the block's other rows: the sweeps solve the blocks in integers
            if (vacuous) return nullptr;      // e.g. the per-worker cut rows of a large cut
            if (!row.is_le || !sc.nonneg || row.hi < 0.0) return "block row that is not a packing row";
            const int b0 = sc.b0, r = T.blk_m[b0];
            if (r >= MMAX_BLOCK) { src.fifth_row(row, b0); return "block with more than 4 rows"; }
            const double *scaled = nullptr; long long g = 1;
            if (const char *why = src.grid(row, scaled, g)) return why;
            const double capv = row.hi * src.sc * GRID;
            if (capv >= 4.0e15) return "block row capacity too large";
            const long long capi = (long long)std::floor(capv + 1e-6);
            for (int k = 0, nt = e - a; k < nt; k++) T.col_a[(size_t)P.flat_of[rcol[a + k]] * MMAX_BLOCK + r] += scaled[k];  // (duplicate terms of one row are summed)
            T.blk_cap[(size_t)b0 * MMAX_BLOCK + r] = (double)(capi / g);
            T.blk_m[b0] = (uint8_t)(r + 1);
            return nullptr;
        }
        if (!row.is_le && !row.is_ge) return "equality or range row across blocks";
        if (vacuous) return nullptr;
        if (row.is_ge && sc.nonneg && row.lo <= 1e-12) return nullptr;   // holds at zero
        if (!sc.multi && sc.has_g && sc.n_bcols >= 1 && row.is_le && sc.nonneg) {  // one block + flags: a conditional bound of the block's column(s)
            if (sc.n_bcols != 1) return "conditional bound over several columns of a block";
            CapRow cr; cr.flat = -1; cr.rhs = 0.0;
            double cx = 0.0;
            for (int k = a; k < e; k++) if (blk[rcol[k]] >= 0) { cr.flat = P.flat_of[rcol[k]]; cx = rcoef[k]; }
            if (!(cx > 0.0)) return "conditional bound with a zero coefficient";
            cr.rhs = row.hi / cx;
            for (int k = a; k < e; k++) if (blk[rcol[k]] < 0) cr.g.push_back({gidx[rcol[k]], rcoef[k] / cx});
            P.caps.push_back(std::move(cr));
            return nullptr;
        }
        if (sc.n_bcols == 0) return "row over global columns only";
        WideRow w; w.ge = row.is_ge ? 1 : 0;
        const double sign = row.is_le ? 1.0 : -1.0;
        w.h = sign * (row.is_le ? row.hi : row.lo) * src.sc;
        Lhs *own = nullptr;
        if (row.list >= 0) w.lhs_key = 2 * row.list + (row.is_ge ? 1 : 0);
        else { w.lhs_key = -1; w.own = (int)own_lists.size(); own_lists.emplace_back(); own = &own_lists.back(); own->reserve((size_t)(e - a)); }
        for (int k = a; k < e; k++) {
            const int j = rcol[k];
            const double v = sign * rcoef[k] * src.sc;
            if (blk[j] < 0) { w.g.push_back({gidx[j], v}); continue; }
            if (!own) return "block column behind a shared list";
            const double rv = Src::rnd(v);
            if (std::fabs(v - rv) > 1e-7 * std::max(1.0, std::fabs(rv)) || std::fabs(rv) > 1.0e9) return "wide row with a non-integer coefficient";
            if (rv != 0.0) own->push_back({P.flat_of[j], (int32_t)rv});
        }
        // (the block terms as the row states them, a shared list's included.  The Request form used to count the terms kept instead, one fewer per coefficient that
        // rounds to zero; the figure is read by the trace alone.)
        P.row_terms += (size_t)(e - a) - w.g.size() + (size_t)row.list_len;
        wide.push_back(std::move(w));
        if ((int)wide.size() > 1024) return "more than 1024 wide rows";
        return nullptr;
    }

    // Behind the rows: the never-binding rows, the hook, the wide rows' groups and their tables.  list_off / list_col: the shared lists the rows name (n_lists of them).
    const char *finish(const int *list_off, const int *list_col, int n_lists, const std::function<void()> *after_blocks) {
        for (int b = 0; b < nb; b++) if (T.blk_m[b] == 0) {
            // every resource row of this worker is slack at its column bounds (a nearly idle worker and a short ready set: the caps bind, not the resources).  The kernel
            // wants a row: the sum of the block's columns against the sum of their caps — never binding either.
            double total = 0.0;
            for (uint32_t f = T.blk_off[b]; f < T.blk_off[b + 1]; f++) { T.col_a[(size_t)f * MMAX_BLOCK] = 1.0; total += (double)T.col_cap[f]; }
            T.blk_cap[(size_t)b * MMAX_BLOCK] = total;
            T.blk_m[b] = 1;
        }
        if (after_blocks && *after_blocks) (*after_blocks)();
        P.K = (int)wide.size();
        if (P.K == 0) return "no wide row";
        P.h.resize(P.K); P.ge.resize(P.K); P.g_rows.assign(P.G, {});
        // Groups of rows with identical left-hand sides, numbered in the order of their first row.  Rows with the same (list, sign) share one without a look at the
        // list; lists of different families with the same content are merged too, and so is a row's own list with the same content.
        // (A hash of the left-hand side first: the rows are a thousand terms long.  ONE hash for both forms — the Request form had an FNV of its own, term by term
        // instead of pair by pair: the hash only picks the candidates for the exact comparison that decides, so which one it is cannot move a group.)
        P.grp_of.assign(P.K, -1);
        std::vector<Lhs> lhs;
        std::vector<uint64_t> lhs_hash;
        std::vector<int> group_of_key((size_t)2 * n_lists, -1);
        auto materialise = [&](int key, Lhs &out) {   // the shared list with the row's sign
            const int l = key >> 1;
            const int32_t sign = (key & 1) ? -1 : 1;
            const int k0 = list_off[l], k1 = list_off[l + 1];
            out.resize((size_t)(k1 - k0));
            std::pair<int, int32_t> *o = out.data(); const int *fo = P.flat_of.data();
            for (int k = k0; k < k1; k++) o[k - k0] = {fo[list_col[k]], sign};
        };
        auto hash_of = [](const Lhs &l) { uint64_t h = 1469598103934665603ull; for (auto &t : l) h = (h ^ ((uint64_t)(uint32_t)t.first | ((uint64_t)(uint32_t)t.second << 32))) * 1099511628211ull; return h; };
        Lhs tmp;
        for (int k = 0; k < P.K; k++) {
            WideRow &w = wide[(size_t)k];
            P.h[k] = w.h; P.ge[k] = w.ge;
            for (auto &t : w.g) P.g_rows[t.first].push_back({k, t.second});
            if (w.lhs_key >= 0 && group_of_key[(size_t)w.lhs_key] >= 0) { P.grp_of[k] = group_of_key[(size_t)w.lhs_key]; continue; }
            Lhs *l;
            if (w.lhs_key >= 0) { materialise(w.lhs_key, tmp); l = &tmp; } else l = &own_lists[(size_t)w.own];
            const uint64_t hsh = hash_of(*l);
            int g = -1;
            for (size_t i = 0; i < lhs.size() && g < 0; i++) if (lhs_hash[i] == hsh && lhs[i] == *l) g = (int)i;
            if (g < 0) { g = (int)lhs.size(); lhs.push_back(std::move(*l)); lhs_hash.push_back(hsh); }
            if (w.lhs_key >= 0) group_of_key[(size_t)w.lhs_key] = g;
            P.grp_of[k] = g;
        }
        P.KG = (int)lhs.size();
        if (P.KG > KMAX_HOST) return "more than 128 distinct wide left-hand sides";
        finish_groups(P, lhs);
        P.base_cap = T.col_cap;
        return nullptr;
    }
};

// ---- the Request's rows: scaled to max |coef| = 1 (row_scale gives the original back), bounds as a range, grid integers worked out row by row
struct RequestRows {
    const Request &rq;
    double sc = 1.0;
    std::vector<long long> vi; std::vector<double> scaled;  // (one allocation for all block rows)
    static double rnd(double v) { return std::round(v); }
    HQ_PER_ROW const char *grid(const Row &row, const double *&out, long long &g) {
        const int nt = row.e - row.a;
        vi.resize((size_t)nt); scaled.resize((size_t)nt);
        if (const char *why = grid_terms(rq.rcoef + row.a, nt, sc, [](double v) { return rnd(v); }, vi.data(), g)) return why;
        if (g < 1) g = 1;
        for (int k = 0; k < nt; k++) scaled[(size_t)k] = (double)(vi[(size_t)k] / g);
        out = scaled.data();
        return nullptr;
    }
    void fifth_row(const Row &row, int b0) const {
        if (!rq.trace) return;
        fprintf(stderr, "[price] 5th row of block %d: hi %.6f scale %.6f:", b0, row.hi, sc);
        for (int k = row.a; k < row.e; k++) fprintf(stderr, " %.6f*x%d(ub %.0f)", rq.rcoef[k] * sc, rq.rcol[k], rq.ub[rq.rcol[k]]);
        fprintf(stderr, "\n");
    }
};

// ---- the model's rows: unscaled; identical workers repeat the same few coefficient lists, so a list seen before (compared as the doubles it is) has its grid integers
// and their gcd ready — no product, rounding and 64-bit remainder per term
struct ModelRows {
    const double *rcoef;
    static constexpr double sc = 1.0;
    struct RowMemo { int n = -1; long long g = 1; double raw[32]; double scaled[64]; };
    RowMemo row_memo[8], memo_big; unsigned memo_next = 0;
    explicit ModelRows(const double *rc) : rcoef(rc) {}
    static double rnd(double v) { return round_fast(v); }
    HQ_PER_ROW const char *grid(const Row &row, const double *&out, long long &g) {
        const int a = row.a, nt = row.e - row.a;
        const RowMemo *hit = nullptr;
        for (const RowMemo &rm : row_memo) if (rm.n == nt && memcmp(rm.raw, rcoef + a, (size_t)nt * sizeof(double)) == 0) { hit = &rm; break; }
        if (!hit) {
            if (nt > 64) return "block row with more than 64 terms";
            long long vi[64], g0 = 0;
            if (const char *why = grid_terms(rcoef + a, nt, sc, [](double v) { return rnd(v); }, vi, g0)) return why;
            if (g0 < 1) g0 = 1;
            RowMemo &rm = nt <= 32 ? row_memo[memo_next++ % 8] : memo_big;
            rm.n = nt <= 32 ? nt : -1; rm.g = g0;
            if (nt <= 32) memcpy(rm.raw, rcoef + a, (size_t)nt * sizeof(double));
            for (int k = 0; k < nt; k++) rm.scaled[k] = (double)(vi[k] / g0);
            hit = &rm;
        }
        out = hit->scaled; g = hit->g;
        return nullptr;
    }
    void fifth_row(const Row &, int) const {}
};

// One flattening of the model.  What is here and not in Core is the model form's alone: the derived column bounds, the shared lists, the builder's hints
// (row_block, col_ub, block_runs) and their checks.
const char *flatten_once(const ModelView &mv, Prob &P, std::vector<double> &ub, std::vector<double> &c, double &cmax, const std::function<void()> *after_blocks) {
    const int n = mv.n, m = mv.m;
    if (!mv.col_group || !mv.row_lhs || !mv.row_lhs_len) return "no structure hints";
    Core F(P, n, mv.col_group, mv.rcol, mv.rcoef);
    if (const char *why = F.number_blocks()) return why;
    const std::vector<int> &blk = F.blk, &bsize = F.bsize, &block_of_group = F.block_of_group;
    const int nb = F.nb, max_group = F.max_group;
    cmax = 0.0;
    for (int j = 0; j < n; j++) cmax = std::max(cmax, std::fabs(mv.obj[j]));
    if (cmax == 0.0) cmax = 1.0;
    c.resize(n);
    for (int j = 0; j < n; j++) c[j] = mv.obj[j] / cmax;
    F.c = c.data();
    if (const char *why = F.take_globals([&](int j) { return mv.kind[j] == 1; })) return why;
    // ---- column bounds, as hqmilp::solve derives them: a row without a negative coefficient bounds every column it holds by floor(rhs / coef + 1e-9).  A shared list of
    // leading terms is walked once, against the smallest right-hand side of its rows (the bound is monotone in the right-hand side).
    const int n_lhs = mv.n_lists;
    for (int i = 0; i < m; i++) if (mv.row_lhs[i] >= n_lhs) return "bad structure hint";
    struct Fam { int first = -1, len = 0; bool scanned = false; double rhs_min = INF;
                 Scan sc; };   // of the list's columns (coefficient 1 each): what Core::scan would say of them
    std::vector<Fam> fam((size_t)n_lhs);
    ub.assign(n, INF);
    for (int j = 0; j < n; j++) if (mv.kind[j] == 1) ub[j] = 1.0;
    const bool hinted = mv.row_block && mv.col_ub;   // the builder's own bounds of the block columns: the rows of single blocks need not be walked for theirs
    if (hinted) for (int j = 0; j < n; j++) if (mv.col_ub[j] != UINT32_MAX) ub[j] = std::min(ub[j], (double)mv.col_ub[j]);
    auto bound_terms = [&](int a, int e, double rhs) { for (int k = a; k < e; k++) if (mv.rcoef[k] > 0.0) { double &u = ub[mv.rcol[k]]; u = std::min(u, std::floor(rhs / mv.rcoef[k] + 1e-9)); } };
    for (int l = 0; l < n_lhs; l++) for (int k = mv.list_off[l]; k < mv.list_off[l + 1]; k++) if (mv.list_col[k] < 0 || mv.list_col[k] >= n) return "bad structure hint";
    for (int i = 0; i < m; i++) {
        const int a = mv.roff[i], e = mv.roff[i + 1];
        if (a == e && mv.row_lhs[i] < 0) { const double b = mv.rhs[i]; const bool ok = mv.rtype[i] == 1 ? b >= -1e-9 : (mv.rtype[i] == 0 ? b <= 1e-9 : std::fabs(b) <= 1e-9); if (!ok) return "infeasible empty row"; continue; }
        if (hinted && mv.row_block[i] >= 0) continue;
        const int L = mv.row_lhs[i];
        bool neg = false;
        if (L >= 0) { Fam &f = fam[(size_t)L]; if (f.first < 0) { f.first = i; f.len = mv.list_off[L + 1] - mv.list_off[L]; } }
        for (int k = a; k < e; k++) if (mv.rcoef[k] < 0.0) neg = true;   // (a shared list's terms are not among the row's stored ones)
        if (mv.rtype[i] == 0 || neg) continue;   // a `>=` row, or a negative coefficient: no bound from here (the multi-node rows that do bound through one are not for this path)
        if (mv.rhs[i] < -1e-9) return "infeasible row";
        if (L >= 0) fam[(size_t)L].rhs_min = std::min(fam[(size_t)L].rhs_min, mv.rhs[i]);
        bound_terms(a, e, mv.rhs[i]);
    }
    for (int l = 0; l < n_lhs; l++) if (fam[(size_t)l].first >= 0 && fam[(size_t)l].rhs_min < INF) {   // coefficient 1: the bound is the right-hand side itself
        const double bnd = std::floor(fam[(size_t)l].rhs_min + 1e-9);
        for (int k = mv.list_off[l]; k < mv.list_off[l + 1]; k++) { double &u = ub[mv.list_col[k]]; u = std::min(u, bnd); }
    }
    // ---- equal-block runs (milp.h: Model::block_runs).  A hint like the others: every block of a run is compared with the run's first one — whole blocks with consecutive
    // numbers, the same kinds, bounds (the builder's and the ones derived above), row types, right-hand sides, implied marks, coefficients and block-relative columns, rows
    // that are their block's alone — and a run that fails anywhere is forgotten: its blocks are then flattened one by one like any other.
    struct Run { int col0, row0, term0, nbk, nc, nr, nt, b0; };
    std::vector<Run> runs;
    if (hinted && mv.block_runs) {
        long long col_end = 0, row_end = 0;
        auto holds = [&](const int32_t *r) -> bool {
            const long long col0 = r[0], row0 = r[1], term0 = r[2], nbk = r[3], nc = r[4], nr = r[5], nt = r[6];
            if (nbk < 2 || nc < 1 || nc > NMAX_BLOCK || nr < 1 || nt < 1 || col0 < col_end || row0 < row_end) return false;
            if (col0 + nbk * nc > n || row0 + nbk * nr > m) return false;
            if (mv.roff[row0] != term0 || (long long)mv.roff[row0 + nbk * nr] != term0 + nbk * nt) return false;
            const int b0 = blk[col0];
            if (b0 < 0 || b0 + nbk > nb) return false;
            for (long long t = 0; t < nt; t++) { const long long rel = (long long)mv.rcol[term0 + t] - col0; if (rel < 0 || rel >= nc) return false; }   // the first block's rows hold its own columns only
            for (long long q = 0; q < nc; q++) if (blk[col0 + q] != b0) return false;
            for (long long k = 0; k < nbk; k++) {   // whole blocks, and rows that are their block's alone
                if (bsize[b0 + k] != nc) return false;
                const int32_t gk = mv.col_group[col0 + k * nc];
                const long long rk = row0 + k * nr;
                for (long long q = 0; q < nr; q++) if (mv.row_lhs[rk + q] >= 0 || mv.row_block[rk + q] != gk) return false;
            }
            // every block against the one before it: the arrays compared with themselves, one block further on
            const size_t cs = (size_t)((nbk - 1) * nc), rs = (size_t)((nbk - 1) * nr), ts = (size_t)((nbk - 1) * nt);
            { const int *bp = blk.data() + col0; bool ok = true; for (size_t q = 0; q < cs; q++) ok &= bp[q + nc] == bp[q] + 1; if (!ok) return false; }
            if (memcmp(mv.kind + col0 + nc, mv.kind + col0, cs) != 0 || memcmp(mv.col_ub + col0 + nc, mv.col_ub + col0, cs * sizeof(uint32_t)) != 0) return false;
            if (memcmp(&ub[col0 + nc], &ub[col0], cs * sizeof(double)) != 0) return false;
            if (memcmp(mv.rtype + row0 + nr, mv.rtype + row0, rs) != 0 || memcmp(mv.rhs + row0 + nr, mv.rhs + row0, rs * sizeof(double)) != 0) return false;
            if (mv.row_implied && memcmp(mv.row_implied + row0 + nr, mv.row_implied + row0, rs) != 0) return false;
            if (memcmp(mv.rcoef + term0 + nt, mv.rcoef + term0, ts * sizeof(double)) != 0) return false;
            { const int *ro = mv.roff + row0; bool ok = true; for (size_t q = 0; q <= rs; q++) ok &= (long long)ro[q + nr] - ro[q] == nt; if (!ok) return false; }
            { const int *rc = mv.rcol + term0; bool ok = true; for (size_t q = 0; q < ts; q++) ok &= (long long)rc[q + nt] - rc[q] == nc; if (!ok) return false; }
            return true;
        };
        for (int q = 0; q < mv.n_block_runs; q++) {
            const int32_t *r = mv.block_runs + (size_t)7 * q;
            if (!holds(r)) continue;
            runs.push_back({r[0], r[1], r[2], r[3], r[4], r[5], r[6], blk[r[0]]});
            col_end = (long long)r[0] + (long long)r[3] * r[4]; row_end = (long long)r[1] + (long long)r[3] * r[5];
        }
    }
    if (hinted && g_check_hints) {   // tests: the builder's column bounds must be what the skipped single-block rows give — not tighter (a point lost), not looser
        std::vector<double> chk(n, INF);
        for (int j = 0; j < n; j++) if (mv.kind[j] == 1) chk[j] = 1.0;
        for (int i = 0; i < m; i++) {
            if (mv.row_block[i] < 0 || mv.rtype[i] == 0) continue;
            bool neg = false;
            for (int k = mv.roff[i]; k < mv.roff[i + 1]; k++) if (mv.rcoef[k] < 0.0) neg = true;
            if (neg) continue;
            for (int k = mv.roff[i]; k < mv.roff[i + 1]; k++) if (mv.rcoef[k] > 0.0) chk[mv.rcol[k]] = std::min(chk[mv.rcol[k]], std::floor(mv.rhs[i] / mv.rcoef[k] + 1e-9));
        }
        // ... unless a row that is NOT one block's alone gives it (an unbounded resource's terms carried into the next worker's row make that row such a one): then it is
        // a bound some row of the model states, which is all a hint has to be — `any` is the tightest bound a single row gives, over all rows
        std::vector<double> any(chk);
        for (int i = 0; i < m; i++) {
            if (mv.row_block[i] >= 0 || mv.rtype[i] == 0) continue;
            bool neg = false;
            for (int k = mv.roff[i]; k < mv.roff[i + 1]; k++) if (mv.rcoef[k] < 0.0) neg = true;
            if (neg) continue;
            for (int k = mv.roff[i]; k < mv.roff[i + 1]; k++) if (mv.rcoef[k] > 0.0) any[mv.rcol[k]] = std::min(any[mv.rcol[k]], std::floor(mv.rhs[i] / mv.rcoef[k] + 1e-9));
            if (mv.row_lhs[i] >= 0) for (int k = mv.list_off[mv.row_lhs[i]]; k < mv.list_off[mv.row_lhs[i] + 1]; k++) any[mv.list_col[k]] = std::min(any[mv.list_col[k]], std::floor(mv.rhs[i] + 1e-9));
        }
        for (int j = 0; j < n; j++) if (mv.col_ub[j] != UINT32_MAX && chk[j] < INF && ((double)mv.col_ub[j] > chk[j] || (double)mv.col_ub[j] < any[j])) { g_hint_mismatches++; return "structure hint: col_ub differs from what the block's rows give"; }
    }

    F.ub = ub.data();
    if (const char *why = F.alloc_tables()) return why;
    HostTables &T = P.T;
    // ---- the rows
    ModelRows src(mv.rcoef);
    // a run's first block goes through the rows below like any block; what they made of it — rows kept, their order, grid coefficients, capacities — is then copied to
    // the other blocks of the run, whose rows are passed over.  (Only where no earlier row has touched one of these blocks: the copy is then all there is to them.)
    size_t run_i = 0; bool run_live = false;
    auto stamp_run = [&](const Run &R) {
        const uint32_t f0 = T.blk_off[R.b0];
        const size_t col_bytes = (size_t)R.nc * MMAX_BLOCK * sizeof(double);
        for (int k = 1; k < R.nbk; k++) {
            const int b = R.b0 + k;
            T.blk_m[b] = T.blk_m[R.b0];
            memcpy(&T.blk_cap[(size_t)b * MMAX_BLOCK], &T.blk_cap[(size_t)R.b0 * MMAX_BLOCK], MMAX_BLOCK * sizeof(double));
            memcpy(&T.col_a[(size_t)T.blk_off[b] * MMAX_BLOCK], &T.col_a[(size_t)f0 * MMAX_BLOCK], col_bytes);
        }
        P.n_runs++; P.run_blocks += R.nbk;
    };
    for (int i = 0; i < m; i++) {
        if (run_live && i == runs[run_i].row0 + runs[run_i].nr) {
            stamp_run(runs[run_i]);
            i = runs[run_i].row0 + runs[run_i].nbk * runs[run_i].nr;
            run_live = false; run_i++;
            if (i >= m) break;
        }
        if (!run_live && run_i < runs.size() && i == runs[run_i].row0) {
            bool fresh = true;
            for (int k = 0; k < runs[run_i].nbk && fresh; k++) if (T.blk_m[runs[run_i].b0 + k] != 0) fresh = false;
            if (fresh) run_live = true; else run_i++;
        }
        Row row; row.a = mv.roff[i]; row.e = mv.roff[i + 1];
        const int a = row.a, e = row.e;
        if (a == e && mv.row_lhs[i] < 0) continue;
        row.is_le = mv.rtype[i] == 1; row.is_ge = mv.rtype[i] == 0;
        row.lo = row.hi = mv.rhs[i];
        row.implied = mv.row_implied && mv.row_implied[i];
        const int L = mv.row_lhs[i];
        Scan &sc = row.sc;
        if (L >= 0) {
            Fam &f = fam[(size_t)L];
            if (!f.scanned) {   // the list itself, once: which blocks its columns are of, what it can reach at most (coefficient 1 each)
                f.scanned = true;
                for (int k = mv.list_off[L]; k < mv.list_off[L + 1]; k++) {
                    const int j = mv.list_col[k];
                    f.sc.amax += ub[j];
                    if (blk[j] < 0) { f.sc.has_g = true; continue; }
                    f.sc.n_bcols++;
                    if (f.sc.b0 == -2) f.sc.b0 = blk[j]; else if (blk[j] != f.sc.b0) f.sc.multi = true;
                }
            }
            if (!(f.sc.multi && !f.sc.has_g)) return "shared list that is not a wide left-hand side";   // (one block's list, or a flag inside it: the plain form's business)
            sc = f.sc;
            row.list = L; row.list_len = f.len;
        }
        const int hint_b = (hinted && L < 0 && mv.row_block[i] >= 0 && mv.row_block[i] <= max_group) ? block_of_group[mv.row_block[i]] : -1;
        if (hint_b >= 0) {   // the builder says: one block's row — no need to look its columns' blocks up
            if (row.implied) continue;
            sc.b0 = hint_b; sc.n_bcols = e - a;
            const int32_t hb = mv.row_block[i];
            for (int k = a; k < e; k++) {
                if (mv.col_group[mv.rcol[k]] != hb) return "structure hint: a row_block row holds a column of another block";   // (hints are checked, not trusted)
                if (mv.rcoef[k] < 0.0) sc.nonneg = false;
                sc.amax += mv.rcoef[k] * ub[mv.rcol[k]];
            }
        } else F.scan(a, e, sc);   // (a row with a shared list: its own terms behind the list; any other row: all of it)
        if (const char *why = F.place(src, row)) return why;
    }
    if (run_live) stamp_run(runs[run_i]);   // (a run whose rows are the model's last)
    return F.finish(mv.list_off, mv.list_col, n_lhs, after_blocks);
}

}  // namespace

const char *flatten(const Request &rq, Prob &P) {
    if (!rq.col_group) return "no block hints";
    Core F(P, rq.n, rq.col_group, rq.rcol, rq.rcoef);
    F.ub = rq.ub; F.c = rq.c;
    if (const char *why = F.number_blocks()) return why;
    if (const char *why = F.take_globals([&](int j) { return rq.ub[j] == 1.0; })) return why;
    if (const char *why = F.alloc_tables()) return why;
    RequestRows src{rq};
    for (int i = 0; i < rq.m; i++) {
        Row row; row.a = rq.roff[i]; row.e = rq.roff[i + 1];
        if (row.a == row.e) continue;
        src.sc = rq.row_scale[i];
        row.is_le = rq.rlo[i] <= -INF; row.is_ge = rq.rhi[i] >= INF;
        row.lo = rq.rlo[i]; row.hi = rq.rhi[i];
        row.implied = rq.row_implied && rq.row_implied[i];
        F.scan(row.a, row.e, row.sc);
        if (const char *why = F.place(src, row)) return why;
    }
    return F.finish(nullptr, nullptr, 0, nullptr);
}

uint64_t digest_of(const Prob &P) {
    using hqmilp::fnv1a; using hqmilp::fnv1a_vec;
    const HostTables &T = P.T;
    uint64_t h = hqmilp::FNV_BASIS;
    const uint32_t dims[3] = {T.n_blocks, T.n_cols, T.K}; h = fnv1a(h, dims, sizeof dims);
    h = fnv1a_vec(h, T.blk_off); h = fnv1a_vec(h, T.blk_m); h = fnv1a_vec(h, T.blk_cap); h = fnv1a_vec(h, T.col_cost); h = fnv1a_vec(h, T.col_a); h = fnv1a_vec(h, T.col_cap);
    h = fnv1a_vec(h, T.col_woff); h = fnv1a_vec(h, T.w_row); h = fnv1a_vec(h, T.w_coef);
    const int dims2[3] = {P.K, P.G, P.KG}; h = fnv1a(h, dims2, sizeof dims2);
    h = fnv1a_vec(h, P.h); h = fnv1a_vec(h, P.ge); h = fnv1a_vec(h, P.grp_of); h = fnv1a_vec(h, P.g_off); h = fnv1a_vec(h, P.g_col); h = fnv1a_vec(h, P.g_coef);
    h = fnv1a_vec(h, P.gr_off); h = fnv1a_vec(h, P.gr_row); h = fnv1a_vec(h, P.gmodel); h = fnv1a_vec(h, P.gcost); h = fnv1a_vec(h, P.flat_of); h = fnv1a_vec(h, P.model_of);
    h = fnv1a_vec(h, P.block_of_flat); h = fnv1a_vec(h, P.base_cap);
    for (const CapRow &cr : P.caps) { h = fnv1a(h, &cr.flat, sizeof cr.flat); h = fnv1a(h, &cr.rhs, sizeof cr.rhs); for (auto &t : cr.g) { h = fnv1a(h, &t.first, sizeof t.first); h = fnv1a(h, &t.second, sizeof t.second); } }
    for (const auto &gr : P.g_rows) { const uint64_t nn = gr.size(); h = fnv1a(h, &nn, 8); for (auto &t : gr) { h = fnv1a(h, &t.first, sizeof t.first); h = fnv1a(h, &t.second, sizeof t.second); } }
    return h;
}

const char *flatten(const ModelView &mv, Prob &P, std::vector<double> &ub, std::vector<double> &c, double &cmax, const std::function<void()> *after_blocks) {
    const char *why = flatten_once(mv, P, ub, c, cmax, after_blocks);   // (the checking flatten below and flatten_for_probe have no hook)
    if (!why && g_check_hints && mv.block_runs) {   // tests: everything the runs passed over, flattened block by block after all, must come out the same
        ModelView plain = mv; plain.block_runs = nullptr; plain.n_block_runs = 0;
        Prob P2; std::vector<double> ub2, c2; double cmax2 = 0.0;
        const char *why2 = flatten_once(plain, P2, ub2, c2, cmax2, nullptr);
        if (why2 || digest_of(P2) != digest_of(P) || ub2 != ub || c2 != c || cmax2 != cmax) { g_hint_mismatches++; return "structure hint: a block run's tables differ from its blocks' own"; }
    }
    if (!why && mv.run_stats) *mv.run_stats += (uint64_t)P.run_blocks;
    if (!why && mv.tables_digest) *mv.tables_digest = digest_of(P);
    return why;
}

void flatten_for_probe(const ModelView &mv, bool trace) {
    Prob P; std::vector<double> ub, c; double cmax = 1.0;
    const char *why = flatten(mv, P, ub, c, cmax);
    if (trace) fprintf(stderr, "[price] flattened for the probe alone: %s\n", why ? why : "tables built");
}

void set_check_hints(bool on) { g_check_hints = on; g_hint_mismatches = 0; }
int hint_mismatches() { return g_hint_mismatches; }

}  // namespace hqprice
