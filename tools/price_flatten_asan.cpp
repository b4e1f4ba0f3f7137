// The coupled solve's flatteners (hyperqueue_amd/csrc/price_flatten.cpp) under AddressSanitizer + UBSan: a stand-alone, host-only program, every input array in an
// exact-size heap block.  Small models written by hand (8 to 11 blocks of 1 to 3 columns), in the model form (ModelView) and the component form (Request):
//   smallest     8 blocks and one wide row: every array of Prob and HostTables against a written-out table
//   refusals     one model per refusal text, in every form the text exists in
//   passed over  an implied row, a vacuous `<=` row, a `>=` row that holds at zero, an empty row, a duplicate term within a block row (summed)
//   block rows   a block with 4 rows, a block left with none (the never-binding row)
//   flags        a conditional bound with two flags, a `>=` wide row with a flag
//   grouping     three wide rows with one left-hand side and two signs; two shared lists with equal content; an own-list row with a shared list's content
//   runs         a run of 3 equal blocks that holds; one that fails in its last block; one whose rows are the model's last; one whose first block an earlier
//                row has touched — each with the digest of the same model without block_runs
//   hook         after_blocks called once, the eight block arrays at the hook and at return equal in every byte
//   both forms   the Request made of the model's rows and the model form's ub and c flattens to the same digest, with row_scale 1 and with every second row scaled by 2
// Built and run by tests/test_price_flatten.py; CPU only.
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -o price_flatten_asan tools/price_flatten_asan.cpp hyperqueue_amd/csrc/price_flatten.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../hyperqueue_amd/csrc/price_prob.h"

using namespace hqprice;

static long checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } checks++; } while (0)

template <class T> struct Arr {  // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p;
    const T *set(const std::vector<T> &v) { p.reset(new T[v.size()]); for (size_t i = 0; i < v.size(); i++) p[i] = v[i]; return p.get(); }
};
typedef std::vector<std::pair<int, double>> Terms;
enum : uint8_t { GE = 0, LE = 1, EQ = 2 };
const double INF = UNBOUNDED;

// ---------------------------------------------------------------------------------------------- a model, written by hand
struct M {
    struct Col { int32_t group; double obj; uint8_t kind; double rub; };   // rub: the column's bound in the component form, where bounds are given
    struct Row { uint8_t type; double rhs; Terms t; int list; int32_t block; uint8_t implied; };
    std::vector<Col> cols; std::vector<Row> rows; std::vector<std::vector<int>> lists;
    bool hinted = false;             // row_block / col_ub go along (col_ub: what the rows with a block give, worked out below)
    std::vector<int32_t> runs;       // block_runs, seven per run
    int col(int32_t group, double obj, double rub = 4.0, uint8_t kind = 0) { cols.push_back({group, obj, kind, rub}); return (int)cols.size() - 1; }
    int flag(double obj = 0.0) { return col(-1, obj, 1.0, 1); }
    int row(uint8_t type, double rhs, Terms t, int list = -1, int32_t block = -1, uint8_t implied = 0) { rows.push_back({type, rhs, std::move(t), list, block, implied}); return (int)rows.size() - 1; }
    int list(std::vector<int> l) { lists.push_back(std::move(l)); return (int)lists.size() - 1; }
    std::vector<int> block_cols() const { std::vector<int> v; for (size_t j = 0; j < cols.size(); j++) if (cols[j].group >= 0) v.push_back((int)j); return v; }
};
// `nb` blocks with the groups 3, 4, ...: block b has `width(b)` columns of cost 1, 2, ... and the row  0.5 (x + x' + ...) <= 2  (every column bounded by 4)
template <class W> static M blocks(int nb, W width, bool block_rows = true) {
    M m;
    for (int b = 0; b < nb; b++) {
        Terms t;
        for (int q = 0; q < width(b); q++) { const int j = m.col(3 + b, (double)m.cols.size() + 1.0); t.push_back({j, 0.5}); }
        if (block_rows) m.row(LE, 2.0, t, -1, 3 + b);
    }
    return m;
}
static M base(int nb = 8) { return blocks(nb, [](int b) { return 1 + b % 3; }); }
static Terms ones(const std::vector<int> &cols, double v = 1.0) { Terms t; for (int j : cols) t.push_back({j, v}); return t; }
static M with_wide(M m) { m.row(LE, 5.0, ones(m.block_cols())); return m; }

// the model form of M
struct View {
    ModelView mv; uint64_t run_blocks = 0, digest = 0;
    Arr<double> obj, rhs, rcoef; Arr<uint8_t> kind, rtype, implied; Arr<int> roff, rcol, list_off, list_col; Arr<int32_t> group, row_lhs, row_lhs_len, row_block, runs; Arr<uint32_t> col_ub;
    explicit View(const M &m) {
        std::vector<double> o, rh, rc; std::vector<uint8_t> kd, rt, im; std::vector<int> ro{0}, rl, lo{0}, lc; std::vector<int32_t> gr, lhs, len, rb; std::vector<uint32_t> cu(m.cols.size(), UINT32_MAX);
        for (auto &c : m.cols) { o.push_back(c.obj); kd.push_back(c.kind); gr.push_back(c.group); }
        for (auto &l : m.lists) { lc.insert(lc.end(), l.begin(), l.end()); lo.push_back((int)lc.size()); }
        for (auto &r : m.rows) {
            rt.push_back(r.type); rh.push_back(r.rhs); im.push_back(r.implied); lhs.push_back(r.list); len.push_back(r.list >= 0 && r.list < (int)m.lists.size() ? (int32_t)m.lists[r.list].size() : 0); rb.push_back(r.block);
            for (auto &t : r.t) { rl.push_back(t.first); rc.push_back(t.second); if (r.block >= 0 && r.type != GE && t.second > 0.0) cu[t.first] = std::min(cu[t.first], (uint32_t)std::floor(r.rhs / t.second + 1e-9)); }
            ro.push_back((int)rl.size());
        }
        mv.n = (int)m.cols.size(); mv.m = (int)m.rows.size();
        mv.obj = obj.set(o); mv.kind = kind.set(kd); mv.rtype = rtype.set(rt); mv.rhs = rhs.set(rh); mv.roff = roff.set(ro); mv.rcol = rcol.set(rl); mv.rcoef = rcoef.set(rc);
        mv.col_group = group.set(gr); mv.row_implied = implied.set(im); mv.row_lhs = row_lhs.set(lhs); mv.row_lhs_len = row_lhs_len.set(len);
        mv.list_off = list_off.set(lo); mv.list_col = list_col.set(lc); mv.n_lists = (int)m.lists.size();
        if (m.hinted) { mv.row_block = row_block.set(rb); mv.col_ub = col_ub.set(cu); }
        if (!m.runs.empty()) { mv.block_runs = runs.set(m.runs); mv.n_block_runs = (int)m.runs.size() / 7; }
        mv.run_stats = &run_blocks; mv.tables_digest = &digest;
    }
};
// the component form of M: shared lists expanded in front of the rows' own terms, bounds and costs given; row_scale 1, or 2 on every second row (coefficients
// and bounds halved, which is exact)
struct Req {
    Request rq;
    Arr<double> rcoef, rlo, rhi, scale, c, ub; Arr<int> roff, rcol; Arr<int32_t> group; Arr<uint8_t> implied;
    Req(const M &m, const std::vector<double> &ub_, const std::vector<double> &c_, bool scaled = false) {
        std::vector<double> rc, lo, hi, sc; std::vector<int> ro{0}, rl; std::vector<int32_t> gr; std::vector<uint8_t> im;
        for (auto &col : m.cols) gr.push_back(col.group);
        for (auto &r : m.rows) {
            const double by = scaled && (sc.size() & 1) ? 2.0 : 1.0;
            sc.push_back(by);
            if (r.list >= 0) for (int j : m.lists[r.list]) { rl.push_back(j); rc.push_back(1.0 / by); }
            for (auto &t : r.t) { rl.push_back(t.first); rc.push_back(t.second / by); }
            ro.push_back((int)rl.size()); im.push_back(r.implied);
            lo.push_back(r.type == LE ? -INF : r.rhs / by); hi.push_back(r.type == GE ? INF : r.rhs / by);
        }
        rq.n = (int)m.cols.size(); rq.m = (int)m.rows.size();
        rq.roff = roff.set(ro); rq.rcol = rcol.set(rl); rq.rcoef = rcoef.set(rc); rq.rlo = rlo.set(lo); rq.rhi = rhi.set(hi);
        rq.row_scale = scale.set(sc); rq.row_implied = implied.set(im); rq.col_group = group.set(gr);
        rq.c = c.set(c_); rq.ub = ub.set(ub_);
    }
    explicit Req(const M &m) : Req(m, given(m, false), given(m, true)) {}
    static std::vector<double> given(const M &m, bool cost) { std::vector<double> v; for (auto &c : m.cols) v.push_back(cost ? c.obj : c.rub); return v; }
};

struct Flat { Prob P; std::vector<double> ub, c; double cmax = 0.0; const char *why = nullptr; uint64_t run_blocks = 0, digest = 0; };
static void flat_model(const M &m, Flat &f, bool with_runs = true) {
    View v(m);
    if (!with_runs) { v.mv.block_runs = nullptr; v.mv.n_block_runs = 0; }
    f.why = flatten(v.mv, f.P, f.ub, f.c, f.cmax);
    f.run_blocks = v.run_blocks; f.digest = v.digest;
    if (!f.why) CHECK(f.digest == digest_of(f.P), "tables_digest is not the digest of what was left");
}
static void same(const char *got, const char *want, const char *what, const char *form) {
    CHECK(got && strcmp(got, want) == 0, "%s, %s form: refused with '%s', expected '%s'", what, form, got ? got : "(accepted)", want);
}
enum { MODEL = 1, REQUEST = 2, BOTH = 3 };
static void refused(const M &m, const char *text, int forms = BOTH) {
    if (forms & MODEL) { Flat f; flat_model(m, f); same(f.why, text, text, "model"); }
    if (forms & REQUEST) { Req r(m); Prob P; same(flatten(r.rq, P), text, text, "request"); }
}
// accepted in the model form; the Request made of the same rows and the model form's ub and c must then leave the same bytes
static void accepted(const M &m, Flat &f, const char *what, bool both_forms = true) {
    flat_model(m, f);
    CHECK(!f.why, "%s: model form refused with '%s'", what, f.why);
    if (!both_forms) return;
    Req r(m, f.ub, f.c); Prob P;
    const char *why = flatten(r.rq, P);
    CHECK(!why, "%s: request form refused with '%s'", what, why);
    CHECK(digest_of(P) == f.digest, "%s: the two forms leave different tables", what);
    Req r2(m, f.ub, f.c, true); Prob P2;
    why = flatten(r2.rq, P2);
    CHECK(!why && digest_of(P2) == f.digest, "%s: rows scaled by 2 leave different tables (%s)", what, why ? why : "accepted");
}
template <class T> static void eq(const std::vector<T> &got, std::initializer_list<T> want, const char *name) {
    CHECK(got == std::vector<T>(want), "%s differs from the table (%zu entries against %zu)", name, got.size(), want.size());
}

// ---------------------------------------------------------------------------------------------- the smallest accepted model
static void smallest() {
    // 8 blocks (groups 3 .. 10), block 2 with two columns whose row is 0.5 x2 + 1.0 x3 <= 2; costs 1 .. 9; one wide row: the sum of all columns <= 5.
    // (A one-column block's row 0.5 x <= 2 is vacuous within the bound 4 it gives: those blocks get the never-binding row, x against its cap — the same numbers.)
    M m = blocks(8, [](int b) { return b == 2 ? 2 : 1; });
    m.rows[2].t[1].second = 1.0;
    m = with_wide(m);
    Flat f; accepted(m, f, "smallest");
    const Prob &P = f.P; const HostTables &T = P.T;
    CHECK(T.n_blocks == 8 && T.n_cols == 9 && T.K == 1 && P.K == 1 && P.G == 0 && P.KG == 1 && P.row_terms == 9 && f.cmax == 9.0, "dimensions");
    eq<uint32_t>(T.blk_off, {0, 1, 2, 4, 5, 6, 7, 8, 9}, "blk_off");
    eq<uint8_t>(T.blk_m, {1, 1, 1, 1, 1, 1, 1, 1}, "blk_m");
    eq<double>(T.blk_cap, {4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0}, "blk_cap");
    eq<double>(T.col_cost, {1.0 / 9, 2.0 / 9, 3.0 / 9, 4.0 / 9, 5.0 / 9, 6.0 / 9, 7.0 / 9, 8.0 / 9, 9.0 / 9}, "col_cost");
    eq<double>(T.col_a, {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, "col_a");
    eq<int32_t>(T.col_cap, {4, 4, 4, 2, 4, 4, 4, 4, 4}, "col_cap");
    eq<uint32_t>(T.col_woff, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, "col_woff");
    eq<uint16_t>(T.w_row, {0, 0, 0, 0, 0, 0, 0, 0, 0}, "w_row");
    eq<int32_t>(T.w_coef, {1, 1, 1, 1, 1, 1, 1, 1, 1}, "w_coef");
    eq<int>(P.flat_of, {0, 1, 2, 3, 4, 5, 6, 7, 8}, "flat_of"); eq<int>(P.model_of, {0, 1, 2, 3, 4, 5, 6, 7, 8}, "model_of");
    eq<int>(P.block_of_flat, {0, 1, 2, 2, 3, 4, 5, 6, 7}, "block_of_flat");
    eq<int>(P.gmodel, {}, "gmodel"); eq<double>(P.gcost, {}, "gcost"); CHECK(P.g_rows.empty() && P.caps.empty(), "no flags, no conditional bounds");
    eq<double>(P.h, {5}, "h"); eq<uint8_t>(P.ge, {0}, "ge"); eq<int>(P.grp_of, {0}, "grp_of");
    eq<int>(P.g_off, {0, 9}, "g_off"); eq<int>(P.g_col, {0, 1, 2, 3, 4, 5, 6, 7, 8}, "g_col"); eq<int32_t>(P.g_coef, {1, 1, 1, 1, 1, 1, 1, 1, 1}, "g_coef");
    eq<int>(P.gr_off, {0, 1}, "gr_off"); eq<int>(P.gr_row, {0}, "gr_row");
    eq<int32_t>(P.base_cap, {4, 4, 4, 2, 4, 4, 4, 4, 4}, "base_cap");
    eq<double>(f.ub, {4, 4, 4, 2, 4, 4, 4, 4, 4}, "ub");
}

// ---------------------------------------------------------------------------------------------- one model per refusal text
static void refusals() {
    { M m = with_wide(base()); Req r(m); r.rq.col_group = nullptr; Prob P; same(flatten(r.rq, P), "no block hints", "no block hints", "request"); }
    { M m = with_wide(base()); View v(m); v.mv.row_lhs = nullptr; Prob P; std::vector<double> ub, c; double cmax; same(flatten(v.mv, P, ub, c, cmax), "no structure hints", "no structure hints", "model"); }
    refused(with_wide(blocks(8, [](int b) { return b == 5 ? 33 : 1; })), "block with more than 32 columns");
    refused(with_wide(base(7)), "fewer than 8 blocks");
    { M m = base(); const int g = m.col(-1, 0.0, 2.0, 0); Terms t = ones(m.block_cols()); t.push_back({g, -3.0}); m.row(LE, 5.0, t); refused(m, "global column that is not 0/1"); }
    { M m = base(); const int g = m.flag(-1.0); Terms t = ones(m.block_cols()); t.push_back({g, -3.0}); m.row(LE, 5.0, t); refused(m, "global column with negative cost"); }
    { M m = with_wide(base()); m.cols[4].obj = -1.0; refused(m, "negative cost"); }
    { M m = base(); m.col(3 + 8, 1.0, 70000.0); m.row(GE, 1.0, ones(m.block_cols())); refused(m, "column bound above 65535"); }   // (model form: a column no row bounds)
    { M m = with_wide(base()); m.row(GE, 1.0, {{1, 1.0}, {2, 1.0}}, -1, 4); refused(m, "block row that is not a packing row"); }
    {   // block 1 (columns 1, 2): its own row bounds both by 4, the four rows behind it do not tighten that and none is vacuous
        M m = with_wide(base());
        const double abr[4][3] = {{1, 2, 8}, {2, 1, 8}, {1, 3, 12}, {3, 1, 12}};
        for (auto &q : abr) m.row(LE, q[2], {{1, q[0]}, {2, q[1]}}, -1, 4);
        refused(m, "block with more than 4 rows");
        Req r(m); r.rq.trace = true; Prob P; same(flatten(r.rq, P), "block with more than 4 rows", "the fifth row's trace line", "request");
    }
    { M m = with_wide(base()); m.row(LE, 0.0003, {{1, 0.00015}, {2, 0.00015}}, -1, 4); refused(m, "block row off the ResourceAmount grid"); }
    { M m = with_wide(base()); m.row(LE, 5e11, {{1, 1e11}, {2, 1e11}}, -1, 4); refused(m, "block row capacity too large"); }
    { M m = with_wide(base()); m.row(EQ, 3.0, {{0, 1.0}, {1, 1.0}}); refused(m, "equality or range row across blocks"); }
    { M m = with_wide(base()); const int g = m.flag(); m.row(LE, 4.0, {{1, 1.0}, {2, 1.0}, {g, 4.0}}); refused(m, "conditional bound over several columns of a block"); }
    { M m = with_wide(base()); const int g = m.flag(), g2 = m.flag(); m.row(LE, 1.0, {{0, 0.0}, {g, 1.0}, {g2, 1.0}}); refused(m, "conditional bound with a zero coefficient"); }
    { M m = with_wide(base()); const int g = m.flag(), g2 = m.flag(); m.row(LE, 1.0, {{g, 1.0}, {g2, 1.0}}); refused(m, "row over global columns only"); }
    { M m = with_wide(base()); m.row(GE, 1.0, {{0, 1.5}, {1, 1.0}}); refused(m, "wide row with a non-integer coefficient"); }
    { M m = base(); for (int k = 0; k < 1025; k++) m.row(LE, 5.0 + k / 128.0, ones(m.block_cols())); refused(m, "more than 1024 wide rows"); }
    refused(base(), "no wide row");
    { M m = base(); for (int k = 0; k < 129; k++) m.row(GE, 1.0, {{0, k + 1.0}, {1, 1.0}}); refused(m, "more than 128 distinct wide left-hand sides"); }
    { M m = base(); for (int k = 0; k < 128; k++) m.row(GE, 1.0, {{0, k + 1.0}, {1, 1.0}}); Flat f; accepted(m, f, "128 distinct left-hand sides"); CHECK(f.P.KG == 128, "groups"); }
    // the model form's own
    { M m = with_wide(base()); m.rows.back().list = 0; refused(m, "bad structure hint", MODEL); }                                      // a list that does not exist
    { M m = with_wide(base()); const int l = m.list({0, 99}); m.row(LE, 5.0, {}, l); refused(m, "bad structure hint", MODEL); }        // a list with a column that does not exist
    { M m = with_wide(base()); m.row(LE, -1.0, {}); refused(m, "infeasible empty row", MODEL); }
    { M m = with_wide(base()); m.row(GE, 1.0, {}); refused(m, "infeasible empty row", MODEL); }
    { M m = with_wide(base()); m.row(EQ, 1.0, {}); refused(m, "infeasible empty row", MODEL); }
    { M m = with_wide(base()); m.row(LE, -1.0, {{0, 1.0}, {1, 1.0}}); refused(m, "infeasible row", MODEL); }
    { M m = with_wide(base()); const int l = m.list({1, 2}); m.row(LE, 3.0, {}, l); refused(m, "shared list that is not a wide left-hand side", MODEL); }   // one block's list
    { M m = with_wide(base()); const int g = m.flag(); const int l = m.list({0, 1, g}); m.row(LE, 1.0, {}, l); refused(m, "shared list that is not a wide left-hand side", MODEL); }   // a flag inside
    { M m = with_wide(base()); m.hinted = true; m.row(LE, 4.0, {{1, 1.0}, {3, 1.0}}, -1, 4); refused(m, "structure hint: a row_block row holds a column of another block", MODEL); }
    { M m = with_wide(base()); Terms t; for (int k = 0; k < 65; k++) t.push_back({1 + k % 2, 1.0}); m.row(LE, 100.0, t, -1, 4); refused(m, "block row with more than 64 terms", MODEL); }
    { M m = base(); const int l = m.list(m.block_cols()); m.row(LE, 5.0, {{0, 1.0}}, l); refused(m, "block column behind a shared list", MODEL); }
    {   // a builder's bound looser than its block's row gives (the row is 0.5 x <= 2); counted, and only looked for under set_check_hints
        M m = with_wide(base()); m.hinted = true;
        View v(m); std::vector<uint32_t> cu(v.mv.col_ub, v.mv.col_ub + v.mv.n); cu[0] = 5; Arr<uint32_t> wrong; v.mv.col_ub = wrong.set(cu);
        Prob P0; std::vector<double> ub, c; double cmax;
        CHECK(!flatten(v.mv, P0, ub, c, cmax), "unchecked, a loose col_ub passes");
        set_check_hints(true);
        Prob P; same(flatten(v.mv, P, ub, c, cmax), "structure hint: col_ub differs from what the block's rows give", "col_ub", "model");
        CHECK(hint_mismatches() == 1, "the mismatch is counted");
        Flat f; flat_model(m, f); CHECK(!f.why && hint_mismatches() == 1, "the right hints pass the check");
        set_check_hints(false);
        CHECK(hint_mismatches() == 0, "switching the check resets the count");
    }
}

// ---------------------------------------------------------------------------------------------- rows passed over, several rows per block
static void passed_over() {
    M plain = with_wide(base());
    Flat f0; accepted(plain, f0, "plain");
    {
        M m = with_wide(base());
        m.row(LE, 8.0, {{1, 1.0}, {2, 2.0}}, -1, 4, 1);   // implied: binding within the bounds 4, 4 (it gives no tighter ones), and only its mark keeps it out of block 1
        m.row(LE, 8.0, {{1, 1.0}, {2, 1.0}}, -1, 4);      // vacuous within the bounds 4, 4
        m.row(LE, 100.0, ones(m.block_cols()));           // vacuous across the blocks
        m.row(GE, 0.0, ones(m.block_cols()));             // holds at zero
        m.row(LE, 0.0, {});                                // empty
        Flat f; accepted(m, f, "rows passed over");
        CHECK(f.digest == f0.digest, "rows that are passed over changed the tables");
    }
    {   // a duplicate term within one block row is summed: 0.5 x1 + 0.5 x2 + 0.5 x2 <= 2
        M m = with_wide(base());
        m.rows[1].t.push_back({2, 0.5});
        Flat f; accepted(m, f, "duplicate term");
        CHECK(f.P.T.col_a[1 * 4] == 1.0 && f.P.T.col_a[2 * 4] == 2.0 && f.P.T.blk_cap[1 * 4] == 4.0 && f.P.T.col_cap[2] == 4, "the duplicate term of column 2 is summed");
    }
    {   // block 1 with four rows (its own and three more), block 3 left with none
        M m = base();
        m.rows.erase(m.rows.begin() + 3);
        const double abr[3][3] = {{1, 2, 8}, {2, 1, 8}, {1, 3, 12}};
        for (auto &q : abr) m.row(LE, q[2], {{1, q[0]}, {2, q[1]}}, -1, 4);
        m = with_wide(m);   // (what bounds block 3's column: by 5)
        Flat f; accepted(m, f, "four rows, no row");
        const HostTables &T = f.P.T;
        CHECK(T.blk_m[1] == 4 && T.blk_m[3] == 1, "rows per block");
        const double a1[4] = {1, 1, 2, 1}, a2[4] = {1, 2, 1, 3}, cap1[4] = {4, 8, 8, 12};
        CHECK(memcmp(&T.col_a[1 * 4], a1, sizeof a1) == 0 && memcmp(&T.col_a[2 * 4], a2, sizeof a2) == 0 && memcmp(&T.blk_cap[1 * 4], cap1, sizeof cap1) == 0, "block 1's four rows");
        const uint32_t f3 = T.blk_off[3];
        CHECK(T.blk_off[4] - f3 == 1 && T.col_a[(size_t)f3 * 4] == 1.0 && T.col_cap[f3] == 5 && T.blk_cap[3 * 4] == 5.0 && T.col_a[(size_t)f3 * 4 + 1] == 0.0, "block 3's never-binding row: its column against its cap");
    }
}

// ---------------------------------------------------------------------------------------------- conditional bounds, flags, groups
static void flags_and_groups() {
    {
        M m = with_wide(base());
        const int g0 = m.flag(0.25), g1 = m.flag(0.5);
        m.row(LE, 4.0, {{g0, 2.0}, {3, 2.0}, {g1, 1.0}});            // x3 + B0 + 0.5 B1 <= 2
        Terms t = ones(m.block_cols()); t.push_back({g1, 3.0});
        m.row(GE, 3.0, t);                                            // sum x + 3 B1 >= 3
        Flat f; accepted(m, f, "conditional bound, flags");
        const Prob &P = f.P;
        CHECK(P.G == 2 && P.caps.size() == 1 && P.caps[0].flat == P.flat_of[3] && P.caps[0].rhs == 2.0, "the conditional bound");
        CHECK(P.caps[0].g == (Terms{{0, 1.0}, {1, 0.5}}), "its two flags, the column's coefficient divided out");
        CHECK(P.K == 2 && P.KG == 2 && P.ge[1] == 1 && P.h[1] == -3.0 && P.g_rows[1] == (Terms{{1, -3.0}}) && P.g_rows[0].empty(), "the `>=` row, negated, with its flag");
        CHECK(P.g_coef[(size_t)P.g_off[1]] == -1 && P.gcost[1] == 0.5 / f.cmax, "negated coefficients; the flags' costs scaled like the others");
    }
    {   // three wide rows over one left-hand side, two signs: <= 5, <= 6 and >= 1 — two groups (the signs differ), in order of first row
        M m = with_wide(base());
        m.row(GE, 1.0, ones(m.block_cols()));
        m.row(LE, 6.0, ones(m.block_cols()));
        Flat f; accepted(m, f, "one left-hand side, two signs");
        eq<int>(f.P.grp_of, {0, 1, 0}, "grp_of"); eq<int>(f.P.gr_off, {0, 2, 3}, "gr_off"); eq<int>(f.P.gr_row, {0, 2, 1}, "gr_row");
    }
    {   // two shared lists with equal content merge; a row with its own list of the same content joins them; a second row of a list takes its group without a look
        M m = base();
        const int l0 = m.list(m.block_cols()), l1 = m.list(m.block_cols());
        const int g = m.flag();
        m.row(LE, 5.0, {}, l0); m.row(LE, 6.0, {{g, -2.0}}, l1); m.row(LE, 7.0, ones(m.block_cols())); m.row(GE, 1.0, {}, l1); m.row(LE, 8.0, {}, l1);
        Flat f; accepted(m, f, "shared lists");
        eq<int>(f.P.grp_of, {0, 0, 0, 1, 0}, "grp_of");
        CHECK(f.P.KG == 2 && f.P.row_terms == 5 * m.block_cols().size() && f.P.g_rows[0] == (Terms{{1, -2.0}}), "two groups; every row's terms counted; the flag behind a list");
    }
}

// ---------------------------------------------------------------------------------------------- equal-block runs
// 10 blocks of 2 columns and 2 rows each, hinted; blocks 2, 3, 4 equal in everything but their costs
static M run_model(bool wide_first, double last_rhs = 8.0) {
    M m; m.hinted = true;
    for (int b = 0; b < 10; b++) { m.col(3 + b, 1.0 + b); m.col(3 + b, 2.0 + b); }
    if (wide_first) m.row(LE, 5.0, ones(m.block_cols()));
    for (int b = 0; b < 10; b++) {
        const bool in_run = b >= 2 && b <= 4;
        m.row(LE, in_run ? 2.0 : 3.0, {{2 * b, 0.5}, {2 * b + 1, 0.5}}, -1, 3 + b);
        m.row(LE, b == 4 ? last_rhs : 8.0, {{2 * b, 1.0}, {2 * b + 1, 2.0}}, -1, 3 + b);
    }
    if (!wide_first) m.row(LE, 5.0, ones(m.block_cols()));
    const int row0 = (wide_first ? 1 : 0) + 2 * 2;
    m.runs = {4, row0, (wide_first ? 20 : 0) + 2 * 4, 3, 2, 2, 4};
    return m;
}
static void one_run(const M &m, uint64_t want_covered, const char *what) {
    Flat with, without;
    flat_model(m, with); flat_model(m, without, false);
    CHECK(!with.why && !without.why, "%s: refused with '%s'", what, with.why ? with.why : without.why);
    CHECK(with.digest == without.digest, "%s: the tables with the run differ from the tables without", what);
    CHECK(with.run_blocks == want_covered && without.run_blocks == 0 && with.P.run_blocks == (int)want_covered, "%s: %llu blocks taken from a run's first block", what, (unsigned long long)with.run_blocks);
    set_check_hints(true);   // the flattener's own second flatten, block by block, and its comparison
    Flat checked; flat_model(m, checked);
    CHECK(!checked.why && hint_mismatches() == 0 && checked.digest == with.digest, "%s: under the hint check", what);
    set_check_hints(false);
}
static void runs() {
    one_run(run_model(false), 3, "a run of three");
    one_run(run_model(false, 9.0), 0, "a run whose last block differs");
    one_run(run_model(true), 3, "a run behind a wide row");
    {   // the run covers the last three blocks: its rows are the model's last
        M m; m.hinted = true;
        for (int b = 0; b < 9; b++) { m.col(3 + b, 1.0 + b); m.col(3 + b, 2.0 + b); }
        m.row(LE, 5.0, ones(m.block_cols()));
        for (int b = 0; b < 9; b++) { m.row(LE, b >= 6 ? 2.0 : 3.0, {{2 * b, 0.5}, {2 * b + 1, 0.5}}, -1, 3 + b); m.row(LE, 8.0, {{2 * b, 1.0}, {2 * b + 1, 2.0}}, -1, 3 + b); }
        m.runs = {12, 13, 18 + 24, 3, 2, 2, 4};
        one_run(m, 3, "a run at the model's end");
    }
    {   // an earlier row has touched the run's first block: that block is more than what the run's rows make of it, so nothing is copied from it and the blocks go one by one
        M m; m.hinted = true;
        for (int b = 0; b < 10; b++) { m.col(3 + b, 1.0 + b); m.col(3 + b, 2.0 + b); }
        m.row(LE, 12.0, {{4, 1.0}, {5, 3.0}}, -1, 5);   // block 2's third row, in front of the run's rows
        for (int b = 0; b < 10; b++) { m.row(LE, b >= 2 && b <= 4 ? 2.0 : 3.0, {{2 * b, 0.5}, {2 * b + 1, 0.5}}, -1, 3 + b); m.row(LE, 8.0, {{2 * b, 1.0}, {2 * b + 1, 2.0}}, -1, 3 + b); }
        m.row(LE, 5.0, ones(m.block_cols()));
        m.runs = {4, 1 + 4, 2 + 8, 3, 2, 2, 4};
        one_run(m, 0, "a run whose first block is not fresh");
        Flat f; flat_model(m, f); CHECK(f.P.T.blk_m[2] == 3 && f.P.T.blk_m[3] == 2, "block 2 keeps its third row, block 3 does not get one");
    }
}

// ---------------------------------------------------------------------------------------------- the hook
static void hook() {
    M m = run_model(false);
    View v(m);
    struct Blocks { uint32_t n_blocks, n_cols; std::vector<uint32_t> blk_off; std::vector<uint8_t> blk_m; std::vector<double> blk_cap, col_cost, col_a; std::vector<int32_t> col_cap; };
    auto take = [](const HostTables &T) { return Blocks{T.n_blocks, T.n_cols, T.blk_off, T.blk_m, T.blk_cap, T.col_cost, T.col_a, T.col_cap}; };
    auto equal = [](const Blocks &a, const Blocks &b) { return a.n_blocks == b.n_blocks && a.n_cols == b.n_cols && a.blk_off == b.blk_off && a.blk_m == b.blk_m && a.blk_cap == b.blk_cap && a.col_cost == b.col_cost && a.col_a == b.col_a && a.col_cap == b.col_cap; };
    Prob P; std::vector<double> ub, c; double cmax = 0.0;
    int calls = 0; Blocks at_hook{};
    const std::function<void()> fn = [&]() { calls++; at_hook = take(P.T); CHECK(P.T.col_woff.empty() && P.K == 0, "the wide rows' tables are built behind the hook"); };
    CHECK(!flatten(v.mv, P, ub, c, cmax, &fn), "refused");
    CHECK(calls == 1, "after_blocks called %d times", calls);
    CHECK(equal(at_hook, take(P.T)) && at_hook.n_blocks == 10 && at_hook.blk_m[3] == 2, "the eight block arrays are final at the hook");
    const std::function<void()> none;   // an empty function is not called
    Prob P2; CHECK(!flatten(v.mv, P2, ub, c, cmax, &none) && digest_of(P2) == digest_of(P), "an empty hook");
    M bad = base();   // refused behind the hook ("no wide row"): the hook has run once all the same
    View vb(bad); Prob P3; calls = 0;
    const std::function<void()> count = [&]() { calls++; };
    same(flatten(vb.mv, P3, ub, c, cmax, &count), "no wide row", "refused behind the hook", "model");
    CHECK(calls == 1, "the hook runs before the wide rows are looked at");
}

int main() {
    smallest();
    refusals();
    passed_over();
    flags_and_groups();
    runs();
    hook();
    printf("%ld checks ok\n", checks);
    return 0;
}
