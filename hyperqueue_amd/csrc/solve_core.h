// The placement's solvers without HIP: what hqsolve::Solver (solve.h) and the CPU test hooks share, and what tools/solve_core_asan.cpp checks
// with no GPU and no Python.
//   BlockLayout     the staged image of one k_block_solve launch — column table, class tables, outputs — from (n_cols, R, n_entries, n_classes): the device launcher
//                   and the emulation pack and view the column table through the same offsets
//   EmulatedBlocks  k_block_solve's algorithm (block_core.h) with the wavefront emulated by a loop over its 64 lanes
//   ShardedBlocks   the class blocks of a separable tick dealt over the ranks of a sharded scheduler, completed by one all-gather
//   FnExchange      the ranks' exchange through a callback of the host (hqtick_set_exchange)
//   run_solver      run_scheduling_solver on a wired Problem, over the ranks of an exchange where one is given
//   fake_worker_set, loaded_flags, tick_status: the small derivations a query and a tick make around the solve
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <vector>

#include "block_core.h"
#include "host_model.h"
#include "price.h"

namespace hqsolve {

inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The staged image of one block-solve launch, as byte offsets: [0, o_free) the column table (what the kernel stages into LDS: 16-byte aligned, a multiple of 16
// long), [o_free, o_x) the class tables — together what the kernel reads —, [o_x, end) what it writes.  Every table starts on 8 bytes.
struct BlockLayout {
    size_t o_off = 0, o_res = 0, o_w = 0, o_kind = 0, o_amt = 0, o_pool = 0;  // ent_off [n_cols + 1] u32, ent_res [ne] u32, weight [n_cols] u32, ent_kind [ne] u8, ent_amount [ne] u64, pool [R] f64
    size_t o_free = 0, o_tot = 0, o_elig = 0;                                 // free_ [nd * R] u64, total [nd * R] u64, elig [nd] u64
    size_t o_x = 0, o_st = 0, o_steps = 0, end = 0;                           // x [nd * n_cols] u32, status [nd] u32, steps [nd] u32
    static constexpr size_t SLACK = 64;
    size_t pinned_bytes() const { return end + SLACK; }   // the pinned staging buffer: the whole image
    size_t device_bytes() const { return o_x + SLACK; }   // its copy in HBM: the inputs
};
inline BlockLayout block_layout(uint32_t n_cols, uint32_t R, uint32_t n_entries, uint32_t n_classes) {
    auto al8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t NC = n_cols, ne = n_entries, nd = n_classes;
    BlockLayout L;
    L.o_off = 0; L.o_res = al8(L.o_off + (NC + 1) * 4); L.o_w = al8(L.o_res + ne * 4); L.o_kind = al8(L.o_w + NC * 4); L.o_amt = al8(L.o_kind + ne);
    L.o_pool = L.o_amt + ne * 8; L.o_free = (L.o_pool + (size_t)R * 8 + 15) & ~(size_t)15; L.o_tot = L.o_free + nd * R * 8; L.o_elig = L.o_tot + nd * R * 8;
    L.o_x = L.o_elig + nd * 8; L.o_st = L.o_x + al8(nd * NC * 4); L.o_steps = L.o_st + al8(nd * 4); L.end = L.o_steps + al8(nd * 4);
    return L;
}
inline void put(unsigned char *dst, const void *src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); }
// the column table -> dst[0, L.o_free) (the padding between the tables is left as it is)
inline void pack_cols(unsigned char *dst, const hqblock::ColTable &ct, const BlockLayout &L) {
    const size_t NC = ct.n_cols, ne = ct.ent_off[NC];
    put(dst + L.o_off, ct.ent_off, (NC + 1) * 4); put(dst + L.o_res, ct.ent_res, ne * 4); put(dst + L.o_w, ct.weight, NC * 4);
    put(dst + L.o_kind, ct.ent_kind, ne); put(dst + L.o_amt, ct.ent_amount, ne * 8); put(dst + L.o_pool, ct.pool, (size_t)ct.R * 8);
}
// the class tables -> dst[L.o_free, L.o_x)
inline void pack_classes(unsigned char *dst, const hqblock::ClassTable &cl, uint32_t R, const BlockLayout &L) {
    const size_t nd = cl.n_classes;
    put(dst + L.o_free, cl.free_, nd * R * 8); put(dst + L.o_tot, cl.total, nd * R * 8); put(dst + L.o_elig, cl.elig, nd * 8);
}
// the tables of an image at `base` (host or device memory): the column table as one blob, which the kernel stages into LDS
inline hqblock::ColTable cols_view(const unsigned char *base, uint32_t n_cols, uint32_t R, const BlockLayout &L) {
    return hqblock::ColTable{n_cols, R, (const uint32_t *)(base + L.o_off), (const uint32_t *)(base + L.o_res), (const uint8_t *)(base + L.o_kind), (const uint64_t *)(base + L.o_amt),
                             (const uint32_t *)(base + L.o_w), (const double *)(base + L.o_pool), base, (uint32_t)L.o_free};
}
inline hqblock::ClassTable classes_view(const unsigned char *base, uint32_t n_classes, const BlockLayout &L) {
    return hqblock::ClassTable{n_classes, (const uint64_t *)(base + L.o_free), (const uint64_t *)(base + L.o_tot), (const uint64_t *)(base + L.o_elig)};
}

// k_block_solve's algorithm (csrc/block_core.h) with the wavefront emulated by a loop over its 64 lanes
struct EmulatedBlocks : hqhost::BlockSolver {
    uint32_t budget;
    explicit EmulatedBlocks(uint32_t b) : budget(b) {}
    bool solve(const hqblock::ColTable &ct, const hqblock::ClassTable &cl, const hqblock::Output &out) override {
        static thread_local std::unique_ptr<hqblock::Shared> S(new hqblock::Shared());  // (a block's working set: 26 KB, off the stack; freed when its thread ends)
        hqblock::HostWave wv;
        // the column table as ONE 16-byte-aligned allocation, as the tick stages it for the kernel (BlockLayout): the emulation then takes the LDS-staging path too
        const uint32_t NC = ct.n_cols;
        const BlockLayout L = block_layout(NC, ct.R, ct.ent_off[NC], 0);
        std::vector<hqblock::V16> store(L.o_free / 16 + 1);
        unsigned char *b = reinterpret_cast<unsigned char *>(store.data());
        pack_cols(b, ct, L);
        const hqblock::ColTable bt = cols_view(b, NC, ct.R, L);
        for (uint32_t c = 0; c < cl.n_classes; c++) hqblock::solve_block(wv, *S, (c & 1) ? ct : bt, cl, c, out, budget);  // odd classes: tables read in place
        if (corrupt_mode && corrupt_class < cl.n_classes && out.status[corrupt_class] == hqblock::ST_OK) {  // fault injection (tests/test_block_solve.py): what a wrong kernel would hand back
            uint32_t *x = out.x + (size_t)corrupt_class * NC;
            if (corrupt_mode == 1) { for (uint32_t g = 0; g < NC; g++) if (x[g]) { x[g]--; break; } }               // one task short: feasible, not maximal
            else if (corrupt_mode == 2) { for (uint32_t g = NC; g-- > 0;) if (x[g]) { x[g] += 1000; break; } }       // does not fit the rows
            else if (corrupt_mode == 3) {                                                                             // everything on ONE column: corrupt_fill = column << 16 | count
                const uint32_t col = corrupt_fill >> 16, n = corrupt_fill & 0xFFFFu;
                if (col < NC) { for (uint32_t g = 0; g < NC; g++) x[g] = 0; x[col] = n; }
            }
        }
        return true;
    }
    int corrupt_mode = 0; uint32_t corrupt_class = 0, corrupt_fill = 0;
};

// The class blocks of a separable tick over the ranks: class i of the launch goes to rank i % world (the launch is ordered longest first: a strided deal spreads the
// hard classes), every rank runs its share through the inner solver, ONE all-gather of (x, status, steps) completes the answer on every rank.  A rank whose inner
// solver fails reports its classes as unsolved — every rank then sends the same classes to its host solver, and the replicas stay in step.
struct ShardedBlocks : hqhost::BlockSolver {
    hqhost::BlockSolver &inner; hqprice::Exchange &ex; uint32_t min_classes;
    hqblock::Output p_out{}; uint32_t p_nd = 0, p_nc = 0, p_nm = 0; bool p_pass = false, p_inner_ok = false, p_pending = false;
    std::vector<uint64_t> cfree, ctot, celig; std::vector<uint32_t> dx, dst, dsteps; std::vector<unsigned char> send, recv;
    ShardedBlocks(hqhost::BlockSolver &in, hqprice::Exchange &e, uint32_t mc) : inner(in), ex(e), min_classes(mc) {}
    static uint32_t share(uint32_t nd, uint32_t r, uint32_t world) { return nd > r ? (nd - r + world - 1) / world : 0; }  // classes of rank r: r, r + world, ...
    bool overlaps() const override { return inner.overlaps(); }
    bool solve(const hqblock::ColTable &ct, const hqblock::ClassTable &cl, const hqblock::Output &out) override { return begin(ct, cl, out) && finish(); }
    bool begin(const hqblock::ColTable &ct, const hqblock::ClassTable &cl, const hqblock::Output &out) override {
        p_pass = ex.world <= 1 || cl.n_classes < min_classes;
        if (p_pass) return inner.begin(ct, cl, out);
        const uint32_t nd = cl.n_classes, R = ct.R, NC = ct.n_cols, W = ex.world, me = ex.rank;
        const uint32_t nm = share(nd, me, W);
        cfree.resize((size_t)nm * R); ctot.resize((size_t)nm * R); celig.resize(nm);
        for (uint32_t j = 0; j < nm; j++) {
            const size_t i = (size_t)me + (size_t)j * W;
            put((unsigned char *)(cfree.data() + (size_t)j * R), cl.free_ + i * R, (size_t)R * 8); put((unsigned char *)(ctot.data() + (size_t)j * R), cl.total + i * R, (size_t)R * 8); celig[j] = cl.elig[i];
        }
        dx.assign((size_t)nm * NC, 0); dst.assign(nm, hqblock::ST_UNSUPPORTED); dsteps.assign(nm, 0);
        p_out = out; p_nd = nd; p_nc = NC; p_nm = nm; p_pending = true;
        p_inner_ok = nm == 0 || inner.begin(ct, hqblock::ClassTable{nm, cfree.data(), ctot.data(), celig.data()}, hqblock::Output{dx.data(), dst.data(), dsteps.data(), nullptr});
        return true;  // (whatever the inner solver said: this rank still owes the others its part of the exchange)
    }
    bool finish() override {
        if (p_pass) return inner.finish();
        if (!p_pending) return false;
        p_pending = false;
        if (p_nm && !(p_inner_ok && inner.finish())) { std::fill(dst.begin(), dst.end(), (uint32_t)hqblock::ST_UNSUPPORTED); std::fill(dx.begin(), dx.end(), 0u); }
        const uint32_t W = ex.world, NC = p_nc, mx = share(p_nd, 0, W);
        const size_t o_st = (size_t)mx * NC * 4, o_steps = o_st + (size_t)mx * 4, bytes = (o_steps + (size_t)mx * 4 + 7) & ~(size_t)7;
        send.assign(bytes, 0); recv.resize(bytes * W);
        if (p_nm) { put(send.data(), dx.data(), (size_t)p_nm * NC * 4); memcpy(send.data() + o_st, dst.data(), (size_t)p_nm * 4); memcpy(send.data() + o_steps, dsteps.data(), (size_t)p_nm * 4); }
        const double t0 = now_us();
        if (!ex.allgather(send.data(), recv.data(), bytes)) return false;
        ex.us += now_us() - t0; ex.n_calls++; ex.n_bytes += bytes * W;
        for (uint32_t r = 0; r < W; r++) {
            const unsigned char *b = recv.data() + (size_t)r * bytes;
            const uint32_t nr = share(p_nd, r, W);
            for (uint32_t j = 0; j < nr; j++) {
                const size_t i = (size_t)r + (size_t)j * W;
                put((unsigned char *)(p_out.x + i * NC), b + (size_t)j * NC * 4, (size_t)NC * 4); memcpy(p_out.status + i, b + o_st + (size_t)j * 4, 4); memcpy(p_out.steps + i, b + o_steps + (size_t)j * 4, 4);
            }
        }
        return true;
    }
};

// The ranks' exchange of small host buffers (price.h: Exchange) through the host's callback (hqtick_set_exchange, hqtick_debug_set_exchange)
struct FnExchange : hqprice::Exchange {
    hqtick_exchange_fn fn; void *user;
    FnExchange(hqtick_exchange_fn f, void *u, uint32_t rank_, uint32_t world_) : fn(f), user(u) { rank = rank_; world = world_; }
    bool allgather(const void *send, void *recv, size_t bytes) override { return fn(user, send, recv, bytes) == 0; }
};

// What a placement solve hangs onto the Problem, and takes off again
struct Wiring { hqhost::BlockSolver *blocks; uint32_t block_min_classes; hqprice::Sweeper *pricer; uint32_t block_verify, tick_seq; hqhost::BlockMemo *memo; };
inline void wire(hqhost::Problem &pb, const Wiring &w) {
    pb.blocks = w.blocks; if (w.blocks) pb.block_min_classes = w.block_min_classes;
    pb.pricer = w.pricer; pb.block_verify = w.block_verify; pb.tick_seq = w.tick_seq; pb.memo = w.memo;
}
inline void unwire(hqhost::Problem &pb) { pb.blocks = nullptr; pb.pricer = nullptr; pb.memo = nullptr; pb.defer_row_check = false; pb.no_fast_path = false; }

// run_scheduling_solver on the Problem as it is wired; with an exchange, as one rank of a sharded scheduler: the ranks split the class blocks and the sweeps
// (no-ops below their thresholds).  shard_sweep_us (may be null): the sharded sweeper's time, where one ran.
inline hqhost::Counts run_solver(hqhost::Problem &pb, const std::vector<hqhost::TaskBatch> &batches, hqprice::Exchange *ex, uint32_t shard_min_classes, uint32_t shard_min_blocks,
                                 double *shard_sweep_us = nullptr) {
    if (!ex) return hqhost::run_scheduling_solver(pb, batches);
    hqhost::BlockSolver *const blocks = pb.blocks; hqprice::Sweeper *const pricer = pb.pricer;
    std::optional<ShardedBlocks> sh_blocks; std::optional<hqprice::ShardedSweeper> sh_sweeps;
    if (blocks) { sh_blocks.emplace(*blocks, *ex, shard_min_classes); pb.blocks = &*sh_blocks; }
    if (pricer) { sh_sweeps.emplace(*pricer, *ex, shard_min_blocks); pb.pricer = &*sh_sweeps; }
    hqhost::Counts cnt = hqhost::run_scheduling_solver(pb, batches);
    if (sh_sweeps && shard_sweep_us) *shard_sweep_us = sh_sweeps->stat_sweep_us;
    pb.blocks = blocks; pb.pricer = pricer;
    return cnt;
}

// The fake workers of a what-if query (query.rs:73-81) as the solver's worker set: fresh (free == total), nothing blocked.  The caller groups its rows
// (hqhost::group_equal_rows(fw, true)).
inline void fake_worker_set(hqhost::WorkerSet &fw, const hqtick_query_workers *fake, uint32_t R, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_variant_slots) {
    fw.n = fake->n_workers; fw.R = R; fw.id = fake->worker_id; fw.total = fake->worker_total; fw.free_ = fake->worker_total;
    fw.remaining_ns = fake->worker_remaining_ns; fw.min_util = fake->worker_min_utilization; fw.flags = nullptr; fw.group = nullptr;
    fw.vflags = vflags; fw.vtmc = vtmc; fw.n_variant_slots = n_variant_slots;
    fw.blocked.assign(fw.n, {});
}
// ... and which of them the solve loaded
inline void loaded_flags(const hqhost::Counts &cnt, uint32_t n_workers, std::vector<uint8_t> &out) {
    out.assign(n_workers, 0);
    for (auto &k : cnt.per_key) for (auto &wc : k) if (wc.second > 0) out[wc.first] = 1;
}
// the tick's status from the counts (scheduler/main.rs:57-68)
inline int tick_status(const hqhost::Counts &cnt) { return cnt.is_optimal ? HQTICK_DONE : (cnt.empty() ? HQTICK_NO_PROGRESS : HQTICK_NEED_MORE_COMPUTE); }

}  // namespace hqsolve
