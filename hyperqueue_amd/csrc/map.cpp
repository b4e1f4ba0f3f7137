// hqmap::Mapper (map.h): the host side of the mapping — GPU phase C on the plan of map_core.h.
#include "map.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace hqmap {

#define HQ_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// a launch wrapper that was handed a timer (hqk::time_next_launch) but returned without launching must not leave it to the next launch
#define HQ_HIP_TIMED(call) do { hipError_t e_ = (call); hqk::take_launch_timer(); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// The last launch of a phase carries a stop event (the dispatch's own completion signal) that the host waits on instead of the stream.  `launched` = the wrapper
// really launched (it consumed the pending timer) and waiting on the kernel is not switched off; otherwise the caller falls back to the stream.
#define HQ_HIP_LAST(call, launched) do { hipError_t e_ = (call); (launched) = hqk::take_launch_timer().stop == nullptr && e.wait_on_kernel; if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

namespace {
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// duration between two dispatch events in us, or -1 when the pair was not recorded by a launch of this tick (the runtime's error state is
// cleared: an unrecorded event must not surface as the "last error" of the next launch)
double elapsed_us(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) return (double)ms * 1000.0;
    (void)hipGetLastError();
    return -1.0;
}
}  // namespace

void Timeline::mark() const { if (*n < 32) tl[(*n)++] = now_us() - t0; }

void Mapper::release() {
    hqbuf::DevBuf *bufs[] = {&d_sel_task, &d_sel_level, &d_map, &d_tsweep, &d_bits, &d_pre};
    for (hqbuf::DevBuf *b : bufs) b->release();
    h_plan.release(); h_rec.release(); h_sinkhdr.release(); h_k5a.release();
}

uint32_t *Mapper::plan_storage(void *mapper, size_t words) {
    Mapper *m = static_cast<Mapper *>(mapper);
    return m->h_plan.ensure(words * 4 + 64) ? m->h_plan.as<uint32_t>() : nullptr;
}

// K5a needs the key tables only (counts in Map order per key): it goes out as soon as plan_keys() has them, reading its small tables in place
// from pinned memory, and runs while the host plans redirects, prefills and outputs — 5.4 us and a launch boundary off the critical path.
int Mapper::launch_sweep_early(const Env &e) {
    const Plan &ps = plan; const uint32_t nkeys = ps.nkeys;
    sweep_launched = false;
    if (nkeys == 0 || ps.n_bit_words == 0 || ps.max_nk > hqk::SWEEP_MAX_WORKERS) return 0;  // (the capacity error is reported by check_capacity)
    if (ps.n_tr == nkeys) { sweep_launched = true; return 0; }  // every key is stored worker-major: no bit row is ever read — no launch at all
    if (sweep_inflight) { HQ_HIP(hipStreamSynchronize(e.stream)); sweep_inflight = false; }  // a tick that failed after its early launch: its kernel still reads h_k5a
    if (!h_k5a.ensure(sweep_words(nkeys, ps.ord_cnt.size()) * 4 + 64) || !d_tsweep.ensure((size_t)ps.key_t_off[nkeys] * 4 + 16) || !d_bits.ensure((size_t)ps.n_bit_words * 8 + 16) ||
        !d_pre.ensure((size_t)ps.n_bit_words * 4 + 16))
        return fail(HQTICK_E_DEVICE, "hipMalloc mapping");
    const SweepTables t = pack_sweep_keys(h_k5a.as<uint32_t>(), ps);
    const uint32_t *d = h_k5a.dev<uint32_t>();
    hqk::MapKeys mk{};
    mk.n_keys = nkeys; mk.key_t_off = d + t.o_toff; mk.key_ord_off = d + t.o_ordoff; mk.key_bits_off = d + t.o_boff; mk.ord_cnt = d + t.o_ord; mk.key_tr = d + t.o_tr;
    mk.t_sweep = d_tsweep.as<uint32_t>(); mk.bits = d_bits.as<uint64_t>(); mk.pre = d_pre.as<uint32_t>();
    if (e.timing) hqk::time_next_launch(e.k5a_start, e.k5a_stop);
    HQ_HIP_TIMED(hqk::sweep_bits(mk, ps.max_count, ps.max_nk, e.stream));
    sweep_launched = true; sweep_inflight = true;
    return 0;
}

int Mapper::check_capacity(bool ordered) {
    const Plan &ps = plan;
    if (hqk::expand_mapping_lds(ps.max_items, ps.nkeys, ps.compact ? ps.max_out : 0, ps.may_reorder, ordered) > 150 * 1024) return fail(HQTICK_E_CAPACITY, "a worker receives more tasks in one tick than the mapping kernel stages in LDS");
    if (ps.max_nk > hqk::SWEEP_MAX_WORKERS) return fail(HQTICK_E_CAPACITY, "more than 24576 workers share one (request, variant) placement: beyond the round-robin kernel's LDS staging");
    return 0;
}

// GPU phase C: selection, round-robin bit rows, per-worker expansion; records land in pinned memory (or the HBM sink)
int Mapper::phase_c(const Env &e, const PhaseC &pc) {
    Plan &ps = plan; const hqscan::Scan &sc = *pc.sc; const hqhost::Counts &cnt = *pc.in->cnt; const hqtick_snapshot *s = pc.in->s;
    const uint32_t W = s->n_workers, Q = s->n_requests, nkeys = ps.nkeys, n_sel = ps.n_sel, n_rec = ps.n_rec;
    const bool compact = ps.compact;
    t_ = Timings{};
    size_t n_mn_ids = 0; for (auto &sets : cnt.mn_sets) n_mn_ids += sets.size();
    delta16 = compact && (e.flags & HQTICK_FLAG_COMPACT_DELTA16) != 0;
    if (compact) {  // [rec_lo u32 x n_rec | units u16 x 4 n_rec][run_span (start, count) x W][runs 12 | 16 B x n_rec] (at most one run per record)
        o_rs = delta16 ? (size_t)n_rec * 8 : (((size_t)n_rec * 4 + 7) & ~(size_t)7); o_rf = o_rs + (size_t)W * 8;
        o_rv = o_rk = 0; o_mn = (o_rf + (size_t)n_rec * (delta16 ? 16 : 12) + 7) & ~(size_t)7;
    } else { o_rv = (size_t)n_rec * 8; o_rk = o_rv + n_rec; o_mn = (o_rk + n_rec + 7) & ~(size_t)7; }
    o_fl = o_mn + n_mn_ids * 8;
    const size_t rec_bytes = o_fl + 64;
    if (!h_rec.ensure(rec_bytes)) return fail(HQTICK_E_DEVICE, "hipHostMalloc records");
    uint64_t *mn_ids = reinterpret_cast<uint64_t *>(h_rec.as<uint8_t>() + o_mn);
    if (n_sel) {
        if (!d_sel_task.ensure((size_t)n_sel * 8) || !d_sel_level.ensure((size_t)n_sel * (sc.ordered ? 4 : 2) + 4))
            return fail(HQTICK_E_DEVICE, "hipMalloc selection");
        // the plan in one upload: the big tables are already at the head of the pinned buffer (plan_keys / plan_prefill), the small ones go behind them
        const size_t o_wpos = 0, o_wcnt = (size_t)nkeys * W, o_pflj = (size_t)2 * nkeys * W;
        const SmallTables t = pack_small(h_plan.as<uint32_t>(), ps, sc, pc.ledger_pfq_rq);
        const size_t plan_words = t.words;
        if (plan_words * 4 + 16 > h_plan.cap) return fail(HQTICK_E_DEVICE, "mapping plan larger than its buffer");  // (sized in plan_keys: small_words)
        if (!d_map.ensure(plan_words * 4 + 16) ||
            !d_tsweep.ensure((size_t)ps.key_t_off[nkeys] * 4 + 16) || !d_bits.ensure((size_t)ps.n_bit_words * 8 + 16) || !d_pre.ensure((size_t)ps.n_bit_words * 4 + 16))
            return fail(HQTICK_E_DEVICE, "hipMalloc mapping");
        e.tl.mark();  // 6: pack
        const uint32_t *d = d_map.as<uint32_t>();
        hqk::MapKeys mk{};
        mk.n_keys = nkeys; mk.key_rq = d + t.o_rq; mk.key_variant = reinterpret_cast<const uint8_t *>(d + t.o_var); mk.key_seg_start = d + t.o_seg;
        mk.key_ord_off = d + t.o_ordoff; mk.ord_cnt = d + t.o_ord; mk.key_t_off = d + t.o_toff; mk.key_bits_off = d + t.o_boff; mk.key_tr = d + t.o_tr;
        mk.t_sweep = d_tsweep.as<uint32_t>(); mk.bits = d_bits.as<uint64_t>(); mk.pre = d_pre.as<uint32_t>();
        mk.wpos = d + o_wpos; mk.wcnt = d + o_wcnt; mk.rq_sel_base = d + t.o_base; mk.rq_pf_start = d + t.o_pfs; mk.rq_pf_n = d + t.o_pfn;
        mk.n_holes = (uint32_t)ps.holes.size(); mk.holes = reinterpret_cast<const uint64_t *>(d + t.o_holes);
        mk.n_pfq = ps.n_pfq; mk.pfq_src = d + t.o_pqs; mk.pfq_size = d + t.o_pqz; mk.pfl_j = d + o_pflj; mk.out_off = d + t.o_out;
        uint32_t *flags = reinterpret_cast<uint32_t *>(h_rec.as<uint8_t>() + o_fl);
        flags[0] = 0;  // K5b reports a capacity overflow straight into this pinned word
        pc.ready->selected(n_sel);  // (of the plan whose launch state is recorded below)
        const hqready::Cols cols = pc.ready->cols();
        const uint64_t N = cols.n;
        if (pc.saved_rq)  // only the redirects of Retracting tasks still look their request id up after K4 has tombstoned it (4 B per slot, device to device)
            HQ_HIP(hipMemcpyAsync(pc.saved_rq, cols.rq, N * 4, hipMemcpyDeviceToDevice, e.stream));
        last_geom = sc.geom; last_L = sc.L; last_Q = Q; last_G = sc.G; last_tb = t.o_tb; last_plan_bytes = plan_words * 4;
        last_ordered = sc.ordered;
        if (sc.ordered) {  // the plan into HBM, then K4 on the view (order.hip)
            HQ_HIP(hqk::copy_pinned_to_hbm(h_plan.dev<void>(), d_map.p, plan_words * 4, e.stream));
            hqk::OrderSelect os{};
            os.task_id = cols.id; os.perm = pc.scan->perm(); os.n_live = sc.run_cnt.empty() ? 0u : sc.run_start.back() + sc.run_cnt.back(); os.Q = Q;
            os.n_runs = (uint32_t)sc.run_cnt.size(); os.rq_sel_base = d + t.o_base; os.run_off = d + t.o_roff; os.run_start = d + t.o_rst; os.run_rank = d + t.o_rrk; os.q_tnc = d + t.o_qtnc;
            os.sel_task = d_sel_task.as<uint64_t>(); os.sel_rank = d_sel_level.as<uint32_t>(); os.err = pc.scan->select_err_dev();
            last_os = os;  // (what replay_selection launches again)
            if (pc.consume_in_tick) { os.mark_rq = cols.rq; os.mark_value = hqk::RQ_TOMBSTONE; os.mark_and_select = 1; }
            if (e.timing) hqk::time_next_launch(e.k4_start, e.k4_stop);
            HQ_HIP_TIMED(hqk::order_select(os, n_sel, e.stream));
        } else {
            if (e.timing) hqk::time_next_launch(e.k4_start, e.k4_stop);
            HQ_HIP_TIMED(hqk::select_scatter(cols.id, pc.scan->group_keys(), N, Q, sc.G, sc.geom, pc.scan->slice_table(), h_plan.as<uint32_t>() + t.o_tb,
                                d + t.o_tb, d_sel_task.as<uint64_t>(), d_sel_level.as<uint16_t>(), h_plan.dev<void>(), d_map.p, plan_words * 4,
                                pc.consume_in_tick ? cols.rq : nullptr, e.stream, pc.consume_in_tick ? 1u : 0u));
        }
        if (pc.consume_in_tick) pc.ready->consumed_in_tick();  // (confirmed when the tick returns without an error)
        if (!sweep_launched && ps.n_tr < nkeys) {
            if (e.timing) hqk::time_next_launch(e.k5a_start, e.k5a_stop);
            HQ_HIP_TIMED(hqk::sweep_bits(mk, ps.max_count, ps.max_nk, e.stream));
        }
        uint8_t *drec = h_rec.dev<uint8_t>();  // K5b writes the records straight into the caller-visible pinned buffer (PCIe-bound, no copy command)
        uint64_t *k_task = reinterpret_cast<uint64_t *>(drec); uint8_t *k_var = drec + o_rv, *k_kind = drec + o_rk;
        if (e.sink) {  // multi-GPU: records stay in HBM, laid out for the all-gather (include/hqtick.h)
            const uint32_t cap = hqtick_sink_capacity_records(W, e.sink_bytes);
            if (n_rec > cap || hqtick_sink_bytes(W, cap) > e.sink_bytes) return fail(HQTICK_E_CAPACITY, "record sink too small for this tick");
            uint8_t *sk = reinterpret_cast<uint8_t *>(e.sink);
            const size_t so_off = 16, so_task = (so_off + (size_t)(W + 1) * 4 + 7) & ~(size_t)7, so_var = so_task + (size_t)cap * 8, so_kind = so_var + cap;
            // header + rec_off: staged in pinned memory and copied with the stream
            std::vector<uint32_t> &hdr = ps.sink_hdr; hdr.assign(4 + W + 1, 0);
            hdr[0] = n_rec; hdr[1] = cnt.checksum(); hdr[2] = HQTICK_SINK_MAGIC; hdr[3] = cap;
            memcpy(hdr.data() + 4, ps.out_off.data(), (size_t)(W + 1) * 4);
            if (!h_sinkhdr.ensure(hdr.size() * 4)) return fail(HQTICK_E_DEVICE, "hipHostMalloc sink header");
            memcpy(h_sinkhdr.p, hdr.data(), hdr.size() * 4);
            HQ_HIP(hipMemcpyAsync(sk, h_sinkhdr.p, hdr.size() * 4, hipMemcpyHostToDevice, e.stream));
            k_task = reinterpret_cast<uint64_t *>(sk + so_task); k_var = sk + so_var; k_kind = sk + so_kind;
        }
        hqk::time_next_launch(e.timing ? e.k5b_start : nullptr, e.k5b_stop);  // k5b_stop: K5b's completion — what the host waits on below
        hqk::CompactOut co{};
        if (compact) co = hqk::CompactOut{reinterpret_cast<uint32_t *>(drec), reinterpret_cast<uint2 *>(drec + o_rs), reinterpret_cast<uint32_t *>(drec + o_rf),
                                          delta16 ? reinterpret_cast<uint16_t *>(drec) : nullptr};
        hqk::Stage stg = pc.stage;  // the ledger's copy of the placement stays in HBM, whatever form the records leave in
        if (stg.task) stg.pfq_rq = d_map.as<uint32_t>() + t.o_pqr;
        bool expand_is_last = false;
        if (sc.ordered) HQ_HIP_LAST(hqk::expand_mapping_wide(mk, W, d_sel_task.as<uint64_t>(), d_sel_level.as<uint32_t>(), ps.max_items, k_task, k_var, k_kind,
                                                       reinterpret_cast<uint32_t *>(drec + o_fl), co, ps.max_out, ps.may_reorder, e.stream, stg), expand_is_last);
        else HQ_HIP_LAST(hqk::expand_mapping(mk, W, d_sel_task.as<uint64_t>(), d_sel_level.as<uint16_t>(), Q, ps.max_items, k_task, k_var, k_kind,
                            reinterpret_cast<uint32_t *>(drec + o_fl), co, ps.max_out, ps.may_reorder, e.stream, stg), expand_is_last);
        if (!cnt.mn_rq.empty()) expand_is_last = false;  // copies of the multi-node task ids follow
        if (sc.ordered) {  // the selection's guard word follows (order.hip: a position outside its request's segment)
            HQ_HIP(hipMemcpyAsync(pc.scan->select_err_host(), pc.scan->select_err_dev(), 4, hipMemcpyDeviceToHost, e.stream));
            expand_is_last = false;
        }
        // multi-node tasks: the heads of their queues
        {
            size_t pos = 0;
            for (size_t i = 0; i < cnt.mn_rq.size(); i++) {
                size_t n = cnt.mn_sets[i].size();
                HQ_HIP(hipMemcpyAsync(mn_ids + pos, d_sel_task.as<uint64_t>() + ps.rq_sel_base[cnt.mn_rq[i]] + ps.mn_first[i], n * 8, hipMemcpyDeviceToHost, e.stream));
                pos += n;
            }
        }
        e.tl.mark();  // 7: phase C enqueued
        assemble_host_part(ps, res, *pc.in);
        static const bool tracing = getenv("HQMILP_TRACE") != nullptr;   // (the solver's trace: the window's lines stand next to its marks)
        const double tw0 = tracing ? now_us() : 0.0;
        if (pc.while_gpu_runs) (*pc.while_gpu_runs)();
        const double tw1 = tracing ? now_us() : 0.0;
        if (expand_is_last) HQ_HIP(hipEventSynchronize(e.k5b_stop)); else HQ_HIP(hipStreamSynchronize(e.stream));
        if (tracing && n_sel > 1000) fprintf(stderr, "[map] phase C: %.1f us of the caller's work while the kernels ran, then %.1f us waiting for them\n", tw1 - tw0, now_us() - tw1);
        sweep_inflight = false;
        if (flags[0]) return fail(HQTICK_E_CAPACITY, "mapping kernel capacity exceeded");
        if (sc.ordered && *pc.scan->select_err_host()) return fail(HQTICK_E_DEVICE, "ordered view: the selection left its request's segment");
        if (e.timing) { t_.select_us = elapsed_us(e.k4_start, e.k4_stop); t_.sweep_us = elapsed_us(e.k5a_start, e.k5a_stop); t_.other_us = elapsed_us(e.k5b_start, e.k5b_stop); }
    }
    if (!n_sel) {
        pc.ready->selected(0);
        assemble_host_part(ps, res, *pc.in);
        if (pc.while_gpu_runs) (*pc.while_gpu_runs)();
    }
    if (!n_sel && e.sink) {  // nothing placed: still publish an empty, well-formed sink
        if (hqtick_sink_bytes(W, 0) > e.sink_bytes) return fail(HQTICK_E_CAPACITY, "record sink too small for this tick");
        std::vector<uint32_t> &hdr = ps.sink_hdr; hdr.assign(4 + W + 1, 0);
        hdr[1] = cnt.checksum(); hdr[2] = HQTICK_SINK_MAGIC; hdr[3] = hqtick_sink_capacity_records(W, e.sink_bytes);
        HQ_HIP(hipMemcpy(e.sink, hdr.data(), hdr.size() * 4, hipMemcpyHostToDevice));
    }
    return 0;
}

void Mapper::export_result(const Env &e, const hqhost::Counts &cnt, hqtick_result *out) {
    const uint64_t *mn_ids = reinterpret_cast<const uint64_t *>(h_rec.as<uint8_t>() + o_mn);
    res.mn_task.clear(); res.mn_off.assign(1, 0); res.mn_worker.clear(); res.mn_rq.clear();
    {
        size_t pos = 0;
        for (size_t i = 0; i < cnt.mn_rq.size(); i++) for (auto &set : cnt.mn_sets[i]) {
            res.mn_task.push_back(mn_ids[pos++]); res.mn_rq.push_back(cnt.mn_rq[i]);
            for (uint32_t w : set) res.mn_worker.push_back(w);
            res.mn_off.push_back((uint32_t)res.mn_worker.size());
        }
    }
    out->n_counts = (uint32_t)res.cnt_rq.size(); out->count_rq = res.cnt_rq.data(); out->count_variant = res.cnt_variant.data();
    out->count_worker = res.cnt_worker.data(); out->count_value = res.cnt_value.data();
    out->rec_off = res.rec_off.data();
    const uint8_t *hb = h_rec.as<uint8_t>();
    if (plan.compact && plan.n_sel) {
        out->run_span = reinterpret_cast<const hqtick_run_span *>(hb + o_rs);
        if (delta16) { out->rec_delta16 = reinterpret_cast<const uint16_t *>(hb); out->runs16 = reinterpret_cast<const hqtick_rec_run16 *>(hb + o_rf); }
        else { out->rec_task_lo = reinterpret_cast<const uint32_t *>(hb); out->runs = reinterpret_cast<const hqtick_rec_run *>(hb + o_rf); }
    } else if (!e.sink) { out->rec_task = reinterpret_cast<const uint64_t *>(hb); out->rec_variant = hb + o_rv; out->rec_kind = hb + o_rk; }
    out->retract_off = res.retract_off.data(); out->retract_task = res.retract_task.data();
    out->n_redirects = (uint32_t)res.red_task.size(); out->redirect_task = res.red_task.data(); out->redirect_worker = res.red_worker.data(); out->redirect_variant = res.red_variant.data(); out->redirect_kind = res.red_kind.data();
    out->n_mn = (uint32_t)res.mn_task.size(); out->mn_task = res.mn_task.data(); out->mn_worker_off = res.mn_off.data(); out->mn_worker = res.mn_worker.data();
    out->new_free = res.new_free.data();
}

int Mapper::replay_selection(hipStream_t st, Replay mode, const hqready::Cols &cols, const hqscan::Scanner &scan, uint32_t n_sel, hqbuf::PinBuf *scratch) {
    const uint32_t *d = d_map.as<uint32_t>();
    if (last_ordered) {  // the view: the same selection on the same permutation — which reads no priority, so hqtick_graph_blevel after the tick changes nothing
        if (mode == REPLAY_TIMED) return fail(HQTICK_E_INVALID, "the timed replay is the dense selection's");  // (hqtick_time_kernel refuses a tick on the view itself)
        hqk::OrderSelect os = last_os;
        os.mark_rq = cols.rq; os.mark_value = mode == REPLAY_TOMBSTONE ? hqk::RQ_TOMBSTONE : 0; os.mark_and_select = 0;  // (restore: the request ids back)
        HQ_HIP(hqk::order_select(os, n_sel, st));
        if (mode == REPLAY_RESTORE) HQ_HIP(hipStreamSynchronize(st));
        return 0;
    }
    switch (mode) {
    case REPLAY_TOMBSTONE:  // tombstones instead of the selected ids (same offsets table, same plan)
        HQ_HIP(hqk::select_scatter(cols.id, scan.group_keys(), cols.n, last_Q, last_G, last_geom, scan.slice_table(), h_plan.as<uint32_t>() + last_tb, d + last_tb,
                                   d_sel_task.as<uint64_t>(), d_sel_level.as<uint16_t>(), nullptr, nullptr, 0, cols.rq, st));
        return 0;
    case REPLAY_RESTORE: {
        // the tick's K1 left a valid group key on every task that was live, so the tombstones K4 wrote are recognisable and their request ids recoverable
        // (k_restore_consumed: one pass over the key and request-id columns)
        if (!last_Q || !scratch || !scratch->ensure(64)) return fail(HQTICK_E_DEVICE, "no restore of the selection");
        uint32_t *cntp = scratch->as<uint32_t>();
        cntp[0] = 0;
        HQ_HIP(hqk::ready_restore_consumed(scan.group_keys(), cols.rq, cols.n, last_Q, scratch->dev<uint32_t>(), st));
        HQ_HIP(hipStreamSynchronize(st));
        return cntp[0] <= n_sel ? 0 : fail(HQTICK_E_DEVICE, "the restore found more tombstones than the tick selected");
    }
    case REPLAY_TIMED:
        HQ_HIP(hqk::select_scatter(cols.id, scan.group_keys(), cols.n, last_Q, last_G, last_geom, scan.slice_table(), h_plan.as<uint32_t>() + last_tb, d + last_tb,
                                   d_sel_task.as<uint64_t>(), d_sel_level.as<uint16_t>(), h_plan.dev<void>(), d_map.p, last_plan_bytes, nullptr, st));
        return 0;
    }
    return HQTICK_E_INVALID;
}

}  // namespace hqmap
