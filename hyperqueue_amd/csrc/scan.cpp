// hqscan::Scanner (scan.h): the host side of GPU phase A.
#include "scan.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

namespace hqscan {

#define HQ_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// a launch wrapper that was handed a timer (hqk::time_next_launch) but returned without launching must not leave it to the next launch
#define HQ_HIP_TIMED(call) do { hipError_t e_ = (call); hqk::take_launch_timer(); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// The last launch of a phase carries a stop event (the dispatch's own completion signal) that the host waits on instead of the stream.  `launched` = the wrapper
// really launched (it consumed the pending timer) and waiting on the kernel is not switched off; otherwise the caller falls back to the stream.
#define HQ_HIP_LAST(call, launched) do { hipError_t e_ = (call); (launched) = hqk::take_launch_timer().stop == nullptr && e.wait_on_kernel; if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

namespace {
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// duration between two dispatch events in us, or -1 when the pair was not recorded by a launch of this scan (the runtime's error state is
// cleared: an unrecorded event must not surface as the "last error" of the next launch)
double elapsed_us(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) return (double)ms * 1000.0;
    (void)hipGetLastError();
    return -1.0;
}
const char *const BAD_RQ = "ready set holds a request id >= n_requests";
bool beyond_levels(const uint32_t *hl) { return hl[2] || hl[0] == 0xFFFFFFFFu || hl[0] > hqk::MAX_LEVELS; }  // the head k_sort_levels wrote: more than MAX_LEVELS distinct priorities
}  // namespace

int Scanner::init() {
    if (const char *v = getenv("HQTICK_ORDERED_VIEW")) force_ordered = atoi(v) != 0;  // (tests: every tick on the ordered view)
    no_spec_scan = getenv("HQTICK_NO_SPEC_SCAN") != nullptr;
    if (!d_flags.ensure(64) || hipMemset(d_flags.p, 0, 64) != hipSuccess) return fail(HQTICK_E_DEVICE, "hipMalloc scan flags");
    return 0;
}

void Scanner::release() {
    hqbuf::DevBuf *bufs[] = {&d_set, &d_flags, &d_levels, &d_nlevels, &d_wave_tab, &d_hist, &d_gkey, &d_ord_hist, &d_ord_tab, &d_perm, &d_perm2, &d_ord_tiles, &d_inv};
    for (hqbuf::DevBuf *b : bufs) b->release();
    h_ord.release(); h_ordh.release(); h_a.release(); h_lv.release(); h_retr.release();
}

bool Scanner::ensure_discovery() {
    return d_set.ensure((size_t)(hqk::PRIO_SET_CAP + hqk::MAX_LEVELS) * 8) && h_lv.ensure((size_t)(hqk::MAX_LEVELS + 4) * 8) && d_flags.ensure(64) &&
           d_levels.ensure((size_t)(hqk::MAX_LEVELS + 2) * 8) && d_nlevels.ensure(64);  // (a 40-byte head: count + the first four levels, kernels.hip: k_sort_levels)
}

// Level discovery, enqueued: K0 into the priority set, K0b sorts it into d_levels and — straight into pinned memory, no copy — into h_lv, whose word 3 becomes
// *seq when everything else of it is written.  The set and the flag words are EMPTY / zero between two discoveries (k_sort_levels clears what a discovery used, the
// scan clears its own flag): the two fills are for the first one of a scanner and for the one after a discovery whose result nobody saw.  `zero`: a buffer of the
// caller's, cleared behind them.  start / stop (may be null): marker packets around K0.
int Scanner::discover(hipStream_t st, hipEvent_t start, hipEvent_t stop, const hqready::Cols &cols, uint32_t *seq, void *zero, size_t zero_bytes) {
    if (!set_clean) {
        HQ_HIP(hipMemsetAsync(d_set.p, 0xFF, (size_t)hqk::PRIO_SET_CAP * 8, st));
        HQ_HIP(hipMemsetAsync(d_flags.p, 0, 64, st));
    }
    set_clean = false;  // until the caller has seen the discovery's result
    if (zero) HQ_HIP(hipMemsetAsync(zero, 0, zero_bytes, st));
    if (start) HQ_HIP(hipEventRecord(start, st));
    HQ_HIP(hqk::distinct_priorities(cols.prio, cols.rq, cols.n, d_set.as<uint64_t>(), d_flags.as<uint32_t>(), st));
    if (stop) HQ_HIP(hipEventRecord(stop, st));
    volatile uint32_t *hl = h_lv.as<uint32_t>();
    *seq = ++lv_seq ? lv_seq : ++lv_seq;  // (never 0)
    hl[0] = 0; hl[1] = 0; hl[2] = 0; hl[3] = 0;
    HQ_HIP(hqk::sort_levels(d_set.as<uint64_t>(), d_flags.as<uint32_t>(), d_levels.as<uint64_t>(), d_nlevels.as<uint32_t>(), h_lv.dev<uint64_t>(), *seq, st));
    return 0;
}

// The ordered view (order.hip) of the columns: sc gets the runs, perm() the permutation, inv() its inverse.  One synchronisation after the digit
// histogram (which passes to run, how many live slots), one after the run table.
int Scanner::view(const Env &e, const hqready::Cols &cols, uint32_t Q, Scan *sc, const std::function<void()> *while_gpu_runs) {
    const uint64_t *prio = cols.prio; const uint32_t *rq = cols.rq; const uint64_t N = cols.n; hipStream_t st = e.stream;
    const size_t hw = (size_t)hqk::ORDER_DIGITS * 256 + 4;
    view_.valid = false; view_.passes = 0; t_.order_us = -1;
    sc->ordered = true; sc->Q = Q; sc->L = 0; sc->G = 0; sc->levels.clear(); sc->hist.clear();
    sc->run_off.assign(Q + 1, 0); sc->run_cnt.clear(); sc->run_group.clear(); sc->run_level.clear(); sc->run_start.clear(); sc->run_prio.clear();
    if (N > 0xFFFFFFF0ull) return fail(HQTICK_E_CAPACITY, "ordered view: more than 2^32 - 16 slots in the ready set");
    if (!d_ord_hist.ensure(hw * 4) || !h_ordh.ensure(hw * 4)) return fail(HQTICK_E_DEVICE, "hipMalloc ordered view");
    if (e.timing) HQ_HIP(hipEventRecord(e.view_start, st));
    HQ_HIP(hqk::order_digits(prio, rq, N, Q, d_ord_hist.as<uint32_t>(), st));
    HQ_HIP(hipMemcpyAsync(h_ordh.p, d_ord_hist.p, hw * 4, hipMemcpyDeviceToHost, st));
    if (while_gpu_runs) (*while_gpu_runs)();
    HQ_HIP(hipStreamSynchronize(st));
    const uint32_t *gh = h_ordh.as<uint32_t>();
    if (gh[hqk::ORDER_DIGITS * 256]) return fail(HQTICK_E_INVALID, BAD_RQ);
    uint64_t n_live = 0;
    for (uint32_t d = 0; d < 256; d++) n_live += gh[d];
    if (n_live == 0) return 0;
    const uint32_t n = (uint32_t)n_live;
    static_assert(hqk::ORDER_DIGITS <= MAX_DIGITS, "Passes holds every digit");
    const Passes passes = order_passes(gh, hqk::ORDER_DIGITS, n);
    const uint32_t tiles = hqk::order_tiles(N);
    const OrderTabLayout tl = order_tab_layout(n);
    if (!d_perm.ensure((size_t)n * 4 + 16) || !d_perm2.ensure((size_t)n * 4 + 16) || !d_ord_tab.ensure((size_t)tiles * 256 * 4 + 16) ||
        !d_ord_tiles.ensure(((size_t)tiles + 1) * 4 + 16) || !d_inv.ensure(N * 8 + 16) || !h_ord.ensure(tl.bytes))
        return fail(HQTICK_E_DEVICE, "hipMalloc ordered view");
    uint32_t *lrank = d_inv.as<uint32_t>() + N, *inv_ = d_inv.as<uint32_t>();  // [inv N][level rank N]
    uint32_t *perr = d_ord_hist.as<uint32_t>() + hqk::ORDER_DIGITS * 256 + 1;
    const uint32_t *in = nullptr;
    for (uint32_t i = 0; i < passes.n; i++) {
        uint32_t *out = ((passes.n - 1 - i) % 2 == 0) ? d_perm.as<uint32_t>() : d_perm2.as<uint32_t>();  // (the last pass writes d_perm)
        HQ_HIP(hqk::order_pass(prio, rq, i == 0 ? N : n, i == 0, in, passes.digit[i], d_ord_hist.as<uint32_t>(), d_ord_tab.as<uint32_t>(), out, n, perr, st));
        in = out;
        if (i == passes.level_after) HQ_HIP(hqk::order_levels(prio, in, n, d_ord_tiles.as<uint32_t>(), lrank, h_ord.dev<uint32_t>() + 1, st));
    }
    uint8_t *hd = h_ord.dev<uint8_t>();
    HQ_HIP(hqk::order_runs(prio, rq, in, n, d_ord_tiles.as<uint32_t>(), lrank, inv_, h_ord.dev<uint32_t>(), reinterpret_cast<uint32_t *>(hd + tl.o_rq),
                           reinterpret_cast<uint32_t *>(hd + tl.o_st), reinterpret_cast<uint32_t *>(hd + tl.o_rk), reinterpret_cast<uint64_t *>(hd + tl.o_pr), st));
    HQ_HIP(hipMemcpyAsync(h_ordh.as<uint32_t>() + hqk::ORDER_DIGITS * 256 + 1, perr, 4, hipMemcpyDeviceToHost, st));
    if (e.timing) HQ_HIP(hipEventRecord(e.view_stop, st));
    HQ_HIP(hipStreamSynchronize(st));
    if (gh[hqk::ORDER_DIGITS * 256 + 1]) return fail(HQTICK_E_DEVICE, "ordered view: a pass's counts disagree with the digit histogram");
    const char *why = nullptr;
    if (int rc = decode_runs(h_ord.as<uint8_t>(), n, Q, sc, &why)) return fail(rc, why);
    if (e.timing) { const double us_ = elapsed_us(e.view_start, e.view_stop); view_.us = us_ >= 0 ? us_ : 0.0; t_.order_us = view_.us; }
    view_.valid = true; view_.runs = sc->G; view_.levels = sc->L; view_.passes = passes.mask();
    return 0;
}

int Scanner::retracting_positions(hipStream_t st, const hqready::Cols &cols, const Scan &sc, const uint64_t *ids, uint32_t n) {
    if (!h_retr.ensure((size_t)n * 16 + 64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc retracting");
    n_retr = n;
    memcpy(h_retr.p, ids, (size_t)n * 8);
    uint8_t *rd = h_retr.dev<uint8_t>();
    const uint64_t *want = reinterpret_cast<const uint64_t *>(rd); uint32_t *keys = reinterpret_cast<uint32_t *>(rd + (size_t)n * 8), *ranks = reinterpret_cast<uint32_t *>(rd + (size_t)n * 12);
    if (!sc.ordered) HQ_HIP(hqk::rank_of(cols.id, d_gkey.as<uint16_t>(), cols.n, d_wave_tab.as<uint32_t>(), sc.geom, want, n, keys, ranks, st));
    else if (sc.run_cnt.empty()) { uint32_t *k = reinterpret_cast<uint32_t *>(h_retr.as<uint8_t>() + (size_t)n * 8); for (uint32_t i = 0; i < n; i++) k[i] = 0xFFFFFFFFu; }
    else {
        HQ_HIP(hqk::order_rank_of(cols.id, cols.rq, cols.n, d_inv.as<uint32_t>(), want, n, keys, ranks, st));
        HQ_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

// Phase A on the ordered view: K2 as its own launch, the view, the positions of the Retracting tasks.
int Scanner::scan_on_view(const Env &e, const hqready::Cols &cols, const Shape &sh, const Workers &wk, WorkerEval *ev, Scan *sc, const std::function<void()> *while_gpu_runs) {
    const uint32_t Q = sh.Q;
    const size_t nwv = wk.slots, o_tmc = 16, o_fl = o_tmc + nwv * 4, bytes = o_fl + nwv + 16;
    if (!h_a.ensure(bytes)) return fail(HQTICK_E_DEVICE, "hipHostMalloc phase A");
    unsigned char *h = h_a.as<unsigned char>(), *hd = h_a.dev<unsigned char>();
    memset(h, 0, 16);
    hqcluster::UpView uv; int rc;
    if ((rc = wk.tables(wk.user, &uv, &err))) return rc;
    HQ_HIP(hqk::worker_eval(uv.total, uv.free_, uv.rem, wk.W, wk.R, uv.rt, uv.n_entries, hd + o_fl, reinterpret_cast<uint32_t *>(hd + o_tmc), e.stream));
    ev->flags = h + o_fl; ev->tmc = reinterpret_cast<const uint32_t *>(h + o_tmc);
    levels_valid = false;  // (the dense level table is rediscovered when a tick fits the dense caps again)
    if ((rc = view(e, cols, Q, sc, while_gpu_runs))) return rc;
    if (!force_ordered && sc->L <= hqk::MAX_LEVELS && (uint64_t)sc->L * Q <= hqk::MAX_GROUPS) ordered_sticky = false;  // the next tick fits the dense scan again
    if (sh.n_retracting) return retracting_positions(e.stream, cols, *sc, sh.retracting_task, sh.n_retracting);  // where do the Retracting tasks sit in their queues?  (mapping.rs:66-80 treats them apart)
    return 0;
}

// K2 on the workers, level table (cached across ticks, re-validated by K1), K1 + K1b on the columns.  One synchronisation in the steady state.
int Scanner::scan(const Env &e, const hqready::Cols &cols, const Shape &sh, const Workers &wk, WorkerEval *ev, Scan *sc, const std::function<void()> *while_gpu_runs) {
    const uint32_t W = wk.W, R = wk.R, Q = sh.Q;
    const uint64_t N = cols.n;
    t_ = Timings{};
    sc->Q = Q; sc->L = 0; sc->G = 0; sc->levels.clear(); sc->hist.clear();
    runs_from_hist(*sc);  // (no run until the scan has counted)
    if (!ensure_discovery()) return fail(HQTICK_E_DEVICE, "hipMalloc phase A");
    const bool scan = N != 0 && Q != 0;
    const size_t nwv = wk.slots;
    view_.valid = false; dense_.valid = false; census_.valid = false;   // (h_a and h_lv are rewritten from here on)
    // the ordered view where the dense table does not fit: forced (HQTICK_ORDERED_VIEW=1), or the last dense attempt did not fit
    if (scan && (force_ordered || ordered_sticky)) return scan_on_view(e, cols, sh, wk, ev, sc, while_gpu_runs);
    for (int attempt = 0; attempt < 2; attempt++) {
        uint32_t L = 0;
        bool levels_fresh = false;  // the level table was (re)built by this attempt
        bool spec = false;          // ... and the scan was launched behind the discovery without waiting for it (sized for four levels)
        if (scan) {
            if (!levels_valid) {
                const bool time_k0 = e.timing;   // (two marker packets around K0: only when every kernel is timed)
                uint32_t seq = 0;
                if (int rc = discover(e.stream, time_k0 ? e.k0_start : nullptr, time_k0 ? e.k0_stop : nullptr, cols, &seq)) return rc;
                levels_fresh = true;
                const uint32_t *hl = h_lv.as<uint32_t>();
                // SPECULATIVE SCAN: with at most 4 levels x Q <= 64 groups — the variant of K1 the BASELINE ticks run — the scan is launched right behind the
                // discovery, sized for four levels, and reads the table and its length from HBM (kernels.h: level_hist, n_levels_dev): no host round trip, no idle GPU
                // between the two (K1 behind a 15-33 us gap took 6.4-7.2 us against 5.5, profiles/r06).  More than four levels: K1 refuses, the table is read below
                // and this loop's second pass launches the general variant.
                // Not with Retracting tasks: k_rank_of reads the group keys K1 leaves, and a refused speculative K1 leaves none (a fresh scanner's key column is
                // uninitialised: the keys would index the slice table out of bounds).
                spec = attempt == 0 && (uint64_t)4 * Q <= 64 && !no_spec_scan && sh.n_retracting == 0;
                if (!spec) {
                    // wait on the kernel's own completion word (the stream synchronisation is the fallback after 2 s)
                    const double w0 = now_us();
                    for (uint64_t spins = 0;; spins++) {
                        if (__atomic_load_n(&hl[3], __ATOMIC_ACQUIRE) == seq) break;
                        if ((spins & 0xFFFF) == 0xFFFF && now_us() - w0 > 2.0e6) { HQ_HIP(hipStreamSynchronize(e.stream)); if (__atomic_load_n(&hl[3], __ATOMIC_ACQUIRE) != seq) return fail(HQTICK_E_DEVICE, "level discovery did not complete"); break; }
                    }
                    L = hl[0];
                    if (beyond_levels(hl)) { ordered_sticky = true; return scan_on_view(e, cols, sh, wk, ev, sc, while_gpu_runs); }  // more than 4096 levels
                    if (L == 0) return fail(HQTICK_E_DEVICE, "level discovery returned no level");
                    h_levels.assign(h_lv.as<uint64_t>() + 2, h_lv.as<uint64_t>() + 2 + L);
                    set_clean = true;
                    float ms = 0;
                    if (time_k0 && (hipEventElapsedTime(&ms, e.k0_start, e.k0_stop) == hipSuccess || (hipEventSynchronize(e.k0_stop) == hipSuccess && hipEventElapsedTime(&ms, e.k0_start, e.k0_stop) == hipSuccess)))
                        t_.distinct_us = ms * 1000.0;  // (the kernel behind k0_stop has finished: the wait, if the runtime has not noticed yet, is short)
                    levels_valid = true; cached_L = L;
                }   // (speculative: levels_valid stays false until the table has been read, after the scan)
            }
            L = spec ? 4u : cached_L;
            uint64_t G64 = (uint64_t)L * Q;
            if (G64 > hqk::MAX_GROUPS) { ordered_sticky = true; return scan_on_view(e, cols, sh, wk, ev, sc, while_gpu_runs); }  // levels x requests over 16384 groups
            sc->L = L; sc->G = (uint32_t)G64;
        }
        // host-visible outputs of phase A, written in place by the kernels: [flags 16][hist G*4][vtmc nwv*4][vflags nwv]
        size_t o_hist = 16, o_tmc = o_hist + (size_t)sc->G * 4, o_fl = o_tmc + nwv * 4, bytes = o_fl + nwv + 16;
        if (!h_a.ensure(bytes)) return fail(HQTICK_E_DEVICE, "hipHostMalloc phase A");
        unsigned char *h = h_a.as<unsigned char>(), *hd = h_a.dev<unsigned char>();
        memset(h, 0, 16);
        // K2 reads the packed tables from pinned memory; with a ready set to scan it rides along the K1 launch
        bool scan_is_last = false;  // K1b was launched and nothing follows it on the stream
        hqcluster::UpView uv;
        if (int rc = wk.tables(wk.user, &uv, &err)) return rc;
        hqk::WorkerEvalArgs wea{uv.total, uv.free_, uv.rem, W, R, uv.rt, uv.n_entries, hd + o_fl, reinterpret_cast<uint32_t *>(hd + o_tmc)};
        if (scan) {
            const Geom cg = wave_geometry(N, sc->G, e.tpw_hint, hqk::MAX_GROUPS_4W);
            hqk::WaveGeom &g = sc->geom;
            g.tasks_per_wave = cg.tasks_per_wave; g.n_waves = cg.n_waves; g.waves_per_block = cg.waves_per_block; g.tab_stride = cg.tab_stride;
            if (!d_wave_tab.ensure((size_t)g.tab_stride * sc->G * 4) || !d_gkey.ensure(N * 2 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc histogram");
            if (e.timing || e.timing_k1) hqk::time_next_launch(e.k1_start, e.k1_stop);
            if (e.k2_own_stream) HQ_HIP(hqk::worker_eval(uv.total, uv.free_, uv.rem, W, R, uv.rt, uv.n_entries, hd + o_fl, reinterpret_cast<uint32_t *>(hd + o_tmc), e.stream2));
            HQ_HIP_TIMED(hqk::level_hist(cols.prio, cols.rq, N, d_levels.as<uint64_t>(), h_levels.data(), L, Q, g, d_wave_tab.as<uint32_t>(),
                                   d_gkey.as<uint16_t>(), d_flags.as<uint32_t>() + 2, e.k2_on_hist ? &wea : nullptr, e.stream, spec ? d_nlevels.as<uint32_t>() : nullptr));
            hqk::time_next_launch((e.timing && !spec) ? e.k0_start : nullptr, e.k1b_stop);  // k1b_stop: K1b's completion — what the host waits on below
            HQ_HIP_LAST(hqk::scan_waves(d_wave_tab.as<uint32_t>(), g, sc->G, reinterpret_cast<uint32_t *>(hd + o_hist), d_flags.as<uint32_t>() + 2,
                                   reinterpret_cast<uint32_t *>(hd) + 2, e.stream, (e.k2_own_stream || e.k2_on_hist) ? nullptr : &wea), scan_is_last);
            if (sh.n_retracting) {  // where do the Retracting tasks sit in their queues?  (mapping.rs:66-80 treats them apart)
                scan_is_last = false;  // k_rank_of follows
                if (int rc = retracting_positions(e.stream, cols, *sc, sh.retracting_task, sh.n_retracting)) return rc;
            }
        } else {
            HQ_HIP(hqk::worker_eval(uv.total, uv.free_, uv.rem, W, R, uv.rt, uv.n_entries, hd + o_fl, reinterpret_cast<uint32_t *>(hd + o_tmc), e.stream));
        }
        ev->flags = h + o_fl; ev->tmc = reinterpret_cast<const uint32_t *>(h + o_tmc);
        if (while_gpu_runs) (*while_gpu_runs)();
        if (scan && scan_is_last) HQ_HIP(hipEventSynchronize(e.k1b_stop)); else HQ_HIP(hipStreamSynchronize(e.stream));
        if (scan && e.k2_own_stream) HQ_HIP(hipStreamSynchronize(e.stream2));
        const uint32_t *flags = reinterpret_cast<const uint32_t *>(h);
        if (spec) {   // the discovery's own results, now that everything behind it has finished too
            const uint32_t *hl = h_lv.as<uint32_t>();
            const uint32_t La = hl[0];
            if (beyond_levels(hl)) {  // more than 4096 levels:
                // the view.  while_gpu_runs runs again: it has published the ADDRESSES of K2's output in the dense layout of h_a, and scan_on_view lays
                // h_a out anew
                levels_valid = false; ordered_sticky = true; return scan_on_view(e, cols, sh, wk, ev, sc, while_gpu_runs);
            }
            if (La == 0) { levels_valid = false; return fail(HQTICK_E_DEVICE, "level discovery returned no level"); }
            h_levels.assign(h_lv.as<uint64_t>() + 2, h_lv.as<uint64_t>() + 2 + La);
            levels_valid = true; cached_L = La; set_clean = true;
            float ms = 0;
            if (e.timing && hipEventElapsedTime(&ms, e.k0_start, e.k0_stop) == hipSuccess) t_.distinct_us = ms * 1000.0;
            if ((flags[2] & 4u) || La > 4) continue;   // more levels than the speculative launch was sized for: the table is known now, scan again with the right variant
            sc->L = La; sc->G = La * Q;                // (group keys and the rows of the per-slice table do not depend on how many levels the launch was sized for)
        }
        if (scan && (flags[2] & 2u)) return fail(HQTICK_E_INVALID, BAD_RQ);
        if (scan && (flags[2] & 1u)) {  // a priority the cached level table does not know: rebuild the table once
            levels_valid = false;
            if (attempt == 0) continue;
            return fail(HQTICK_E_DEVICE, "level table inconsistent with the ready set");
        }
        if (scan) {
            sc->levels = h_levels;
            sc->hist.assign(reinterpret_cast<const uint32_t *>(h + o_hist), reinterpret_cast<const uint32_t *>(h + o_hist) + sc->G);
            // A level without a single task (its tasks were handed out or cancelled since the table was built — or the table was built from a column that
            // was still being written) only costs: more groups, and beyond 4 levels / 2048 groups the slower kernel variants.  This tick is right either
            // way (empty levels take part in nothing); the next one rediscovers the levels.
            for (uint32_t l = 0; l < sc->L && levels_valid && !levels_fresh; l++) {  // (a table built in this very tick is not questioned: no rediscovery loop)
                uint64_t tot = 0;
                for (uint32_t q = 0; q < Q; q++) tot += sc->hist[(size_t)l * Q + q];
                if (tot == 0) levels_valid = false;
            }
            if (e.timing || e.timing_k1) { const double us_ = elapsed_us(e.k1_start, e.k1_stop); if (us_ >= 0) t_.level_hist_us = us_; }
            if (e.timing && !spec) { const double us_ = elapsed_us(e.k0_start, e.k1b_stop); if (us_ >= 0) t_.scan_us = us_; }  // (a speculative scan shares k0_start with the discovery: K1b untimed on that tick)
            dense_.valid = true; dense_.L = sc->L; dense_.G = sc->G;
            dense_.shape[0] = sc->geom.waves_per_block; dense_.shape[1] = sc->geom.tasks_per_wave; dense_.shape[2] = sc->geom.n_waves; dense_.shape[3] = hqk::lds_levels_for(sc->L) ? 1u : 0u;
        }
        runs_from_hist(*sc);
        return 0;
    }
    return 0;
}

// The census of a resident set (census.hip) in place of the dense scan: level discovery and the count kernel read the columns on `st` — behind every add, remove,
// append and compaction queued there — and write only this scanner's buffers; one synchronisation.
int Scanner::census(hipStream_t st, const hqready::Cols &cols, uint64_t live, uint32_t Q, Scan *sc) {
    sc->Q = Q; sc->L = 0; sc->G = 0; sc->levels.clear(); sc->hist.clear();
    runs_from_hist(*sc);
    census_.valid = false;
    const uint64_t N = cols.n;
    if (N == 0 || Q == 0 || live == 0) return 0;
    const size_t tab_words = 4 + (size_t)std::min<uint64_t>(hqk::MAX_GROUPS, (uint64_t)Q * hqk::MAX_LEVELS);   // [err x 4][counts]: what the census can write for this Q
    if (!ensure_discovery() || !d_hist.ensure((4 + (size_t)hqk::MAX_GROUPS) * 4) || !h_a.ensure(tab_words * 4)) return fail(HQTICK_E_DEVICE, "hipMalloc query census");
    uint32_t seq = 0;
    if (int rc = discover(st, nullptr, nullptr, cols, &seq, d_hist.p, tab_words * 4)) return rc;
    HQ_HIP(hqk::ready_census(cols.prio, cols.rq, N, Q, d_levels.as<uint64_t>(), d_nlevels.as<uint32_t>(), d_hist.as<uint32_t>(), st));
    HQ_HIP(hipMemcpyAsync(h_a.p, d_hist.p, tab_words * 4, hipMemcpyDeviceToHost, st));
    HQ_HIP(hipStreamSynchronize(st));
    const uint32_t *hl = h_lv.as<uint32_t>();
    const uint32_t L = hl[0];
    // beyond the dense caps: the ordered view's run table
    Env untimed{}; untimed.stream = st;  // (no event is recorded for a query)
    if (beyond_levels(hl)) return view(untimed, cols, Q, sc);
    set_clean = true;
    if (L == 0) return 0;   // only tombstones
    if ((uint64_t)L * Q > hqk::MAX_GROUPS) return view(untimed, cols, Q, sc);
    const uint32_t *h = h_a.as<uint32_t>();
    if (h[0] & 2u) return fail(HQTICK_E_INVALID, BAD_RQ);
    if (h[0]) return fail(HQTICK_E_DEVICE, "census: level table inconsistent with the ready set");
    sc->L = L; sc->G = L * Q;
    sc->levels.assign(h_lv.as<uint64_t>() + 2, h_lv.as<uint64_t>() + 2 + L);
    sc->hist.assign(h + 4, h + 4 + sc->G);
    census_.valid = true; census_.L = sc->L; census_.G = sc->G;
    runs_from_hist(*sc);
    return 0;
}

int Scanner::relaunch_level_hist(hipStream_t st, const hqready::Cols &cols, uint32_t L, uint32_t Q, hqk::WaveGeom g) {
    HQ_HIP(hqk::level_hist(cols.prio, cols.rq, cols.n, d_levels.as<uint64_t>(), h_levels.data(), L, Q, g, d_wave_tab.as<uint32_t>(), d_gkey.as<uint16_t>(), d_flags.as<uint32_t>() + 2, nullptr, st));
    return 0;
}
// K1 left raw counts in the slice table: turn them back into offsets
int Scanner::relaunch_scan_waves(hipStream_t st, hqk::WaveGeom g, uint32_t G) {
    HQ_HIP(hqk::scan_waves(d_wave_tab.as<uint32_t>(), g, G, reinterpret_cast<uint32_t *>(h_a.dev<unsigned char>() + 16), d_flags.as<uint32_t>() + 2, reinterpret_cast<uint32_t *>(h_a.dev<unsigned char>()) + 2, st));
    return 0;
}

}  // namespace hqscan
