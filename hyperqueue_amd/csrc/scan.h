// The host side of GPU phase A: the scan of the ready set that every tick, every query and three debug hooks start with.  A Scanner owns the
// buffers of the three forms of that scan and what is cached between two of them:
//   scan()    the dense scan: level discovery K0 / K0b (the level table is kept across ticks and re-validated by K1), K1 + K1b per (level, request) group — launched
//             speculatively behind a fresh discovery where at most four levels can fit — with K2 (worker evaluation) riding in K1's or K1b's launch
//   view()    the ordered view (order.hip) where the dense table does not fit: a permutation of the live slots, its inverse and the run table
//   census()  the count of the resident set for a query (census.hip), falling through to view() beyond the dense caps
// The kernels are kernels.hip's, order.hip's and census.hip's.  Like hqready::ReadySet, a method returns an HQTICK_E_* code (negative) with `err` set and enqueues
// on the stream it is given.  The scanner knows the ready set only as columns and the workers only as a number of (worker, variant) slots and a callable that
// yields K2's tables; what it decides from device output without a GPU in sight is scan_core.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/hqtick.h"
#include "cluster.h"
#include "devbuf.h"
#include "kernels.h"
#include "ready.h"
#include "scan_core.h"

namespace hqscan {

struct Scan : Table { hqk::WaveGeom geom{}; };  // result of GPU phase A

// What the scanner uses of its context.  The event pairs are recorded only where `timing` (every measured kernel) or `timing_k1` (K1 alone) asks for them; k1b_stop
// is carried by K1b's dispatch in any case — it is what the host waits on.  k0_start also opens K1b's pair on a tick whose level table was cached.
struct Env {
    hipStream_t stream, stream2;
    hipEvent_t k0_start, k0_stop, k1_start, k1_stop, k1b_stop, view_start, view_stop;
    bool timing, timing_k1, wait_on_kernel;
    bool k2_on_hist, k2_own_stream;  // where K2 runs: along K1's launch / as a launch of its own on stream2 (default: along K1b's)
    uint32_t tpw_hint;               // tasks per wavefront slice (0: chosen by wave_geometry)
};
struct Shape { uint32_t Q, n_retracting; const uint64_t *retracting_task; };  // of the snapshot: requests, and the Retracting tasks whose queue positions the tick needs
// The worker side of K2: `tables` is invoked once per attempt, right before the launch that carries K2, and enqueues whatever brings the tables up to date.
struct Workers { uint32_t W, R; size_t slots; int (*tables)(void *user, hqcluster::UpView *uv, std::string *err); void *user; };  // slots: (worker, variant) pairs
struct Timings { double distinct_us = -1, level_hist_us = -1, scan_us = -1, order_us = -1; };  // of the last scan() / view(); < 0: not measured

class Scanner {
  public:
    std::string err;
    int init();  // HQTICK_ORDERED_VIEW, HQTICK_NO_SPEC_SCAN; the flag words K1 reports into
    void release();
    // ---- the three scans
    // `while_gpu_runs` (may be null) is host work that needs only the ADDRESSES of K2's output, run between the launches and the synchronisation — again if the
    // speculative scan falls back to the view, which lays K2's output out anew.
    int scan(const Env &e, const hqready::Cols &cols, const Shape &sh, const Workers &wk, WorkerEval *ev, Scan *sc, const std::function<void()> *while_gpu_runs = nullptr);
    int view(const Env &e, const hqready::Cols &cols, uint32_t Q, Scan *sc, const std::function<void()> *while_gpu_runs = nullptr);
    int census(hipStream_t st, const hqready::Cols &cols, uint64_t live, uint32_t Q, Scan *sc);
    // (request | group key, position) of n task ids in the queues of `sc`, into pinned memory: dense -> k_rank_of on the group keys K1 left (not waited for: scan()
    // launches it in front of its own wait), view -> k_order_rank_of (waited for), a view of nothing -> 0xFFFFFFFF without a launch
    int retracting_positions(hipStream_t st, const hqready::Cols &cols, const Scan &sc, const uint64_t *ids, uint32_t n);
    const uint32_t *retracting_keys() const { return reinterpret_cast<const uint32_t *>(h_retr.as<uint8_t>() + (size_t)n_retr * 8); }
    const uint32_t *retracting_ranks() const { return reinterpret_cast<const uint32_t *>(h_retr.as<uint8_t>() + (size_t)n_retr * 12); }
    // the columns changed under the cached level table (an upload, a tick's own columns, rewritten priorities, flushed tick caches): the next scan rediscovers it
    void columns_changed() { levels_valid = false; }
    const Timings &timings() const { return t_; }
    // ---- what the selection, the replay of a selection, the ledger and the hooks read of the last scan
    uint16_t *group_keys() const { return d_gkey.as<uint16_t>(); }  // per slot, as K1 left them
    uint32_t *slice_table() const { return d_wave_tab.as<uint32_t>(); }  // [G][tab_stride] offsets, as K1b left them
    uint32_t *perm() const { return d_perm.as<uint32_t>(); }
    uint32_t *inv() const { return d_inv.as<uint32_t>(); }
    uint32_t *level_ranks(uint64_t N) const { return d_inv.as<uint32_t>() + N; }
    uint32_t *select_err_dev() const { return d_ord_hist.as<uint32_t>() + hqk::ORDER_DIGITS * 256 + 2; }  // k_order_select's guard word, behind the digit histogram
    uint32_t *select_err_host() const { return h_ordh.as<uint32_t>() + hqk::ORDER_DIGITS * 256 + 2; }  // ... and where the tick copies it
    const uint64_t *levels_dev() const { return d_levels.as<uint64_t>(); }
    const uint8_t *run_table() const { return h_ord.as<uint8_t>(); }  // of the last view of n live slots: order_tab_layout(n)
    struct Dense { bool valid = false; uint32_t L = 0, G = 0, shape[4] = {0, 0, 0, 0}; const uint64_t *levels = nullptr; const uint32_t *hist = nullptr; };
    Dense last_dense() const { Dense d = dense_; d.levels = h_levels.data(); d.hist = counts(); return d; }
    Dense last_census() const { Dense d = census_; d.levels = h_lv.as<uint64_t>() + 2; d.hist = counts(); return d; }
    struct View { bool valid = false; uint32_t runs = 0, levels = 0, passes = 0; double us = 0; };  // passes: bit dg = a pass ran on digit dg
    const View &last_view() const { return view_; }
    // ---- K1 / K1b once more on the last dense scan's tables (hqtick_time_kernel)
    int relaunch_level_hist(hipStream_t st, const hqready::Cols &cols, uint32_t L, uint32_t Q, hqk::WaveGeom g);
    int relaunch_scan_waves(hipStream_t st, hqk::WaveGeom g, uint32_t G);

  private:
    int fail(int code, const std::string &m) { err = m; return code; }
    const uint32_t *counts() const { return reinterpret_cast<const uint32_t *>(h_a.as<unsigned char>() + 16); }  // both forms keep 16 bytes in front of the counts: phase A its flag words, the census its four error words
    bool ensure_discovery();
    int discover(hipStream_t st, hipEvent_t start, hipEvent_t stop, const hqready::Cols &cols, uint32_t *seq, void *zero = nullptr, size_t zero_bytes = 0);
    int scan_on_view(const Env &e, const hqready::Cols &cols, const Shape &sh, const Workers &wk, WorkerEval *ev, Scan *sc, const std::function<void()> *while_gpu_runs);

    hqbuf::DevBuf d_set, d_flags, d_levels, d_nlevels, d_wave_tab, d_hist, d_gkey;
    hqbuf::DevBuf d_ord_hist, d_ord_tab, d_perm, d_perm2, d_ord_tiles, d_inv; hqbuf::PinBuf h_ord, h_ordh;  // the ordered view
    hqbuf::PinBuf h_a;     // phase A's host-visible output, written in place by the kernels: [flags 16][hist G*4][vtmc slots*4][vflags slots] (the view: no hist; the census: [err 16][counts])
    hqbuf::PinBuf h_lv;    // the level table as k_sort_levels writes it
    hqbuf::PinBuf h_retr; uint32_t n_retr = 0;  // [ids n u64][keys n u32][ranks n u32]
    bool force_ordered = false;   // HQTICK_ORDERED_VIEW=1 (tests): every scan of a ready set takes the view
    bool no_spec_scan = false;    // HQTICK_NO_SPEC_SCAN: no speculative launch
    bool ordered_sticky = false;  // the last dense attempt did not fit: go straight to the view until a view fits the dense caps again
    uint32_t lv_seq = 0; bool set_clean = false;  // set_clean: the priority set and the flag words are as a successful discovery leaves them (empty / zero)
    bool levels_valid = false; uint32_t cached_L = 0; std::vector<uint64_t> h_levels;  // level table of the previous tick (re-validated by K1 every tick)
    Timings t_;
    Dense dense_, census_; View view_;
};

}  // namespace hqscan
