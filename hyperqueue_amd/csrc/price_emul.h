// libhqtick_test.so only (see price_emul.cpp).
#pragma once
#include <algorithm>
#include <vector>

#include "price.h"

namespace hqprice {

struct EmulatedSweeper : Sweeper {
    const HostTables *T = nullptr;
    std::vector<int32_t> caps;
    std::vector<double> bcaps;
    std::vector<uint16_t> pats;
    std::vector<double> blk_cx, blk_rc, blk_bnd;
    std::vector<uint32_t> blk_steps;
    std::vector<long long> slots;
    uint32_t n_sweeps = 0, cap_sweeps = 0;
    // fault injection (hqtick_debug_set_price_fault): begin() refuses the model (fail_at == 0) / the sweep number fail_at - 1 fails (fail_at >= 1); -1: off
    int fail_at = -1;
    // begin() in two halves (price.h), in the order the device walks them: the sweep launched between the halves runs AT the launch, on the block arrays and an
    // all-zero col_woff with K = 0 — the wide rows' tables need not exist yet —, and its totals wait for sweep_finish
    bool blocks_only = false, held_there = false;
    std::vector<uint32_t> zero_woff;
    SweepTotals held;
    bool begin(const HostTables &t, uint32_t max_sweeps) override;
    int begin_blocks(const HostTables &t, uint32_t max_sweeps) override;
    bool begin_wide() override;
    bool sweep_launch(const double *pi) override;
    bool sweep_finish(SweepTotals &out) override;
    bool set_caps(const int32_t *col_cap) override;
    bool set_block_caps(const double *blk_cap) override;
    bool sweep(const double *pi, SweepTotals &out) override;
    bool sweep_range(const double *pi, uint32_t b0, uint32_t b1, RangeValues &out) override;
    const uint16_t *patterns(uint32_t first, uint32_t count) override;
    void end() override;
};

}  // namespace hqprice
