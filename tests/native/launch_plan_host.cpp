// Host shim around csrc/launch_plan.cpp's plan_launches (tests/test_launch_plan_cpu.py builds it together with that file:
// the planner makes no HIP call and needs no device).  Flat int64 arrays in and out, loaded with ctypes.
#include "../../cfmmrouter.jl_amd/csrc/launch_plan.h"

using namespace cfmm;

// opts:   {max_grid, block, bin_copies, direct_small, fuse_segments, geomean_exact, cost_geomean, cost_univ3, pack}
// segs:   per segment {kind, m, n_coins, n_ticks_total, has_walk, packed, n_fees}
// seg_out:   per segment {block, grid, row_off, trade_off, flat_off, gbase}
// group_out: per group {first, nseg, multi, block, grid, row_off, gtab_n, xcd_map, pattern[32], rank[32], seg_w[kMaxMulti]}
// totals:    {rows, pools, trades, flat, touched_bytes, any_ragged}
// returns the number of groups (at most n_seg)
extern "C" int launch_plan_host(int n, const int64_t* opts, int n_seg, const int64_t* segs, int64_t* seg_out, int64_t* group_out,
                                int64_t* totals)
{
    PlanOpts o;
    o.max_grid = opts[0]; o.block = opts[1]; o.bin_copies = opts[2]; o.direct_small = opts[3]; o.fuse_segments = opts[4];
    o.geomean_exact = opts[5]; o.cost_geomean = opts[6]; o.cost_univ3 = opts[7]; o.pack = opts[8];
    std::vector<PlanSeg> in((size_t)n_seg);
    for (int i = 0; i < n_seg; ++i) {
        const int64_t* s = segs + 7 * i;
        in[(size_t)i] = PlanSeg{(int)s[0], s[1], (int)s[2], s[3], (int)s[4], s[5] != 0, (int)s[6]};
    }
    const LaunchPlan plan = plan_launches(in, n, o);
    for (int i = 0; i < n_seg; ++i) {
        const SegPlan& p = plan.segs[(size_t)i];
        const int64_t row[6] = {p.block, p.grid, p.row_off, p.trade_off, p.flat_off, p.gbase};
        for (int k = 0; k < 6; ++k) seg_out[6 * i + k] = row[k];
    }
    constexpr int kGroupWords = 8 + 32 + 32 + kMaxMulti;
    for (size_t i = 0; i < plan.groups.size(); ++i) {
        const Group& g = plan.groups[i];
        int64_t* out = group_out + kGroupWords * i;
        const int64_t head[8] = {g.first, g.nseg, g.multi, g.block, g.grid, g.row_off, g.gtab_n, g.xcd_map};
        for (int k = 0; k < 8; ++k) out[k] = head[k];
        for (int k = 0; k < 32; ++k) out[8 + k] = g.pattern[k];
        for (int k = 0; k < 32; ++k) out[40 + k] = g.rank[k];
        for (int k = 0; k < kMaxMulti; ++k) out[72 + k] = g.seg_w[k];
    }
    const int64_t t[6] = {plan.rows, plan.pools, plan.trades, plan.flat, plan.touched_bytes, plan.any_ragged};
    for (int k = 0; k < 6; ++k) totals[k] = t[k];
    return (int)plan.groups.size();
}

// launch_plan.cpp's bin_copies (how many LDS bin copies a block of `block` threads keeps for n tokens under option
// bin_copies = 0 / 1 / 2): tests/test_reduction_exact_cpu.py holds its NumPy restatement against this
extern "C" int launch_plan_bin_copies(int n, int option, int block)
{
    PlanOpts o;
    o.bin_copies = option;
    return bin_copies(n, o, block);
}
