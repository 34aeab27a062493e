// launch_plan.h -- internal: the launch geometry of one evaluation as a pure function of the segments' shapes and the
// options.  No HIP call, no cfmm_ctx: every block, grid, row offset and launch group is decided here and pinned on the CPU
// (tests/test_launch_plan_cpu.py); abi_sweep.cpp's ensure_geometry applies the plan, uploads the fee tables and grows the
// buffers.
#pragma once

#include "sweep.h"

#include <cstdint>
#include <vector>

namespace cfmm {

// A launch: either one segment (sweep_kernel / sweep_ncoin) or up to kMaxMulti segments fused (sweep_multi).
struct Group {
    int first = 0, nseg = 1;
    bool multi = false;
    int block = kMidBlock;
    int grid = 0;       // total blocks of the launch
    int64_t row_off = 0;
    int gtab_n = 0;     // entries of this launch's fee table (0: its segments use the plain gamma / Ai arrays)
    // XCD-aware weighted block -> segment map of a fused launch (see sweep_multi); xcd_map == false: block b -> segment b % nseg
    bool xcd_map = false;
    unsigned char pattern[32] = {0}, rank[32] = {0};
    int seg_w[kMaxMulti] = {0};
};

// The options (cfmm_set_option) the geometry depends on
struct PlanOpts {
    int64_t max_grid = 0;        // 0 = auto
    int64_t block = 0;           // 0 = auto, else kMidBlock or kBigBlock
    int64_t bin_copies = 0;      // 0 = auto, 1 = one shared copy, 2 = one copy per wavefront
    int64_t direct_small = 1;    // 1: single-family markets of up to kDirectPools pools are swept by ONE block that publishes {Ψ, acc}
                                 //    itself (no fold launch); 0: the general two-launch geometry
    int64_t fuse_segments = 1;   // 1: sweep all pool families in one launch (sweep_multi)
    int64_t geomean_exact = 0;   // 1: pow-based reference-order forms instead of log-space
    int64_t cost_geomean = 10;   // cost of a GeometricMean / UniV3 evaluation in tenths of a ProductTwoCoin one (10 = blocks in
    int64_t cost_univ3 = 10;     // proportion to pool counts)
    int64_t pack = 1;            // 1: sweeps read the packed fee + token record when the launch's distinct fees fit the LDS table
};
inline bool global_bins(int n_tokens) { return n_tokens > kMaxLdsTokens; }   // large-market mode
inline int n_pad_of(int n_tokens) { return (n_tokens + 1) & ~1; }           // n rounded up to even (LDS row pitch)

// What the plan needs to know of a segment
struct PlanSeg {
    int kind = 0;
    int64_t m = 0;
    int n_coins = 2;
    int64_t n_ticks_total = 0;
    int has_walk = 1;      // UniV3: some pool has a tick beyond its current one
    bool packed = false;   // the segment has packed {tokens, fee index} records
    int n_fees = 0;        // its distinct fees (0: more than a fee table holds)
};

// What the plan decides for a segment
struct SegPlan {
    int block = kMidBlock;
    int grid = 0;
    int64_t row_off = 0;     // first partial row (of the segment's launch)
    int64_t trade_off = 0;   // first row of this segment in the (two-coin) trade buffers
    int64_t flat_off = 0;    // first double of this segment in the ragged trade layout of cfmm_get_trades (Σ coins before it)
    int gbase = 0;           // first entry of this segment in its launch's fee table
};

struct LaunchPlan {
    std::vector<SegPlan> segs;
    std::vector<Group> groups;
    int64_t rows = 0, pools = 0, trades = 0, flat = 0;   // partial rows, pools, two-coin trade rows, Σ m × coins
    int64_t touched_bytes = 0;   // what one materialising sweep moves by construction (packed layout)
    bool any_ragged = false;
};

LaunchPlan plan_launches(const std::vector<PlanSeg>& segs, int n_tokens, const PlanOpts& o);

// The launch-invariant descriptors of an evaluation's sweep_kernel / sweep_multi launches (sweep.h SweepDesc) as ONE byte
// block, ready to be copied to the device: per launch group the head -- heads[gi], filled by the caller: the launch's
// LDS geometry and buffers, and per segment its size and device pointers -- followed by the group's block table, which is
// computed here from the group's map and heads[gi].seg[k].m.  offsets[gi] is where group gi's descriptor starts (a multiple
// of 128 bytes), or kNoDesc for a group that takes none (heads[gi].nseg == 0: the N-coin launches keep plain arguments).
// The block records restate, block by block, what the kernels computed from blockIdx / gridDim before the table existed:
// a segment's own launch gives block b the tiles b, b + grid, ...; a fused launch maps b to {segment, block of the
// segment} through Group::pattern / rank / seg_w (xcd_map) or b % nseg, b / nseg.  kinds[gi][k]: the CFMM_KIND_* of the
// segments.  Pure, like plan_launches; pinned on the CPU by tests/test_sweep_desc_cpu.py.
constexpr size_t kNoDesc = ~(size_t)0;
std::vector<unsigned char> build_sweep_desc(const std::vector<Group>& groups, const std::vector<SweepDesc>& heads,
                                            const std::vector<int>& seg_kinds, std::vector<size_t>& offsets);
BlockRec plan_block_rec(const Group& g, int b, const SweepDesc& head, const int* kinds);

// Does a launch take the LEAN form of its kernel (sweep_core.h sweep_body<..., LEAN>)?  Pure: the head of the launch's
// descriptor with its segments filled in, the group, the segments' kinds and the arithmetic the launch runs on (LaunchCfg::arith).
// Lean iff the launch is what every default launch is -- compact trade records, write-through trade stores, prices staged as
// pairs (which excludes large-market mode), one bin copy per wavefront, not direct, the log-price row there when a segment reads
// it -- and every segment has its fees in the launch's table (gbase >= 0), at most kLeanMaxPools pools (32-bit byte offsets
// into every pool stream) and a kind with a lean kernel at this block size: a fused launch of 512-thread blocks, or
// ProductTwoCoin, log-space GeometricMean or UniV3 with threshold heads alone at 1024; on the fast or the auto arithmetic.
// True means the kernel table HAS the kernel.
constexpr int64_t kLeanMaxPools = (int64_t)1 << 26;   // x 32 bytes per pool (UniV3's threshold heads) = 2 GiB
bool lean_launch(const SweepDesc& head, const Group& g, const int* kinds, int arith);

// Prices are staged in LDS as {v, rcp_refined(v)} pairs unless the market is too wide for them (sweep.h SweepArgs::v_shift)
bool stage_pairs(int n_tokens, int block);
// private bin copies per block (SweepArgs::copies)
int bin_copies(int n_tokens, const PlanOpts& o, int block);

} // namespace cfmm
