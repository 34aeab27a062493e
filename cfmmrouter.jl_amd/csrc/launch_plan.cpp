// launch_plan.cpp -- the launch geometry of one evaluation (launch_plan.h): per-segment blocks and grids, the launch
// groups with their XCD maps and fee-table sizes, every offset and total.  Pure: plain inputs in, a LaunchPlan out.
#include "ctx.h"

#include <algorithm>
#include <cstring>

namespace cfmm {

namespace {

// Grid cap for the fat (512/1024-thread) blocks: HALF a machine of resident threads -- one 1024-thread block
// (16 wavefronts) per CU.  Round 1 ran a full machine (two blocks per CU); with consecutive sweeps walking the
// tiles in alternating directions (option "alternate") fewer, longer lanes win: each lane owns 2x the tiles, so
// more of a sweep starts on L2-resident data, and there are half as many partial rows and LDS prologues
// (measured, sweep span us at 256 / 384 / 512 blocks: product1m 9.7 / 10.6 / 10.6, config5 19.1 / 22.6 / 21.7,
// config-4 shard 7.1 / - / 8.1; 128 blocks: 14.9 / 24.5 / 9.2).
// Fused multi-family launches share the cap: 512 blocks of 512 threads in total measured best on config3
// (19.9 us per step vs 21.9 at 1024 blocks and 21.4 at 256; bench.py --opt block=.. --opt max_grid=..).
int fat_grid_cap(int block) { return kResidentThreads / 2 / block; }

int64_t tiles_of(int64_t m, int block) { return std::max<int64_t>(1, (m + block - 1) / block); }

// Launch geometry for a segment of m pools.  Small markets: 512-thread blocks, one tile each.  Large markets:
// 1024-thread blocks, at most one per CU, each striding over many tiles -- this keeps the number of partial rows
// (and the fold kernel) small.  Large-market mode (global bins) uses 512-thread blocks throughout.
void plan_segment(const PlanOpts& o, bool gb, size_t n_segs, const PlanSeg& s, SegPlan& p)
{
    const auto capped = [&](int64_t tiles, int64_t cap) { return (int)std::min<int64_t>(tiles, o.max_grid > 0 ? o.max_grid : cap); };
    const int64_t tiles_mid = tiles_of(s.m, kMidBlock);
    // N-coin segments (weighted, Curve): their own launch of 512-thread blocks (sweep_ncoin), never single-block direct
    if (kind_info(s.kind).ragged) {
        p.block = kMidBlock;
        p.grid = capped(tiles_mid, fat_grid_cap(kMidBlock));
        return;
    }
    // tiny single-family markets: ONE block, whose row is the result (SweepArgs::direct: no fold launch)
    if (o.direct_small != 0 && n_segs == 1 && s.m <= kDirectPools && !gb && o.block == 0 && o.max_grid == 0) {
        p.block = kBigBlock;
        p.grid = 1;
        return;
    }
    if (gb || o.block == kMidBlock || (o.block == 0 && tiles_mid <= 256)) {
        p.block = kMidBlock;
        p.grid = capped(tiles_mid, tiles_mid <= 256 ? 256 : fat_grid_cap(kMidBlock));
    } else {
        p.block = kBigBlock;
        p.grid = capped(tiles_of(s.m, kBigBlock), fat_grid_cap(kBigBlock));
    }
}

int64_t family_cost(const PlanOpts& o, const PlanSeg& s)
{
    const KindInfo& k = kind_info(s.kind);
    return (k.cost_opt ? o.*k.cost_opt : k.cost) + (s.m > 0 && s.n_ticks_total / s.m > 2 ? k.multi_tick_cost : 0);
}

// XCD-aware, cost-weighted map of a fused launch (grid a multiple of 256 blocks): 32-deal pattern in
// which segment s appears seg_w[s] times, spread evenly (largest-remainder weights, Bresenham order).
void plan_xcd_map(const PlanOpts& o, bool gb, const std::vector<PlanSeg>& segs, LaunchPlan& plan, Group& g)
{
    g.xcd_map = false;
    if (!g.multi || g.grid % 256 != 0 || gb) return;
    double cost[kMaxMulti], total = 0.0;
    for (int k = 0; k < g.nseg; ++k) {
        const PlanSeg& s = segs[(size_t)g.first + k];
        cost[k] = (double)s.m * (double)family_cost(o, s);
        total += cost[k];
    }
    if (!(total > 0.0)) return;
    int w[kMaxMulti], sum = 0;
    double frac[kMaxMulti];
    for (int k = 0; k < g.nseg; ++k) {
        const double share = 32.0 * cost[k] / total;
        w[k] = std::max(1, (int)share);
        frac[k] = share - (int)share;
        sum += w[k];
    }
    while (sum < 32) {   // hand the remaining deals to the largest remainders
        int best = 0;
        for (int k = 1; k < g.nseg; ++k) if (frac[k] > frac[best]) best = k;
        ++w[best]; frac[best] = -1.0; ++sum;
    }
    while (sum > 32) {   // (only when several tiny segments were rounded up to one deal each)
        int big = 0;
        for (int k = 1; k < g.nseg; ++k) if (w[k] > w[big]) big = k;
        --w[big]; --sum;
    }
    // Bresenham spread: at every position pick the segment that is furthest behind its share
    int given[kMaxMulti] = {0};
    for (int p = 0; p < 32; ++p) {
        int best = -1;
        double lag_best = -1e30;
        for (int k = 0; k < g.nseg; ++k) {
            if (given[k] >= w[k]) continue;
            const double lag = (double)(p + 1) * w[k] / 32.0 - given[k];
            if (lag > lag_best) { lag_best = lag; best = k; }
        }
        g.pattern[p] = (unsigned char)best;
        g.rank[p] = (unsigned char)given[best];
        ++given[best];
    }
    for (int k = 0; k < g.nseg; ++k) {
        g.seg_w[k] = w[k];
        plan.segs[(size_t)g.first + k].grid = (g.grid / 256) * w[k] * 8;
    }
    g.xcd_map = true;
}

// the launch takes the next g.grid partial rows; its fee table: the packed records of a launch's segments index ONE table
// staged in LDS, which exists when every segment has packed records and the distinct fees of all of them fit
void push_group(const PlanOpts& o, bool gb, const std::vector<PlanSeg>& segs, LaunchPlan& plan, Group g)
{
    g.row_off = plan.segs[(size_t)g.first].row_off = plan.rows;
    plan.rows += g.grid;
    int total = 0;
    bool ok = o.pack != 0 && !gb;
    for (int k = 0; k < g.nseg && ok; ++k) {
        const PlanSeg& s = segs[(size_t)g.first + k];
        if (!s.packed || s.n_fees == 0) ok = false;   // (0: the segment has more fee tiers than a table holds)
        total += s.n_fees;
    }
    g.gtab_n = ok && total <= kMaxFeeTable ? total : 0;
    for (int k = 0, base = 0; k < g.nseg && g.gtab_n != 0; ++k) {
        plan.segs[(size_t)g.first + k].gbase = base;
        base += segs[(size_t)g.first + k].n_fees;
    }
    plan.groups.push_back(g);
}

} // namespace

LaunchPlan plan_launches(const std::vector<PlanSeg>& segs, int n_tokens, const PlanOpts& o)
{
    const bool gb = global_bins(n_tokens);
    LaunchPlan plan;
    plan.segs.resize(segs.size());
    size_t n_fusable = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        const PlanSeg& s = segs[i];
        const KindInfo& k = kind_info(s.kind);
        SegPlan& p = plan.segs[i];
        plan_segment(o, gb, segs.size(), s, p);
        p.trade_off = plan.trades;   // (ragged segments have no rows in the two-coin trade buffers)
        p.flat_off = plan.flat;
        if (!k.ragged) plan.trades += s.m;
        plan.pools += s.m;
        plan.flat += s.m * (k.ragged ? s.n_coins : 2);
        plan.touched_bytes += s.m * k.bytes_per_pool(s.n_coins, s.has_walk);
        plan.any_ragged = plan.any_ragged || k.ragged;
        if (k.fusable) ++n_fusable;
    }
    const bool fuse = o.fuse_segments != 0 && n_fusable >= 2 && o.geomean_exact == 0;
    // fused launches use 512-thread blocks (Product / GeoMean blocks interleave on every CU) unless asked otherwise
    const int fused_block = o.block == kBigBlock && !gb ? kBigBlock : kMidBlock;
    // launch groups: every segment of a kind that is not fusable alone; runs of consecutive fusable segments fused by up to
    // kMaxMulti (sweep_multi) or one launch each
    for (size_t first = 0; first < segs.size();) {
        Group g;
        g.first = (int)first;
        const bool fused = fuse && kind_info(segs[first].kind).fusable;
        size_t run_end = first + 1;
        while (fused && run_end < segs.size() && run_end - first < (size_t)kMaxMulti && kind_info(segs[run_end].kind).fusable)
            ++run_end;
        if (!fused) {
            g.block = plan.segs[first].block;
            g.grid = plan.segs[first].grid;
        } else {
            g.nseg = (int)(run_end - first);
            g.multi = g.nseg >= 2;
            g.block = fused_block;
            int64_t tiles = 1;
            for (size_t i = first; i < run_end; ++i) tiles = std::max(tiles, tiles_of(segs[i].m, g.block));
            const int64_t cap = std::max<int64_t>(1, (o.max_grid > 0 ? o.max_grid : fat_grid_cap(g.block)) / g.nseg);
            const int per_seg = (int)std::min(tiles, cap);
            for (size_t i = first; i < run_end; ++i) {
                plan.segs[i].block = g.block;
                plan.segs[i].grid = per_seg;
            }
            g.grid = per_seg * g.nseg;
            plan_xcd_map(o, gb, segs, plan, g);   // may re-divide the same number of blocks among the segments by cost
        }
        push_group(o, gb, segs, plan, g);
        first = run_end;
    }
    return plan;
}

// Block b of launch g: its segment and the block of that segment it is (the maps sweep_multi used to evaluate on the
// device), then the tiles of that block: first + k·stride < m, all of them full but possibly the last
BlockRec plan_block_rec(const Group& g, int b, const SweepDesc& head, const int* kinds)
{
    int sidx = 0, local = b, nblocks = g.grid;
    if (g.multi && g.xcd_map) {
        const int x = b & 7, j = b >> 3, q = j >> 5, p = (j + q) & 31;
        sidx = g.pattern[p];
        const int w = g.seg_w[sidx];
        local = (q * w + g.rank[p]) * 8 + x;
        nblocks = (g.grid >> 8) * w * 8;
    } else if (g.multi) {
        nblocks = g.grid / g.nseg;
        sidx = b % g.nseg;
        local = b / g.nseg;
    }
    const int64_t m = head.seg[sidx].m;
    BlockRec r;
    r.first = (int64_t)local * g.block;
    r.stride = (int64_t)nblocks * g.block;
    r.full = r.tail = 0;
    if (r.first < m) {
        const int64_t tiles = (m - r.first + r.stride - 1) / r.stride;       // tiles of lane 0
        const int64_t rest = m - (r.first + (tiles - 1) * r.stride);          // pools of the last one, >= 1
        r.full = (int32_t)(rest >= g.block ? tiles : tiles - 1);
        r.tail = (int32_t)(rest >= g.block ? 0 : rest);
    }
    r.row = b;
    r.seg = (int16_t)sidx;
    r.kind = (int16_t)kinds[sidx];
    return r;
}

std::vector<unsigned char> build_sweep_desc(const std::vector<Group>& groups, const std::vector<SweepDesc>& heads,
                                            const std::vector<int>& seg_kinds, std::vector<size_t>& offsets)
{
    offsets.assign(groups.size(), kNoDesc);
    size_t total = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        if (heads[gi].nseg == 0) continue;
        offsets[gi] = total;
        total += sweep_desc_bytes(groups[gi].grid);
    }
    std::vector<unsigned char> bytes(total, 0);
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        if (offsets[gi] == kNoDesc) continue;
        const Group& g = groups[gi];
        SweepDesc head = heads[gi];
        head.nseg = g.nseg;
        head.grid = g.grid;
        std::memcpy(bytes.data() + offsets[gi], &head, sizeof head);
        BlockRec* recs = reinterpret_cast<BlockRec*>(bytes.data() + offsets[gi] + kSweepDescHead);
        for (int b = 0; b < g.grid; ++b) recs[b] = plan_block_rec(g, b, head, seg_kinds.data() + g.first);
    }
    return bytes;
}

bool lean_launch(const SweepDesc& d, const Group& g, const int* kinds, int arith)
{
    if (arith != 1 && arith != 2) return false;                  // (LaunchCfg::arith: fast, auto)
    if (d.nseg < 1 || d.nseg != g.nseg) return false;            // (0: an N-coin launch, which takes no descriptor)
    if (d.compact != 1 || d.nt_stores != 0 || d.v_shift != 4 || d.direct != 0 || d.copies != g.block / 64) return false;
    if (g.block != (g.multi ? kMidBlock : kBigBlock)) return false;
    for (int k = 0; k < d.nseg; ++k) {
        const SegRec& s = d.seg[k];
        if (s.m > kLeanMaxPools) return false;
        switch (kinds[k]) {
        case CFMM_KIND_PRODUCT:
            if (s.pools.p.gbase < 0) return false;
            break;
        case CFMM_KIND_GEOMEAN:
            if (s.pools.g.gbase < 0 || s.pools.g.reference_order != 0 || d.need_logv != 1) return false;
            break;
        case CFMM_KIND_UNIV3:
            if (s.pools.u.gbase < 0 || (!g.multi && !s.pools.u.head)) return false;
            break;
        default: return false;                                   // Solidly and the N-coin kinds
        }
    }
    return true;
}

bool stage_pairs(int n_tokens, int block)
{
    return !global_bins(n_tokens) && sweep_lds_bytes(n_pad_of(n_tokens), 1, block, 1, kMaxFeeTable, 1) <= 160 * 1024;
}

int bin_copies(int n_tokens, const PlanOpts& o, int block)
{
    if (global_bins(n_tokens) || o.bin_copies == 1) return 1;
    const int waves = block / 64;
    // incl. the log-price row and the fee table a launch may stage
    const size_t per_wave = sweep_lds_bytes(n_pad_of(n_tokens), waves, block, 1, kMaxFeeTable, stage_pairs(n_tokens, block) ? 1 : 0);
    if (o.bin_copies == 2) return per_wave <= 160 * 1024 ? waves : 1;
    // auto: one private copy per wavefront while the launch geometry's blocks still fit a CU's 160 KiB of LDS together
    // (1024-thread blocks: one per CU; 512-thread blocks: two)
    return per_wave <= (block == kBigBlock ? 128 : 64) * 1024 ? waves : 1;
}

} // namespace cfmm
