// Host shim around csrc/launch_plan.cpp's build_sweep_desc (tests/test_sweep_desc_cpu.py builds it together with that file: the
// builder makes no HIP call and needs no device).  It plans the launches of the given segments, builds the descriptors with
// null device pointers and hands back what the BYTES hold, parsed at the offsets the kernels use.
#include "../../cfmmrouter.jl_amd/csrc/ctx.h"

#include <cstring>

using namespace cfmm;

// opts, segs: as launch_plan_host (tests/native/launch_plan_host.cpp)
// group_out: per group {first, nseg, multi, block, grid, row_off, gtab_n, xcd_map, pattern[32], rank[32], seg_w[kMaxMulti],
//                       descriptor offset (-1: none), head.nseg, head.grid, head.seg[0..3].m}
// rec_out:   per block record, in descriptor order, {group, block, seg, kind, first, stride, full, tail, row}
// returns the number of block records written (at most rec_cap; -1: more), *n_groups and *desc_bytes are set
extern "C" int64_t sweep_desc_host(int n, const int64_t* opts, int n_seg, const int64_t* segs, int64_t* group_out, int64_t* n_groups,
                                   int64_t* rec_out, int64_t rec_cap, int64_t* desc_bytes)
{
    PlanOpts o;
    o.max_grid = opts[0]; o.block = opts[1]; o.bin_copies = opts[2]; o.direct_small = opts[3]; o.fuse_segments = opts[4];
    o.geomean_exact = opts[5]; o.cost_geomean = opts[6]; o.cost_univ3 = opts[7]; o.pack = opts[8];
    std::vector<PlanSeg> in((size_t)n_seg);
    std::vector<int> kinds((size_t)n_seg);
    for (int i = 0; i < n_seg; ++i) {
        const int64_t* s = segs + 7 * i;
        in[(size_t)i] = PlanSeg{(int)s[0], s[1], (int)s[2], s[3], (int)s[4], s[5] != 0, (int)s[6]};
        kinds[(size_t)i] = (int)s[0];
    }
    const LaunchPlan plan = plan_launches(in, n, o);
    std::vector<SweepDesc> heads(plan.groups.size());
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const Group& g = plan.groups[gi];
        SweepDesc& d = heads[gi];
        std::memset(&d, 0, sizeof d);
        d.nseg = ragged_kind(kinds[(size_t)g.first]) ? 0 : g.nseg;
        for (int k = 0; k < d.nseg; ++k) d.seg[k].m = in[(size_t)g.first + k].m;
    }
    std::vector<size_t> off;
    const std::vector<unsigned char> bytes = build_sweep_desc(plan.groups, heads, kinds, off);
    *desc_bytes = (int64_t)bytes.size();
    *n_groups = (int64_t)plan.groups.size();
    constexpr int kGroupWords = 8 + 32 + 32 + kMaxMulti + 3 + kMaxMulti;
    int64_t n_rec = 0;
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const Group& g = plan.groups[gi];
        int64_t* out = group_out + kGroupWords * gi;
        const int64_t head[8] = {g.first, g.nseg, g.multi, g.block, g.grid, g.row_off, g.gtab_n, g.xcd_map};
        for (int k = 0; k < 8; ++k) out[k] = head[k];
        for (int k = 0; k < 32; ++k) out[8 + k] = g.pattern[k];
        for (int k = 0; k < 32; ++k) out[40 + k] = g.rank[k];
        for (int k = 0; k < kMaxMulti; ++k) out[72 + k] = g.seg_w[k];
        out[76] = off[gi] == kNoDesc ? -1 : (int64_t)off[gi];
        out[77] = out[78] = -1;
        for (int k = 0; k < kMaxMulti; ++k) out[79 + k] = -1;
        if (off[gi] == kNoDesc) continue;
        if (off[gi] % 128 != 0 || off[gi] + sweep_desc_bytes(g.grid) > bytes.size()) return -2;
        SweepDesc d;
        std::memcpy(&d, bytes.data() + off[gi], sizeof d);
        out[77] = d.nseg;
        out[78] = d.grid;
        for (int k = 0; k < kMaxMulti; ++k) out[79 + k] = d.seg[k].m;
        for (int b = 0; b < g.grid; ++b) {
            BlockRec r;
            std::memcpy(&r, bytes.data() + off[gi] + kSweepDescHead + (size_t)b * sizeof r, sizeof r);
            if (n_rec >= rec_cap) return -1;
            const int64_t row[9] = {(int64_t)gi, b, r.seg, r.kind, r.first, r.stride, r.full, r.tail, r.row};
            for (int k = 0; k < 9; ++k) rec_out[9 * n_rec + k] = row[k];
            ++n_rec;
        }
    }
    return n_rec;
}
