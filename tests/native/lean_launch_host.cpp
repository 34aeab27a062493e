// Host shim around csrc/launch_plan.cpp's lean_launch (tests/test_lean_launch_cpu.py builds it together with that file: the
// predicate makes no HIP call and needs no device).  A market goes through plan_launches, every group gets the descriptor head
// abi_sweep.cpp's desc_head / ensure_desc would give it -- restated here from the same pure helpers (stage_pairs, bin_copies,
// sweep_lds_bytes) and the launch options -- and lean_launch answers per group.
#include "../../cfmmrouter.jl_amd/csrc/ctx.h"
#include "../../cfmmrouter.jl_amd/csrc/launch_plan.h"

#include <cstring>

using namespace cfmm;

// opts:   {max_grid, block, bin_copies, direct_small, fuse_segments, geomean_exact, cost_geomean, cost_univ3, pack}
// segs:   per segment {kind, m, n_coins, n_ticks_total, has_walk, packed, n_fees}
// launch: {compact_trades, stream_stores (1 = write-through, 2 = non-temporal), univ3_heads, arith (LaunchCfg::arith)}
// lean_out: per group 1 / 0
// returns the number of groups (at most n_seg)
extern "C" int lean_launch_host(int n, const int64_t* opts, int n_seg, const int64_t* segs, const int64_t* launch, int64_t* lean_out)
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
    const bool gb = global_bins(n);
    static const int dummy = 0;   // stands for a device array: the predicate only asks whether the heads are there
    for (size_t gi = 0; gi < plan.groups.size(); ++gi) {
        const Group& g = plan.groups[gi];
        SweepDesc d;
        std::memset(&d, 0, sizeof d);
        d.n = n;
        d.n_pad = n_pad_of(n);
        d.v_shift = stage_pairs(n, g.block) ? 4 : 3;
        d.gtab_n = g.gtab_n;
        int kinds[kMaxMulti] = {0};
        const bool ragged = kind_info(in[(size_t)g.first].kind).ragged;
        d.nseg = ragged ? 0 : g.nseg;
        for (int k = 0; k < d.nseg && !gb; ++k)
            if (kind_info(in[(size_t)g.first + k].kind).logv && o.geomean_exact == 0) d.need_logv = 1;
        if (d.need_logv && sweep_lds_bytes(d.n_pad, 1, g.block, 1, d.gtab_n, d.v_shift == 4 ? 1 : 0) > 160 * 1024) d.need_logv = 0;
        d.copies = bin_copies(n, o, g.block);
        d.compact = launch[0] != 0 && !gb ? 1 : 0;
        d.nt_stores = launch[1] == 2 || (launch[1] == 0 && plan.touched_bytes > (int64_t)256 << 20) ? 1 : 0;
        d.direct = plan.groups.size() == 1 && g.grid == 1 && !g.multi && !gb && !ragged ? 1 : 0;
        for (int k = 0; k < d.nseg; ++k) {
            const PlanSeg& s = in[(size_t)g.first + k];
            const int gbase = d.gtab_n ? plan.segs[(size_t)g.first + k].gbase : -1;
            kinds[k] = s.kind;
            d.seg[k].m = s.m;
            if (s.kind == CFMM_KIND_GEOMEAN) {
                d.seg[k].pools.g.gbase = gbase;
                d.seg[k].pools.g.reference_order = (int)o.geomean_exact;
            } else if (s.kind == CFMM_KIND_UNIV3) {
                d.seg[k].pools.u.gbase = gbase;
                d.seg[k].pools.u.has_walk = s.has_walk;
                d.seg[k].pools.u.head = launch[2] != 0 && s.has_walk ? reinterpret_cast<const uint4*>(&dummy) : nullptr;
            } else {
                d.seg[k].pools.p.gbase = gbase;
            }
        }
        lean_out[gi] = lean_launch(d, g, kinds, (int)launch[3]) ? 1 : 0;
    }
    return (int)plan.groups.size();
}
