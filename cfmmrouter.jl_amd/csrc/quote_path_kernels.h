// quote_path_kernels.h -- cfmm_quote_path / cfmm_quote_path_out: an amount carried through a path of pools, ONE LANE PER
// PATH, grid-stride over the paths.  Per hop the lane reads its 20 bytes of hop (segment, row, two coins; hop-major arrays,
// so a wavefront reads each as one stream), the PathSeg of that segment from the table in device memory (sweep.h), and
// evaluates the hop with the body of the single-pool kernels -- quote_one<KIND> / quote_out_one<KIND> of quote_kernels.h,
// picked by with_kind (kind_switch.h) on the segment's kind -- so a path's amounts carry the bits of chaining cfmm_quote / cfmm_quote_out hop
// by hop.  Every hop is quoted against the pool AS IT STANDS: no state advances between hops, a pool visited twice is quoted
// twice from the same reserves.  No LDS, no atomics, no state; lanes whose hops land in different kinds serialise.
// Nothing is trusted (cfmm_quote_path_dev takes unchecked device arrays): an n_hops outside 1 .. max_hops makes the whole
// path NaN with no hop evaluated; a hop whose segment, row or coins are out of range, or whose amount is negative or not
// finite, is clamped BEFORE any read and poisoned after (query_read.h read_hop), and the NaN then travels through the
// remaining hops by that same rule.  The kernels never read out of bounds.
#pragma once

#include "../../include/cfmm_amd.h"
#include "kind_switch.h"
#include "quote_kernels.h"

namespace cfmm {

static_assert(sizeof(PathSeg) == 128, "one 128-byte line per segment of the table");

// The views quote_one<KIND> / quote_out_one<KIND> take, filled from a PathSeg: only the members that KIND's body reads are
// set (and therefore loaded from the table); the bodies themselves are quote_kernels.h's, unchanged.
template <int KIND, bool OUT>
__device__ __forceinline__ double path_hop(const PathSeg& s, int64_t m, int64_t row, int ci, int co, double amt)
{
    QuoteArgs q{};
    UniV3Pools u{};
    NCoinPools n{};
    q.m = m;
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        q.R = s.R;
        q.gamma = s.gamma;
        if constexpr (KIND == CFMM_KIND_GEOMEAN) q.w = s.w;
    } else if constexpr (KIND == CFMM_KIND_UNIV3) {
        u.pg = s.pg;
        u.cur_a = s.cur_a;
        u.cur_b = s.cur_b;
        u.cur_c = s.cur_c;
        u.curR = s.curR;
        u.walk = s.walk;
        u.ticks = s.ticks;
    } else {
        n.R = s.nR;
        n.q = s.nq;
        n.glg = s.nglg;
        n.par = s.npar;
        n.n_coins = s.n_coins;
    }
    if constexpr (OUT) return quote_out_one<KIND>(q, u, n, row, ci, co, amt);
    else return quote_one<KIND>(q, u, n, row, ci, co, amt);
}

// One hop: hop `at` (= k*count + p) of the arrays, the amount `amt` entering it (exact input) or wanted from it (exact
// output).  Read by the rule of query_read.h, evaluated by the kind's body, poisoned.
template <bool OUT>
__device__ __forceinline__ double path_step(const PathArgs& a, int64_t at, double amt)
{
    const auto h = read_hop(a, at, amt);
    const PathSeg& s = h.seg;
    bool ok = h.ok;
    double r;
    with_kind(h.kind, [&](auto K) { r = path_hop<decltype(K)::value, OUT>(s, h.m, h.row, h.ci, h.co, h.amt); }, [&] { r = 0.0; ok = false; });
    return ok ? r : __builtin_nan("");
}

// exact input: x_0 = amount_in, x_{k+1} = quote(hop k, x_k); hops[k] = the amount LEAVING hop k.
// (The block size is a template argument, as it is of the sweep kernels: templates are emitted behind every kernel the
// translation unit had before, which therefore keep their function numbers, labels and bytes.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void quote_path_kernel(PathArgs a)
{
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.count; p += step) {
        int nh = a.n_hops[p];
        double x = a.given[p];
        if (nh < 1 || nh > a.max_hops) {
            nh = 0;
            x = __builtin_nan("");
        }
        for (int k = 0; k < nh; ++k) {
            const int64_t at = (int64_t)k * a.count + p;
            x = path_step<false>(a, at, x);
            if (a.hops) a.hops[at] = x;
        }
        if (a.hops)
            for (int k = nh; k < a.max_hops; ++k) a.hops[(int64_t)k * a.count + p] = __builtin_nan("");
        a.answer[p] = x;
    }
}

// exact output: y_H = amount_out, y_k = quote_out(hop k, y_{k+1}), from the last hop to the first; hops[k] = the amount TO
// TENDER to hop k.  Once a hop answers +inf (that pool cannot give that much) or NaN, every earlier hop and the answer are
// that value and no further form is evaluated.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void quote_path_out_kernel(PathArgs a)
{
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.count; p += step) {
        int nh = a.n_hops[p];
        double y = a.given[p];
        if (nh < 1 || nh > a.max_hops) {
            nh = 0;
            y = __builtin_nan("");
        }
        if (a.hops)
            for (int k = nh; k < a.max_hops; ++k) a.hops[(int64_t)k * a.count + p] = __builtin_nan("");
        for (int k = nh - 1; k >= 0; --k) {
            const int64_t at = (int64_t)k * a.count + p;
            if (y < __builtin_inf()) y = path_step<true>(a, at, y);   // (+inf and NaN pass through unevaluated)
            if (a.hops) a.hops[at] = y;
        }
        a.answer[p] = y;
    }
}

} // namespace cfmm
