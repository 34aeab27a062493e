// to_rate_kernels.h -- cfmm_quote_to_rate / cfmm_quote_to_rate_dev: the amount that brings a pool's marginal rate down to a limit
// (to_rate_pool.h) AND what that amount buys, ONE LANE PER QUERY, grid-stride.  rate_kernel's gather: to_rate_any reads the
// pool exactly as rate_any does, and the amount out is quote_any<KIND, false> on the answer -- the same function on the same
// operands, so amount_out carries cfmm_quote's bits for amount_in.  A read-only gather with two 8-byte stores per query;
// nothing is staged in LDS, no atomics, no state.  The limit travels where the quotes carry the amount given
// (QuoteArgs::amount_in), so the refusal rule is query_read.h's read_query with one test more: a limit must be > 0.  A bad
// query gets NaN in BOTH outputs.
// The Curve search (to_rate_curve) iterates per lane: the lanes of a wavefront wait for its slowest, and the loop keeps two
// bracket ends with their values beside the pool's five scalars -- no array, no scratch.
#pragma once

#include "../../include/cfmm_amd.h"
#include "kind_switch.h"
#include "query_read.h"
#include "quote_kernels.h"
#include "to_rate_pool.h"

namespace cfmm {

template <int KIND>
__device__ __forceinline__ double to_rate_any(const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, int64_t row, int ci, int co,
                                              double lim)
{
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        const double2 R = a.R[row];
        const double g = a.gamma[row];
        const double Ri = ci == 0 ? R.x : R.y, Ro = co == 0 ? R.x : R.y;
        if constexpr (KIND == CFMM_KIND_GEOMEAN) {
            const double2 w = a.w[row];
            return to_rate_weighted(Ri, Ro, ci == 0 ? w.x : w.y, co == 0 ? w.x : w.y, g, lim);
        } else if constexpr (KIND == CFMM_KIND_SOLIDLY) {
            return to_rate_solidly(Ri, Ro, g, lim);
        } else {
            return to_rate_product(Ri, Ro, g, lim);
        }
    } else if constexpr (KIND == CFMM_KIND_UNIV3) {
        return to_rate_univ3(u.cur_a[row], u.cur_b[row], u.cur_c[row], u.curR[row], u.walk[row], u.ticks, u.pg[row].y, ci, lim);
    } else {
        // coin-major columns: coin k of pool i at k·m + i
        const int64_t m = a.m;
        const double Ri = n.R[(int64_t)ci * m + row], Ro = n.R[(int64_t)co * m + row];
        const double g = n.glg[row].x;
        if constexpr (KIND == CFMM_KIND_WEIGHTED) {
            return to_rate_weighted(Ri, Ro, n.par[(int64_t)ci * m + row], n.par[(int64_t)co * m + row], g, lim);
        } else {
            const double2 ab = reinterpret_cast<const double2*>(n.par)[row];   // {α, log β}
            double srho;
            switch (n.n_coins) {
            case 2: srho = quote_sum_logs<2>(n.q, m, row); break;
            case 3: srho = quote_sum_logs<3>(n.q, m, row); break;
            case 4: srho = quote_sum_logs<4>(n.q, m, row); break;
            case 5: srho = quote_sum_logs<5>(n.q, m, row); break;
            case 6: srho = quote_sum_logs<6>(n.q, m, row); break;
            case 7: srho = quote_sum_logs<7>(n.q, m, row); break;
            default: srho = quote_sum_logs<8>(n.q, m, row); break;
            }
            return to_rate_curve(Ri, Ro, srho, ab.x, ab.y, g, lim);
        }
    }
}

// t.q.amount_in: the limits; t.q.amount_out may be null
template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void to_rate_kernel(ToRateArgs t, UniV3Pools u, NCoinPools n)
{
    const QuoteArgs& a = t.q;
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        const Query s = read_query(a, q);
        const bool ok = s.ok && s.amt > 0.0;
        // (a bad query is evaluated at limit +inf: the spot test answers +0.0 at once, nothing iterates)
        const double amt = to_rate_any<KIND>(a, u, n, s.row, s.ci, s.co, ok ? s.amt : __builtin_inf());
        const double out = quote_any<KIND, false>(a, u, n, s.row, s.ci, s.co, ok ? amt : 0.0);
        t.amount[q] = ok ? amt : __builtin_nan("");
        if (a.amount_out) a.amount_out[q] = ok ? out : __builtin_nan("");
    }
}

} // namespace cfmm
