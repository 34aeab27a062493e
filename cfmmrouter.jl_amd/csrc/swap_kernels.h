// swap_kernels.h -- cfmm_swap: exact-input swaps that MOVE the pools (swap_pool.h), ONE LANE PER SWAP of one wave, grid-stride
// over the wave.  quote_kernel's gather with two to four more 8-byte stores per lane: the lane reads its query, computes the
// amount out through quote_one<KIND> -- the very function quote_kernel calls, so the answer carries cfmm_quote's bits -- and
// writes the answer, the pool's new reserves and its refreshed prepared constants back to the segment's own arrays.
// The rows of a wave are DISTINCT (the host numbers the waves: abi_swap.cpp), so no two lanes touch one pool: plain vector
// loads and stores, no LDS, no atomics.  A reserve that leaves the window of the fast arithmetic stores a 1 to the segment's
// flag, as update_two_coin does.  A swap whose new state cfmm_pools_set_* would refuse (swap_pool.h) writes NaN as its
// answer and nothing else; a == 0 writes +0.0 and nothing else.  UniV3: the kernel writes the answer and the price the swap
// comes to rest at and changes nothing -- the host re-prepares the pool.
// The host has checked every query; the clamp-then-poison rule of quote_kernel stays, so that nothing is ever read or
// written out of bounds.
#pragma once

#include "quote_kernels.h"
#include "swap_pool.h"

namespace cfmm {

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void swap_kernel(SwapArgs s, UniV3Pools u, NCoinPools n)
{
    const QuoteArgs& a = s.q;
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        long long row = a.idx ? a.idx[q] : (long long)q;
        int ci = a.coin_in[q];
        int co = a.coin_out ? a.coin_out[q] : 1 - ci;
        const double amt = a.amount_in[q];
        const bool ok = row >= 0 && row < a.m && ci >= 0 && ci < a.n_coins && co >= 0 && co < a.n_coins && ci != co &&
                        amt >= 0.0 && amt < __builtin_inf();
        row = row < 0 ? 0 : (row >= a.m ? a.m - 1 : row);
        ci = ci < 0 ? 0 : (ci >= a.n_coins ? a.n_coins - 1 : ci);
        co = co < 0 ? 0 : (co >= a.n_coins ? a.n_coins - 1 : co);
        const double out = quote_one<KIND>(a, u, n, row, ci, co, ok ? amt : 0.0);
        const double nan = __builtin_nan("");
        if constexpr (KIND == CFMM_KIND_UNIV3) {
            const double P = swap_univ3_price(u.pg[row].x, u.cur_a[row], u.cur_b[row], u.cur_c[row], u.walk[row], u.ticks, u.pg[row].y,
                                              ci, ok ? amt : 0.0);
            s.price[q] = ok ? P : nan;
            a.amount_out[q] = ok ? out : nan;
        } else {
            if (!ok || amt == 0.0) {   // nothing moves
                a.amount_out[q] = ok ? out : nan;
                continue;
            }
            if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
                const double2 R = a.R[row];
                const double g = a.gamma[row];
                const double2 rn = swap_reserves(ci == 0 ? R.x : R.y, co == 0 ? R.x : R.y, g, amt, out);
                if (!swap_reserves_valid(rn, KIND == CFMM_KIND_SOLIDLY)) {
                    a.amount_out[q] = nan;
                    continue;
                }
                const double2 Rn = ci == 0 ? rn : make_double2(rn.y, rn.x);
                s.R[row] = Rn;
                if (s.left_window && !(swap_in_window(Rn.x) && swap_in_window(Rn.y))) *s.left_window = 1;
                if constexpr (KIND == CFMM_KIND_GEOMEAN) s.Q[row] = swap_geomean_q(g, s.eta[row], Rn.x, Rn.y);
                a.amount_out[q] = out;
            } else {
                const int64_t m = a.m;
                const int64_t ji = (int64_t)ci * m + row, jo = (int64_t)co * m + row;
                const double2 rn = swap_reserves(n.R[ji], n.R[jo], n.glg[row].x, amt, out);
                bool valid = swap_reserves_valid(rn, false);
                double qi, qo;
                if constexpr (KIND == CFMM_KIND_WEIGHTED) {
                    qi = swap_weighted_q(rn.x, n.par[ji]);
                    qo = swap_weighted_q(rn.y, n.par[jo]);
                } else {
                    qi = swap_curve_q(rn.x);
                    qo = swap_curve_q(rn.y);
                    const double2 ab = reinterpret_cast<const double2*>(n.par)[row];   // {α, log β}
                    if (valid && ab.x > 0.0) valid = swap_curve_in_range(ab.y, n.q + row, m, n.n_coins, ci, qi, co, qo);
                }
                if (!valid) {
                    a.amount_out[q] = nan;
                    continue;
                }
                s.ncR[ji] = rn.x;
                s.ncR[jo] = rn.y;
                s.ncq[ji] = qi;
                s.ncq[jo] = qo;
                a.amount_out[q] = out;
            }
        }
    }
}

} // namespace cfmm
