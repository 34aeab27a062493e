// swap_out_kernels.h -- cfmm_swap_out: exact-output swaps that MOVE the pools, ONE LANE PER SWAP of one wave, grid-stride
// over the wave.  swap_kernel with the closed form exchanged: the lane reads its query, computes the amount to tender through
// quote_out_one<KIND> -- the very function quote_out_kernel calls, so the answer carries cfmm_quote_out's bits -- and leaves
// the pool at R_in + γ·in, R_out − want (swap_pool.h swap_reserves: the pool gives exactly the amount asked for, not
// quote(in)), with the prepared constants refreshed by swap_kernel's own expressions.  The rows of a wave are distinct
// (abi_swap.cpp), so plain vector loads and stores, no LDS, no atomics.  Every swap gets a status (sweep.h kSwap*):
//   kSwapUnobtainable  quote_out answers +inf: the answer is +inf                          nothing else is written
//   kSwapRefused       the new state is one cfmm_pools_set_* refuses (swap_pool.h's tests,   "
//                      as swap_kernel applies them; UniV3: a landing price that is not
//                      finite and > 0): the answer is NaN
//   kSwapOverLimit     !(in <= max_in[q]): the answer is the quote it would have cost        "
//   kSwapApplied       the answer, then the new state; want == 0 answers +0.0 and writes no state
// in that order of precedence (cfmm_swap_path_out tests its hops in the same order).
// UniV3: the state is the price and the price is determined by the input: the pool rests at swap_univ3_price(.., in), the
// function swap_kernel uses, which goes to the price scratch for the host to apply (abi_swap.cpp).  quote_out_univ3 finds its
// record on the ΣR_out sums and swap_univ3_price finds its own on the Σδmax sums; when want equals a running ΣR_out at a tick
// boundary, in·γ may round to either side of the matching Σδmax and the two then name neighbouring records.  That is
// harmless: the price is continuous across the boundary -- the far edge of record e (d_t = δmax_e) and the near edge of
// record e+1 (d_t = 0) are the same tick price up to the rounding of their prepared constants.
// The host has checked every query; the clamp-then-poison rule of quote_kernel stays, so that nothing is ever read or
// written out of bounds.
#pragma once

#include "quote_kernels.h"
#include "swap_pool.h"

namespace cfmm {

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void swap_out_kernel(SwapOutArgs so, UniV3Pools u, NCoinPools n)
{
    const SwapArgs& s = so.s;
    const QuoteArgs& a = s.q;
    const double nan = __builtin_nan("");
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        long long row = a.idx ? a.idx[q] : (long long)q;
        int ci = a.coin_in[q];
        int co = a.coin_out ? a.coin_out[q] : 1 - ci;
        const double want = a.amount_in[q];   // the wanted output
        const bool ok = row >= 0 && row < a.m && ci >= 0 && ci < a.n_coins && co >= 0 && co < a.n_coins && ci != co &&
                        want >= 0.0 && want < __builtin_inf();
        row = row < 0 ? 0 : (row >= a.m ? a.m - 1 : row);
        ci = ci < 0 ? 0 : (ci >= a.n_coins ? a.n_coins - 1 : ci);
        co = co < 0 ? 0 : (co >= a.n_coins ? a.n_coins - 1 : co);
        const double in = quote_out_one<KIND>(a, u, n, row, ci, co, ok ? want : 0.0);   // the input to tender
        const bool within = !so.max_in || in <= so.max_in[q];
        if (!ok || in == __builtin_inf()) {
            a.amount_out[q] = ok ? in : nan;
            so.status[q] = ok ? kSwapUnobtainable : kSwapRefused;
            continue;
        }
        if constexpr (KIND == CFMM_KIND_UNIV3) {
            const double P = swap_univ3_price(u.pg[row].x, u.cur_a[row], u.cur_b[row], u.cur_c[row], u.walk[row], u.ticks, u.pg[row].y,
                                              ci, in);
            const bool valid = swap_finite_pos(P);
            const int32_t st = !valid ? kSwapRefused : (within ? kSwapApplied : kSwapOverLimit);
            s.price[q] = st == kSwapApplied ? P : nan;
            a.amount_out[q] = valid ? in : nan;
            so.status[q] = st;
        } else {
            if (want == 0.0) {   // nothing moves: in is +0.0, within any limit
                a.amount_out[q] = in;
                so.status[q] = kSwapApplied;
                continue;
            }
            if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
                const double2 R = a.R[row];
                const double g = a.gamma[row];
                const double2 rn = swap_reserves(ci == 0 ? R.x : R.y, co == 0 ? R.x : R.y, g, in, want);
                if (!swap_reserves_valid(rn, KIND == CFMM_KIND_SOLIDLY)) {
                    a.amount_out[q] = nan;
                    so.status[q] = kSwapRefused;
                    continue;
                }
                a.amount_out[q] = in;
                so.status[q] = within ? kSwapApplied : kSwapOverLimit;
                if (!within) continue;
                const double2 Rn = ci == 0 ? rn : make_double2(rn.y, rn.x);
                s.R[row] = Rn;
                if (s.left_window && !(swap_in_window(Rn.x) && swap_in_window(Rn.y))) *s.left_window = 1;
                if constexpr (KIND == CFMM_KIND_GEOMEAN) s.Q[row] = swap_geomean_q(g, s.eta[row], Rn.x, Rn.y);
            } else {
                const int64_t m = a.m;
                const int64_t ji = (int64_t)ci * m + row, jo = (int64_t)co * m + row;
                const double2 rn = swap_reserves(n.R[ji], n.R[jo], n.glg[row].x, in, want);
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
                    so.status[q] = kSwapRefused;
                    continue;
                }
                a.amount_out[q] = in;
                so.status[q] = within ? kSwapApplied : kSwapOverLimit;
                if (!within) continue;
                s.ncR[ji] = rn.x;
                s.ncR[jo] = rn.y;
                s.ncq[ji] = qi;
                s.ncq[jo] = qo;
            }
        }
    }
}

} // namespace cfmm
