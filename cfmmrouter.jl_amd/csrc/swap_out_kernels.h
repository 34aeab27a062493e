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
// The host has checked every query; the query is still read by the rule of query_read.h (read_query), so that nothing is
// ever read or written out of bounds.  The new state is swap_pool.h's: swap_move computes and tests it, swap_store writes it.
#pragma once

#include "quote_kernels.h"
#include "swap_pool.h"

namespace cfmm {

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void swap_out_kernel(SwapOutArgs so, UniV3Pools u, NCoinPools n)
{
    const SwapArgs& s = so.s;
    const QuoteArgs& a = s.q;
    const SwapView v = swap_view(s, n);
    const double nan = __builtin_nan("");
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        const Query r = read_query(a, q);
        const double want = r.amt;   // the wanted output
        const double in = quote_out_one<KIND>(a, u, n, r.row, r.ci, r.co, r.ok ? want : 0.0);   // the input to tender
        const bool within = !so.max_in || in <= so.max_in[q];
        if (!r.ok || in == __builtin_inf()) {
            a.amount_out[q] = r.ok ? in : nan;
            so.status[q] = r.ok ? kSwapUnobtainable : kSwapRefused;
            continue;
        }
        if constexpr (KIND == CFMM_KIND_UNIV3) {
            const double P = swap_univ3_price(u.pg[r.row].x, u.cur_a[r.row], u.cur_b[r.row], u.cur_c[r.row], u.walk[r.row], u.ticks,
                                              u.pg[r.row].y, r.ci, in);
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
            const SwapMove mv = swap_move<KIND>(v, a.m, r.row, r.ci, r.co, in, want);
            if (!mv.valid) {
                a.amount_out[q] = nan;
                so.status[q] = kSwapRefused;
                continue;
            }
            a.amount_out[q] = in;
            so.status[q] = within ? kSwapApplied : kSwapOverLimit;
            if (within) swap_store<KIND>(v, a.m, r.row, r.ci, r.co, mv);
        }
    }
}

} // namespace cfmm
