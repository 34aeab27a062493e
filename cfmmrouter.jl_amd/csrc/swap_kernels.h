// swap_kernels.h -- cfmm_swap: exact-input swaps that MOVE the pools (swap_pool.h), ONE LANE PER SWAP of one wave, grid-stride
// over the wave.  quote_kernel's gather with two to four more 8-byte stores per lane: the lane reads its query, computes the
// amount out through quote_one<KIND> -- the very function quote_kernel calls, so the answer carries cfmm_quote's bits -- and
// writes the answer, the pool's new reserves and its refreshed prepared constants back to the segment's own arrays.
// The rows of a wave are DISTINCT (the host numbers the waves: abi_swap.cpp), so no two lanes touch one pool: plain vector
// loads and stores, no LDS, no atomics.  A reserve that leaves the window of the fast arithmetic stores a 1 to the segment's
// flag, as update_two_coin does.  A swap whose new state cfmm_pools_set_* would refuse (swap_pool.h) writes NaN as its
// answer and nothing else; a == 0 writes +0.0 and nothing else.  UniV3: the kernel writes the answer and the price the swap
// comes to rest at and changes nothing -- the host re-prepares the pool.
// The host has checked every query; the query is still read by the rule of query_read.h (read_query), so that nothing is
// ever read or written out of bounds.  The new state is swap_pool.h's: swap_move computes and tests it, swap_store writes it.
#pragma once

#include "quote_kernels.h"
#include "swap_pool.h"

namespace cfmm {

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void swap_kernel(SwapArgs s, UniV3Pools u, NCoinPools n)
{
    const QuoteArgs& a = s.q;
    const SwapView v = swap_view(s, n);
    const double nan = __builtin_nan("");
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        const Query r = read_query(a, q);
        const double out = quote_one<KIND>(a, u, n, r.row, r.ci, r.co, r.ok ? r.amt : 0.0);
        if constexpr (KIND == CFMM_KIND_UNIV3) {
            const double P = swap_univ3_price(u.pg[r.row].x, u.cur_a[r.row], u.cur_b[r.row], u.cur_c[r.row], u.walk[r.row], u.ticks,
                                              u.pg[r.row].y, r.ci, r.ok ? r.amt : 0.0);
            s.price[q] = r.ok ? P : nan;
            a.amount_out[q] = r.ok ? out : nan;
        } else {
            if (!r.ok || r.amt == 0.0) {   // nothing moves
                a.amount_out[q] = r.ok ? out : nan;
                continue;
            }
            const SwapMove mv = swap_move<KIND>(v, a.m, r.row, r.ci, r.co, r.amt, out);
            if (!mv.valid) {
                a.amount_out[q] = nan;
                continue;
            }
            swap_store<KIND>(v, a.m, r.row, r.ci, r.co, mv);
            a.amount_out[q] = out;
        }
    }
}

} // namespace cfmm
