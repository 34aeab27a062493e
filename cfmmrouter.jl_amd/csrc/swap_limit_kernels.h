// swap_limit_kernels.h -- cfmm_swap_limit: exact-input swaps that stop where the pool's marginal rate reaches a limit, ONE LANE
// PER SWAP of one wave, grid-stride over the wave.  swap_kernel's body with one step in front: the lane computes
// a_lim = to_rate_any<KIND> (to_rate_kernels.h: the function to_rate_kernel runs, so cfmm_quote_to_rate's bits on the pool as
// the earlier waves left it) where the swap has a limit > 0, else +inf, and used = min(amount_in, a_lim).  From there on it does
// for `used` exactly what swap_kernel does for its amount: quote_one, swap_move, swap_store (UniV3: the landing price through
// swap_univ3_price for the host to apply), so the answer and the new state carry cfmm_swap(used)'s bits.  Beside the answer it
// stores `used` and a status (sweep.h kLimit*):
//   kLimitNone      used == 0 (the spot rate is at or below the limit, or amount_in == 0): used +0.0, out +0.0, nothing moved
//   kLimitRefused   the new state is one cfmm_pools_set_* refuses (swap_pool.h's tests): used and out NaN, nothing moved.
//                   (UniV3: the host tests the landing price, as for cfmm_swap, and rewrites the three answers)
//   kLimitFilled    used == amount_in, bit for bit
//   kLimitPartial   0 < used < amount_in: the pool rests at the limit
// The rows of a wave are distinct (abi_swap.cpp), so plain vector loads and stores, no LDS, no atomics.  The host has checked
// every query; the query is still read by the rule of query_read.h (test, clamp, read, poison) with the tests this entry has:
// the amount may be +inf where the limit is > 0, the limit is finite and >= 0.
#pragma once

#include "swap_kernels.h"
#include "to_rate_kernels.h"

namespace cfmm {

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void swap_limit_kernel(SwapLimitArgs sl, UniV3Pools u, NCoinPools n)
{
    const SwapArgs& s = sl.o.s;
    const QuoteArgs& a = s.q;
    const SwapView v = swap_view(s, n);
    const double nan = __builtin_nan("");
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        long long row = a.idx ? a.idx[q] : (long long)q;
        int ci = a.coin_in[q];
        int co = a.coin_out ? a.coin_out[q] : 1 - ci;
        const double amt = a.amount_in[q], lim = sl.o.max_in[q];
        const bool ok = row >= 0 && row < a.m && ci >= 0 && ci < a.n_coins && co >= 0 && co < a.n_coins && ci != co && amt >= 0.0 &&
                        lim >= 0.0 && lim < __builtin_inf() && (amt < __builtin_inf() || lim > 0.0);
        row = row < 0 ? 0 : (row >= a.m ? a.m - 1 : row);
        ci = clamp_coin(ci, a.n_coins);
        co = clamp_coin(co, a.n_coins);
        if (!ok) {
            a.amount_out[q] = nan;
            sl.used[q] = nan;
            sl.o.status[q] = kLimitRefused;
            if constexpr (KIND == CFMM_KIND_UNIV3) s.price[q] = nan;
            continue;
        }
        const double a_lim = lim > 0.0 ? to_rate_any<KIND>(a, u, n, row, ci, co, lim) : __builtin_inf();
        const double used = amt < a_lim ? amt : a_lim;   // (a NaN a_lim stays)
        const double out = quote_one<KIND>(a, u, n, row, ci, co, used);
        if constexpr (KIND == CFMM_KIND_UNIV3) {
            s.price[q] = swap_univ3_price(u.pg[row].x, u.cur_a[row], u.cur_b[row], u.cur_c[row], u.walk[row], u.ticks, u.pg[row].y, ci, used);
            a.amount_out[q] = out;
            sl.used[q] = used;
            sl.o.status[q] = used == 0.0 ? kLimitNone : (used == amt ? kLimitFilled : kLimitPartial);
        } else {
            if (used == 0.0) {   // nothing moves
                a.amount_out[q] = out;
                sl.used[q] = used;
                sl.o.status[q] = kLimitNone;
                continue;
            }
            const SwapMove mv = swap_move<KIND>(v, a.m, row, ci, co, used, out);
            if (!mv.valid) {
                a.amount_out[q] = nan;
                sl.used[q] = nan;
                sl.o.status[q] = kLimitRefused;
                continue;
            }
            swap_store<KIND>(v, a.m, row, ci, co, mv);
            a.amount_out[q] = out;
            sl.used[q] = used;
            sl.o.status[q] = used == amt ? kLimitFilled : kLimitPartial;
        }
    }
}

} // namespace cfmm
