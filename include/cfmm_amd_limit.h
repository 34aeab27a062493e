/* cfmm_amd_limit.h -- price-limited swaps: the amount that brings a pool's marginal rate down to a limit, and the swap that
 * stops there.  An addition to cfmm_amd_rate.h (same library, same context, same conventions; include it after or instead of
 * cfmm_amd_rate.h, which it includes). */
#ifndef CFMM_AMD_LIMIT_H
#define CFMM_AMD_LIMIT_H

#include "cfmm_amd_rate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The inverse of cfmm_quote_rate: how much can be tendered before the pool's marginal rate falls to rate_limit[q].
 *     amount_in[q] = sup { a >= 0 : rate(pool, coin_in -> coin_out, a) >= rate_limit[q] },     0 where the set is empty,
 * rate what cfmm_quote_rate answers (the right derivative of the quote, fee included; non-increasing in a on every family), on
 * the pool as it stands.  amount_out[q] (may be NULL) is, bit for bit, what cfmm_quote answers for amount_in[q].
 *   - exactly +0.0 (and amount_out +0.0) where the spot rate -- cfmm_quote_rate at amount 0 -- is already <= the limit;
 *   - UniV3: a limit inside an empty tick's price range answers the boundary in front of it; a limit below the rate at the end
 *     of the direction's last tick answers the direction's whole capacity, the amount cfmm_quote_out(cfmm_quote(.)) reports;
 *   - an answer that overflows a double is +inf (amount_out is then cfmm_quote's formula at +inf, which need not be a number).
 * With s the spot rate, x' = R_in + gamma*a:
 *   Product    x'/R_in = sqrt(s/r)
 *   weighted   x'/R_in = (s/r)^(1/(1 + w_in/w_out))                      (GeometricMean and the N-coin pools)
 *   Solidly    u = y'/x' with u(3 + u^2)/(1 + 3u^2) = r/gamma in closed form, then (x'/R_in)^4 = (t0 + t0^3)/(u + u^3), t0 = R_out/R_in
 *   Curve      no closed form: a bracketed search on cfmm_quote_rate's own rate, at most 128 evaluations per query; the answer
 *              is a pure function of pool and limit (no dependence on batching or launch geometry) and, should the cap be hit,
 *              the lower end of the bracket -- an amount whose rate is still >= the limit
 *   UniV3      the tick in which gamma*k/s^2 crosses r, found by bisection over the direction's ticks, and the closed form in it
 * The rate the pool rests at after tendering the answer is the limit only TO ROUNDING: cfmm_quote_rate(amount_in[q]) may lie an
 * ulp-scale amount below rate_limit[q].  A caller that must never cross its limit passes a margin.
 * The query arguments are cfmm_quote's with rate_limit in the place of the amount: idx == NULL is the dense pass over rows
 * 0 .. count-1, coin_out == NULL means 1 - coin_in (two-coin kinds and UniV3).  Every rate_limit must be finite and > 0.
 * Checks, messages (prefix "cfmm_quote_to_rate:", the failing query named, outputs untouched, nothing enqueued), the read-only
 * guarantee, large-market mode and count == 0 are cfmm_quote's.  On a multi-device context the queries go to the shards that
 * hold their rows and the answers carry the bits of a single device.  Option "limit_ns" (read-only, under "time_kernels"): the
 * span of the latest call's kernel, on a multi-device context the longest among the shards touched. */
int cfmm_quote_to_rate(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                       const int32_t* coin_out, const double* rate_limit, double* amount_in, double* amount_out);

/* The same on DEVICE arrays, by cfmm_quote_rate_dev's rule: asynchronous on the context's stream, nothing checked on the host
 * but the scalars; every index is clamped before any read, and a query whose row, coins or limit are out of range gets NaN in
 * BOTH outputs, for that query alone.  d_amount_out may be NULL.  Single-device contexts only (CFMM_ERR_UNSUPPORTED otherwise). */
int cfmm_quote_to_rate_dev(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
                           const int32_t* d_coin_out, const double* d_rate_limit, double* d_amount_in, double* d_amount_out);

#define CFMM_LIMIT_FILLED  0   /* used == amount_in, bit for bit */
#define CFMM_LIMIT_PARTIAL 1   /* 0 < used < amount_in: the pool rests at the limit */
#define CFMM_LIMIT_NONE    2   /* spot already at or below the limit (or amount_in == 0): used +0.0, out +0.0, nothing moved */
#define CFMM_LIMIT_REFUSED 3   /* the new state is one cfmm_pools_set_* refuses: used and out NaN, nothing moved */

/* cfmm_swap behind a limit on the marginal rate: swap q tenders
 *     amount_used[q] = min(amount_in[q], cfmm_quote_to_rate(rate_limit[q]))            on the pool as the earlier swaps of the
 * batch left it, bit for bit; amount_out[q] and the pool's new state are, bit for bit, those of cfmm_swap(amount_used[q]).
 * rate_limit[q] must be finite and >= 0; +0.0 means "no limit for this swap" (the swap is cfmm_swap's).  amount_in[q] must be
 * >= 0 and may be +inf -- "as much as it takes" -- only where the limit is > 0.  status (may be NULL) receives CFMM_LIMIT_*.
 * The swaps apply in caller order, by waves of distinct rows, as cfmm_swap's; a multi-device context behaves as it does for
 * cfmm_swap.  Checks, messages (prefix "cfmm_swap_limit:"), untouched outputs on refusal and the options "swap_ns" /
 * "swap_refused" / "swap_launches" are cfmm_swap's.  After a CFMM_LIMIT_PARTIAL swap the pool's spot rate is the limit to
 * rounding and may lie an ulp-scale amount below it (see cfmm_quote_to_rate).  There is no _dev form: the waves are decided on
 * the host. */
int cfmm_swap_limit(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                    const int32_t* coin_out, const double* amount_in, const double* rate_limit, double* amount_used,
                    double* amount_out, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
