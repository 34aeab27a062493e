/* cfmm_amd_rate.h -- marginal rates of the exact-input quotes: spot price and price impact, an addition to cfmm_amd.h (same
 * library, same context, same conventions; include it after or instead of cfmm_amd.h, which it includes). */
#ifndef CFMM_AMD_RATE_H
#define CFMM_AMD_RATE_H

#include "cfmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cfmm_quote's answer AND its marginal rate, from one read of each pool.  The query arguments are cfmm_quote's.
 * amount_out[q] is, bit for bit, what cfmm_quote answers for the query.  rate[q] is the RIGHT derivative of
 * a -> cfmm_quote(pool, coin_in -> coin_out, a) at a = amount_in[q]: γ·∂φ/∂R_in ÷ ∂φ/∂R_out at the state the trade leaves,
 * R + γ·a·e_in − amount_out·e_out.  At a = 0 it is the pool's spot rate, fee included; the execution price of the query is
 * amount_out/amount_in and its price impact 1 − amount_out/(amount_in·rate at 0).  With x = γa, x′ = R_in + x, y′ = R_out − out:
 *   Product    γ·R_in·R_out/x′²
 *   weighted   γ·(w_in/w_out)·y′/x′                                    (GeometricMean and the N-coin pools)
 *   Solidly    γ·u(3 + u²)/(1 + 3u²), u = y′/x′
 *   Curve      γ·(α + P′/x′)/(α + P′/y′), P′ = β/ΠR′
 *   UniV3      γ·k/(s_in + d)² in the tick the amount lands in, d the part of γa that reaches it; +0.0 once the ladder of the
 *              direction is exhausted (or holds no liquidity); at an exact tick boundary the NEXT tick's rate; at a = 0 the
 *              first tick of the direction that has capacity, also when the current tick is empty
 * amount_in == NULL means 0 for every query -- a spot-price table -- and amount_out may be NULL exactly then (else it
 * receives +0.0).  idx == NULL is the dense, coalesced pass over rows 0 .. count-1 of the segment.
 * Checks, messages (prefix "cfmm_quote_rate:", the failing query named, outputs untouched, nothing enqueued), the read-only
 * guarantee, large-market mode and count == 0 are cfmm_quote's.  On a multi-device context the queries go to the shards
 * that hold their rows and the answers carry the bits of a single device; on a cfmm_set_peers / RCCL context the call is
 * rank-local.  Option "rate_ns" (read-only, under "time_kernels"): the span of the latest call's kernel, on a multi-device
 * context the longest among the shards touched. */
int cfmm_quote_rate(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                    const int32_t* coin_out, const double* amount_in, double* amount_out, double* rate);

/* The same on DEVICE arrays, by cfmm_quote_dev's rule: asynchronous on the context's stream, nothing checked on the host
 * but the scalars; every index is clamped before any read, and a query whose row, coins or amount are out of range gets NaN
 * in BOTH outputs, for that query alone.  d_amount_in may be NULL (every amount 0), d_amount_out exactly then.  Single-device
 * contexts only (CFMM_ERR_UNSUPPORTED otherwise). */
int cfmm_quote_rate_dev(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
                        const int32_t* d_coin_out, const double* d_amount_in, double* d_amount_out, double* d_rate);

/* cfmm_quote_path's answer and the path's marginal rate.  The path arguments, checks and refusals are cfmm_quote_path's
 * (prefix "cfmm_quote_path_rate:").  x_0 = amount_in[p], x_{k+1} = cfmm_quote(hop k, x_k), r_k = rate of (hop k, x_k) as
 * cfmm_quote_rate answers it; every hop is evaluated against the pool as it stands.  amount_out[p] and hop_out are
 * cfmm_quote_path's, bit for bit; hop_rate[k*count+p] = r_k; rate[p] = ((r_0·r_1)·r_2)..., each product rounded on its own:
 * the chain rule, a pure function of market and path.  A hop of rate 0 (an exhausted ladder) makes the path's rate 0; the
 * hops behind it are still evaluated.  Unused hop_out / hop_rate slots are NaN.  hop_out and hop_rate may be NULL, each on
 * its own; both are [max_hops][count].  On a multi-device context the paths are walked level by level through
 * cfmm_quote_rate and folded on the host, with the same bits.  "rate_ns" as above. */
int cfmm_quote_path_rate(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                         const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out,
                         const double* amount_in, double* amount_out, double* rate, double* hop_out, double* hop_rate);

/* The same on DEVICE arrays, by cfmm_quote_path_dev's rule: a bad n_hops or hop makes amount_out AND rate of that path NaN
 * (and the hop slots from the bad hop on), nothing is read out of bounds.  Single-device contexts only. */
int cfmm_quote_path_rate_dev(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                             const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                             const double* d_amount_in, double* d_amount_out, double* d_rate, double* d_hop_out,
                             double* d_hop_rate);

#ifdef __cplusplus
}
#endif
#endif
