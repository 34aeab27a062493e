/* cfmm_amd_find_out.h -- the exact-output form of cfmm_find_path, an addition to cfmm_amd.h (same library, same context,
 * same conventions; include it after or instead of cfmm_amd.h, which it includes).  The status codes are cfmm_find_path's
 * CFMM_FOUND* of cfmm_amd.h. */
#ifndef CFMM_AMD_FIND_OUT_H
#define CFMM_AMD_FIND_OUT_H

#include "cfmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cheapest swap path that BUYS an exact amount, FOUND on the device: "I want exactly amount_out of token_out and pay in
 * token_in -- through which pools, and what does it cost?"  It produces the path that cfmm_quote_path_out prices and
 * cfmm_swap_path_out executes (with a limit on the input), as cfmm_find_path produces the one cfmm_quote_path and
 * cfmm_swap_path take.  The best path for an input amount is not the cheapest path for an output amount -- the two depend on
 * depth differently -- so this is a search of its own: cfmm_find_path's, run backwards from the wanted output.  Per query q:
 * token_in[q], token_out[q] (0-based, < n_tokens), amount_out[q] finite and >= 0, at most max_hops (1 .. CFMM_MAX_PATH_HOPS).
 * THE CONTRACT IS THE LAYERED SEARCH, on the market as it stands on the device:
 *   need[0][token_out] = amount_out; everything else is unreached.
 *   need[h][t], h = 1 .. max_hops: the MINIMUM of quote_out(pool, ci -> co, need[h-1][tok(co)]) over every pool of every
 *   segment and every ordered pair of its coins (ci, co) with tok(ci) == t whose destination need[h-1][tok(co)] is reached.  A
 *   quote that is NaN, +inf (that pool cannot give that much) or <= 0 enters nothing.
 *   amount_in = the minimum over h >= 1 of need[h][token_in]; the path has the FEWEST hops h* that attain it bit for bit, and
 *   is found by a forward walk from (h*, token_in): hop k sits at layer h* - k with the current token t, and is the
 *   SMALLEST (segment, row, coin_in, coin_out), in lexicographic order, among the edges out of t whose quote equals
 *   need[h* - k][t] bit for bit; tok(coin_out) becomes the current token.  Hops come out in path order, hop 0 first.
 * So the answer is a pure function of the market and the query -- not of launch geometry, the order atomics arrive in, how
 * queries are batched or option "find_lds".  The quotes are cfmm_quote_out's own, and EVERY HOP IS QUOTED AGAINST THE POOL AS IT
 * STANDS, cfmm_quote_path_out's rule: cfmm_quote_path_out on the returned arrays answers amount_in bit for bit, and every
 * hop_in[k] with it equals the layer value need[h* - k][.].  What is found is a WALK, as in cfmm_find_path: it may pass a token
 * twice and may visit a pool twice (quoted twice from the same reserves); a search constrained to simple paths is not
 * offered.  Where every pool's quote_out is non-decreasing in the wanted output -- it is mathematically; rounding can break it
 * by ulps -- the layered minimum is the minimum over all walks of at most max_hops hops; the contract is the layered one.
 * token_in == token_out is allowed: the cheapest cycle through that token.
 *   amount_in, n_hops, status   [count]
 *   hop_seg, hop_row, hop_coin_in, hop_coin_out   [max_hops][count], hop-major: exactly what cfmm_quote_path_out and
 *                 cfmm_swap_path_out take (with n_hops and max_hops); -1 in the slots at k >= n_hops[q]
 *   status[q]:
 *     CFMM_FOUND          a walk was found; every pool on it is visited once
 *     CFMM_FOUND_NONE     n_hops 0, hop slots -1, and amount_in is
 *                           +inf  when token_in is not reached within max_hops -- which covers every case where no pool can give
 *                                 that much: cfmm_quote_out's convention
 *                           +0.0  when amount_out[q] == 0: buying nothing costs nothing and needs no path
 *     CFMM_FOUND_REPEATS  a walk was found and its amounts are cfmm_quote_path_out's, but it visits some pool more than once:
 *                         cfmm_swap_path_out would refuse it as one path
 * The checks are cfmm_find_path's: everything is checked before anything is enqueued (count >= 0, max_hops, no null array,
 * every token in 0 .. n_tokens-1, every amount finite and >= 0); a failure is CFMM_ERR_INVALID_ARG, names the query
 * ("cfmm_find_path_out: query 12: ...") and leaves the outputs untouched.  Read-only exactly as cfmm_quote_out.  Synchronous
 * on the context's stream; count == 0 is a no-op; a context without pools answers CFMM_FOUND_NONE everywhere; large-market mode
 * needs nothing special.  A MULTI-DEVICE CONTEXT answers CFMM_ERR_UNSUPPORTED.  Launches, scratch (bounded by 256 MiB, larger
 * calls in chunks of queries with the same results) and option "find_lds" are cfmm_find_path's; the read-only options
 * "find_launches", "find_relax_ns", "find_walk_ns", "find_relax_ns_<h>", "find_claim_ns_<h>" and "find_advance_ns_<h>" describe
 * the latest call of EITHER entry (h is the layer: the forward walk claims layer h* first). */
int cfmm_find_path_out(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                       const double* amount_out, double* amount_in, int32_t* n_hops, int32_t* hop_seg, int64_t* hop_row,
                       int32_t* hop_coin_in, int32_t* hop_coin_out, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
