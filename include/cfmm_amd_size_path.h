/* cfmm_amd_size_path.h -- sizing a swap path on the device, an addition to cfmm_amd.h (same library, same context, same
 * conventions; include it after or instead of cfmm_amd.h, which it includes). */
#ifndef CFMM_AMD_SIZE_PATH_H
#define CFMM_AMD_SIZE_PATH_H

#include "cfmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CFMM_SIZE_POINTS 64        /* trial sizes per round: one wavefront */
#define CFMM_MAX_SIZE_ROUNDS 16
#define CFMM_SIZED 0               /* a size with gain > 0 below the limit */
#define CFMM_SIZED_NONE 1          /* no trial size gains: amount_in 0.0, amount_out 0.0, gain 0.0 */
#define CFMM_SIZED_AT_LIMIT 2      /* gain > 0 and amount_in == max_amount_in, bit for bit: the limit binds */
#define CFMM_SIZED_NAN 3           /* some round had no trial size whose gain is a number: outputs NaN */

/* HOW MUCH to put into a path: the input, at most max_amount_in[p], that maximises the path's gain -- the question before
 * cfmm_swap_path ("this cycle is profitable at a probe size; at which size is it most profitable?").  The path arguments are
 * exactly cfmm_quote_path's: hop-major [max_hops][count] arrays, 1 .. CFMM_MAX_PATH_HOPS hops per path, slots at
 * k >= n_hops[p] ignored.  The gain of path p at size x is
 *     gain(x) = value_out[p] * quote_path(p, x) - value_in[p] * x,
 * a product, a product and a difference, each rounded on its own (no fused multiply-add).  value_in and value_out may each be
 * NULL, which means 1.0: with both NULL the gain is "out minus in", the profit of a cycle; with prices given it is the worth
 * of a path that is no cycle at outside prices (a venue off this market, say).  A value array that is given holds finite
 * entries > 0.
 * THE CONTRACT IS THE BRACKETING SEARCH, on the market as it stands on the device:
 *   lo = 0, hi = max_amount_in[p].  For round 1 .. rounds:
 *     the CFMM_SIZE_POINTS trial sizes are x_0 = lo, x_63 = hi and otherwise x_j = min(lo + (hi - lo) * (j / 63.0), hi) --
 *       the subtraction, the division, the product and the sum each rounded on their own;
 *     y_j = quote_path(p, x_j), with cfmm_quote_path's own per-hop forms, EVERY HOP QUOTED AGAINST THE POOL AS IT STANDS
 *       (cfmm_quote_path's rule: a pool visited twice is quoted twice from the same reserves);
 *     g_j = gain(x_j);
 *     j* = the smallest j whose g_j is the largest, compared as numbers; a NaN loses to every number;
 *     the next bracket is [x_max(j*-1, 0), x_min(j*+1, 63)].
 *   After the last round amount_in = x_j*, amount_out = y_j*, gain = g_j*, and
 *     status[p] = CFMM_SIZED_NAN       some round had no trial size whose gain is a number: the three outputs are NaN
 *                 CFMM_SIZED_NONE      !(gain > 0): the three outputs are written as +0.0 (max_amount_in == 0 ends here)
 *                 CFMM_SIZED_AT_LIMIT  gain > 0 and amount_in == max_amount_in[p] bit for bit: the limit binds
 *                 CFMM_SIZED           gain > 0 below the limit
 * So the answer is a pure function of the market, the path and `rounds` -- not of launch geometry (option "size_max_blocks")
 * or of how paths are batched -- and cfmm_quote_path at the returned amount_in answers amount_out bit for bit.
 * What the search finds.  Every pool family's quote is concave and non-decreasing in its input, so a path's gain is concave:
 * its maximiser lies inside every bracket, and the bracket shrinks by 2/63 per round.  Rounding can break concavity by ulps:
 * once neighbouring trial sizes differ in gain by less than the rounding of the amounts, further rounds move amount_in without
 * improving the gain; the bracket is then near sqrt(eps) of the scale.  A numpy run of this contract on 4000 random two-pool
 * ProductTwoCoin cycles (tests/test_size_path_cpu.py) gave: through round 3 amount_in within 0.3 of the bracket of the
 * closed-form optimum; the gain within 6e-10 (relative) of the closed-form gain at 4 rounds, within 1.2e-12 at 5 rounds, and no
 * improvement beyond 6 rounds (4e-13: the rounding of the gain itself).
 * Against 80-digit optima on every pool family, alone and mixed, 1 .. 8 hops (tests/test_optimum_precise_cpu.py,
 * profiles/optimum_precise.txt): over exact quotes the search is within 3.5e-13 of the optimal gain at 5 rounds on smooth optima,
 * but within 2.4e-7 only where the optimum sits on the end of a UniV3 list and 5.1e-8 on a tick boundary (a kink gains one
 * bracket per round, not its square; 16 rounds: 1e-15); "the maximiser lies in the bracket" holds through round 3 and from round 5
 * on amount_in is placed by the noise of the quotes (within 4.3e-5 of the optimum's: the gain is flat); on a Solidly cycle sized
 * below 1e-4 of the reserves the quote's noise is up to 0.13 of the optimal gain and the reported gain can exceed the optimum's.
 * The Python default is therefore rounds = 5.  THE CONTRACT IS THE SEARCH, not "the global maximum".
 * It sizes ONE path on the STANDING market: it does not split an amount over several paths (cfmm_split_paths of
 * cfmm_amd_split.h does), and no state advances between hops.
 *   amount_in, amount_out, gain, status   [count]
 * Everything is checked before anything is enqueued: cfmm_quote_path's checks of the paths, max_amount_in[p] finite and
 * >= 0, rounds in 1 .. CFMM_MAX_SIZE_ROUNDS, the values, no null output array.  A failure is CFMM_ERR_INVALID_ARG, names the
 * path and the hop ("cfmm_size_path: path 12, hop 3: ...") and leaves the outputs untouched.  Synchronous on the context's
 * stream; read-only exactly as cfmm_quote; count == 0 is a no-op; large-market mode needs nothing special; on a context
 * sharded with cfmm_set_peers or RCCL the call is local to the rank.  A MULTI-DEVICE CONTEXT runs the search on the host
 * through cfmm_quote_path's parent path, one call of 64 * count paths per round, with the grid and selection arithmetic of
 * the kernel: the same bits.
 * Read-only options: under "time_kernels", "size_ns" is the latest call's kernel span (a parent: the sum over its rounds of
 * "quote_ns"); "size_launches" its kernel launches (a parent: its cfmm_quote_path calls).  Option "size_max_blocks" (any
 * value >= 1) caps the grid: the same bits either way, a measurement and test switch like "find_lds". */
int cfmm_size_path(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                   const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out,
                   const double* max_amount_in, const double* value_in, const double* value_out, int32_t rounds,
                   double* amount_in, double* amount_out, double* gain, int32_t* status);

/* The same on device arrays (d_value_in / d_value_out may be NULL), asynchronous on the context's stream, single-device
 * contexts only.  Only the scalars and the null pointers are checked: a path whose n_hops is outside 1 .. max_hops, that has
 * an out-of-range hop, or whose max_amount_in or value is not a valid number, yields CFMM_SIZED_NAN with NaN outputs for
 * that path alone.  Indices are clamped before any read (cfmm_quote_path_dev's rule); neighbouring paths are unaffected. */
int cfmm_size_path_dev(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                       const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                       const double* d_max_amount_in, const double* d_value_in, const double* d_value_out, int32_t rounds,
                       double* d_amount_in, double* d_amount_out, double* d_gain, int32_t* d_status);

#ifdef __cplusplus
}
#endif
#endif
