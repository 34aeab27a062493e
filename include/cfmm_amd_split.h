/* cfmm_amd_split.h -- splitting an order over several swap paths on the device, an addition to cfmm_amd.h (same library, same
 * context, same conventions; include it after or instead of cfmm_amd.h, which it includes). */
#ifndef CFMM_AMD_SPLIT_H
#define CFMM_AMD_SPLIT_H

#include "cfmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CFMM_SPLIT_POINTS 64         /* grid points per path and round: one wavefront */
#define CFMM_MAX_SPLIT_PATHS 8       /* paths per order */
#define CFMM_MAX_SPLIT_ROUNDS 16
#define CFMM_SPLIT_OK 0
#define CFMM_SPLIT_NONE 1            /* amount 0, or total_out not > 0: every output of the order +0.0 */
#define CFMM_SPLIT_NAN 2             /* some greedy step had no increment that is a number, or the total is none: outputs NaN */
#define CFMM_SPLIT_SATURATED 3       /* shares are valid, but a step of the LAST round took an increment that is not > 0:
                                        part of the amount buys nothing, the paths cannot absorb it */

/* HOW MUCH OF AN ORDER GOES DOWN EACH PATH: "I have A of token X and these K routes to Y; how much goes down each?" -- the
 * question between cfmm_find_path (one path) and cfmm_swap_path (execution) for an order that is large against the pools it
 * crosses.  The n_paths paths are exactly cfmm_quote_path's: hop-major [max_hops][n_paths] arrays, 1 .. CFMM_MAX_PATH_HOPS hops
 * per path, slots at k >= n_hops[p] ignored.  Order g owns the paths order_first[g] .. order_first[g+1] - 1 -- K of them,
 * 1 <= K <= CFMM_MAX_SPLIT_PATHS -- and has the amount A = amount_in[g] to spread over them.
 * THE CONTRACT IS THE SEARCH, on the market as it stands on the device, every operation rounded on its own (no fused
 * multiply-add):
 *   base_k = 0 (k = 0 .. K-1);  rem = A
 *   for round r = 1 .. rounds:
 *     s = rem / 63.0
 *     x[k][j] = base_k + s * j  (j = 0 .. 62: the product, then the sum);  x[k][63] = base_k + rem
 *     y[k][j] = quote_path(path k, x[k][j]), with cfmm_quote_path's own per-hop forms, EVERY HOP QUOTED AGAINST THE POOL AS IT
 *       STANDS;
 *     n_k = 0;  63 times:
 *       d_k = y[k][n_k + 1] - y[k][n_k]
 *       k* = the smallest k whose d_k is the largest, compared as numbers (+0.0 == -0.0); a NaN loses to every number
 *       (no d_k is a number: the order is CFMM_SPLIT_NAN);  n_{k*} += 1
 *     if r < rounds:  m_k = max(n_k - 1, 0);  base_k = x[k][m_k];
 *                     rem = max(A - (base_0 + base_1 + ... in increasing k), 0.0)
 *   path_amount_in[k] = x[k][n_k],  path_amount_out[k] = y[k][n_k]  (of the last round);
 *   total_out = y_0 + y_1 + ... in increasing k, and
 *     status[g] = CFMM_SPLIT_NAN        some greedy step of some round had no increment that is a number, or total_out is
 *                                       no number (a path that quotes NaN everywhere receives no slice, but its output is
 *                                       NaN): the order's shares, outputs and total are NaN
 *                 CFMM_SPLIT_NONE       A == 0 or total_out is a number that is not > 0: they are written as +0.0
 *                 CFMM_SPLIT_SATURATED  a step of the LAST round took an increment that is not > 0: the shares are valid and
 *                                       sum to A, but part of A buys nothing -- the paths cannot absorb it
 *                 CFMM_SPLIT_OK         otherwise
 * This is greedy marginal allocation with scaling, after the scaling algorithm for the resource allocation problem (D. S.
 * Hochbaum, "Lower and upper bounds for the allocation problem and other nonlinear optimization problems", Mathematics of
 * Operations Research 19 (1994); cited from memory).  Every pool family's quote is concave and non-decreasing, and so is a
 * path's: for such quotes the greedy is optimal on each round's grid, and after the step back rem is at most K slices, so it
 * shrinks by at least 63/K per round.  The step back of ONE slice is a lower bound of the finer optimum for two paths.  With K
 * paths it is not always one: each of the other paths may want up to a slice more than the grid gave it, so the path that took
 * the slack can stand up to K-1 slices above its optimum, and no later round takes a share below its restart point.  Rounding
 * can break concavity by ulps.  THE CONTRACT IS THE SEARCH, not "the global optimum".
 * So the answer is a pure function of the market, the order and `rounds` -- not of launch geometry (option "split_max_blocks")
 * or of how orders are batched.  With K = 1 the single share is A bit for bit, and cfmm_quote_path on path k at
 * path_amount_in[k] answers path_amount_out[k] bit for bit.
 * What the search finds.  A numpy run of this contract on 4000 random orders (tests/test_split_paths_cpu.py: K = 1 .. 8
 * ProductTwoCoin chains of 1 .. 3 hops, A from 10 to 1e6 against reserves of 1e3 .. 1e6) against the closed-form optimum (a
 * product chain composes to a*x / (b + c*x); its marginal a*b / (b + c*x)^2 is solved for the multiplier) gave, as the relative
 * shortfall of total_out, worst / 99th percentile / median of the orders:
 *     1 round 1.8e-2 / 3.9e-3 / 9e-14      2 rounds 1.6e-4 / 1.2e-5 / 9e-14      3 rounds 1.8e-6 / 8.5e-8 / 5e-14
 *     4 rounds 1.6e-7 / 6.4e-10 / 2e-15    5 rounds 1.6e-7 / 8.0e-12 / 2e-16     6 or more 1.6e-7 / 2e-13 / 2e-16
 * The worst case stalls after round 4 for the reason above (8-path orders in which one path carries most of the amount);
 * shares within 4.7e-4 * A of the optimum's for all orders and within 1.0e-6 * A for 99 % of them at 5 rounds (1.5e-7 * A at 6 or
 * more: the optimum is flat, this is sqrt(eps)); |sum of shares - A| <= 3.0e-16 * A.  Beyond what the amounts' precision
 * supports a slice falls below the rounding of the outputs, an increment rounds to 0.0 and the order reports
 * CFMM_SPLIT_SATURATED though the paths could absorb it: one-path orders, whose remainder shrinks 63-fold per round, reach
 * that at 6 rounds; no order of the sample did at 5.
 * Against 80-digit water-filling optima on orders of every pool family, single-family and mixed (tests/test_optimum_precise_cpu.py,
 * profiles/optimum_precise.txt; 56 orders): worst shortfall 6.5e-7 at 5 rounds (an 8-path order of mixed families: the stall
 * above, four times the product chains' 1.6e-7) and 2.4e-10 at 16; median 2e-14 at 5.  A path the optimum leaves empty gets +0.0
 * through 5 rounds; at 16 rounds it can be handed a slice of noise (measured 3.4e-13), at most A*(K/63)^5.
 * The Python default is therefore rounds = 5.
 *   path_amount_in, path_amount_out   [n_paths]
 *   total_out, status                 [count]
 * Everything is checked before anything is enqueued: cfmm_quote_path's checks of the paths; order_first[0] == 0,
 * non-decreasing, order_first[count] == n_paths; 1 .. CFMM_MAX_SPLIT_PATHS paths per order; amount_in[g] finite and >= 0;
 * rounds in 1 .. CFMM_MAX_SPLIT_ROUNDS; no null array; and NO POOL (segment, row) OCCURS TWICE AMONG ALL HOPS OF ONE ORDER'S
 * PATHS -- the paths are quoted independently against the standing market, so a shared pool would be counted twice
 * ("cfmm_split_paths: order 3: paths 0 and 2 share pool (segment 1, row 17)").  A failure is CFMM_ERR_INVALID_ARG, names the
 * order, and the path and hop where there is one, and leaves the outputs untouched.  Synchronous on the context's stream;
 * read-only exactly as cfmm_quote; count == 0 is a no-op; large-market mode needs nothing special; on a context sharded with
 * cfmm_set_peers or RCCL the call is local to the rank.  A MULTI-DEVICE CONTEXT runs the search on the host through
 * cfmm_quote_path's parent path, one call of 64 * n_paths paths per round, with the grid and greedy arithmetic of the kernel:
 * the same bits.
 * Read-only options: under "time_kernels", "split_ns" is the latest call's kernel span (a parent: the sum over its rounds of
 * "quote_ns"); "split_launches" its kernel launches (1; a parent: its cfmm_quote_path calls).  Option "split_max_blocks" (any
 * value >= 1) caps the grid: the same bits either way, a measurement and test switch.
 * OUT OF SCOPE: finding the K candidate paths (cfmm_find_path answers with one; a pool-exclusion mask for it is its own
 * addition); paths that share pools.  EXECUTING the answer: cfmm_swap_order (include/cfmm_amd_order.h) takes order_first, the
 * path arrays and path_amount_in unchanged and executes every order all or nothing across its paths, with one limit on its
 * total; cfmm_swap_path on the order's paths at path_amount_in executes the paths one by one, each all or nothing on its own. */
int cfmm_split_paths(cfmm_ctx* ctx, int64_t count, const int64_t* order_first, const double* amount_in, int64_t n_paths,
                     int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                     const int32_t* hop_coin_in, const int32_t* hop_coin_out, int32_t rounds, double* path_amount_in,
                     double* path_amount_out, double* total_out, int32_t* status);

/* The same on device arrays, asynchronous on the context's stream, single-device contexts only.  Only the scalars (count >= 0,
 * n_paths >= 1 where count > 0, max_hops, rounds) and the null pointers are checked.  An order whose path range is not
 * 1 .. CFMM_MAX_SPLIT_PATHS paths inside 0 .. n_paths, that has a path with n_hops outside 1 .. max_hops or an out-of-range
 * hop, or whose amount is not a valid number, yields CFMM_SPLIT_NAN with NaN total for that order alone; its path outputs are
 * written as NaN where its path range is valid and left untouched otherwise.  Indices are clamped before any read
 * (cfmm_quote_path_dev's rule); neighbouring orders are unaffected.  SHARED POOLS ARE THE CALLER'S RESPONSIBILITY here: they
 * are not looked for, and an order whose paths share a pool is answered as if they did not. */
int cfmm_split_paths_dev(cfmm_ctx* ctx, int64_t count, const int64_t* d_order_first, const double* d_amount_in, int64_t n_paths,
                         int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg, const int64_t* d_hop_row,
                         const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out, int32_t rounds, double* d_path_amount_in,
                         double* d_path_amount_out, double* d_total_out, int32_t* d_status);

#ifdef __cplusplus
}
#endif
#endif
