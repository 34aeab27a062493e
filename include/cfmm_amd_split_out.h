/* cfmm_amd_split_out.h -- buying an exact amount through several swap paths on the device: the exact-output twin of
 * cfmm_amd_split.h, which it includes (same library, same context, same conventions). */
#ifndef CFMM_AMD_SPLIT_OUT_H
#define CFMM_AMD_SPLIT_OUT_H

#include "cfmm_amd_split.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CFMM_SPLIT_UNOBTAINABLE 4    /* a greedy step found no path that can give another slice: total_in and the order's
                                        path_amount_in are +inf, its path_amount_out +0.0 */

/* HOW MUCH OF A WANTED AMOUNT COMES OUT OF EACH PATH: "I want B of token Y and have these K routes from X; how much do I buy
 * through each?" -- cfmm_split_paths with the direction turned.  CFMM_SPLIT_POINTS, CFMM_MAX_SPLIT_PATHS,
 * CFMM_MAX_SPLIT_ROUNDS, the CFMM_SPLIT_* codes and the argument order (order_first, the hop-major path arrays, rounds) are
 * cfmm_split_paths'.  Order g owns the paths order_first[g] .. order_first[g+1] - 1 -- K of them, 1 <= K <=
 * CFMM_MAX_SPLIT_PATHS, all ending in the same token -- and wants B = amount_out[g] of that token.
 * THE CONTRACT IS THE SEARCH, on the market as it stands on the device, every operation rounded on its own (no fused
 * multiply-add).  The grid is cfmm_split_paths' grid, laid over the output:
 *   base_k = 0 (k = 0 .. K-1);  rem = B
 *   for round r = 1 .. rounds:
 *     s = rem / 63.0
 *     x[k][j] = base_k + s * j  (j = 0 .. 62: the product, then the sum);  x[k][63] = base_k + rem
 *     c[k][j] = quote_path_out(path k, x[k][j]), with cfmm_quote_path_out's own per-hop forms from the last hop to the first,
 *       EVERY HOP QUOTED AGAINST THE POOL AS IT STANDS; +inf where the path cannot give that much (and then no earlier hop is
 *       evaluated);
 *     n_k = 0;  63 times:
 *       d_k = c[k][n_k + 1] - c[k][n_k]
 *       k* = the smallest k whose d_k is the SMALLEST, compared as numbers (+0.0 == -0.0, and +inf is a number); a NaN loses
 *       to every number;  n_{k*} += 1
 *     if r < rounds:  m_k = max(n_k - 1, 0);  base_k = x[k][m_k];
 *                     rem = max(B - (base_0 + base_1 + ... in increasing k), 0.0)
 *   path_amount_out[k] = x[k][n_k],  path_amount_in[k] = c[k][n_k]  (of the last round);
 *   total_in = c_0 + c_1 + ... in increasing k.
 * STATUS.  The FIRST step, in round and step order, whose taken increment d_{k*} is not finite decides a failure:
 *     CFMM_SPLIT_UNOBTAINABLE  it is an infinity: the cheapest next slice of every path costs +inf, no path can give another
 *                              slice.  total_in and the order's path_amount_in are +inf, its path_amount_out +0.0
 *     CFMM_SPLIT_NAN           it is no number (no d_k was one), or no step was bad and total_in is no number (a path that
 *                              quotes NaN everywhere receives no slice, but its cost is NaN): every output of the order NaN
 *     CFMM_SPLIT_NONE          no bad step, and B == 0: every output +0.0
 *     CFMM_SPLIT_OK            otherwise
 * Why the first: the path that takes a +inf step stands at c = +inf from then on, its next increment is inf - inf, no number,
 * and what the later steps of the order compare says nothing about the paths.  They still run -- the instructions do not
 * depend on the data -- and do not count.  There is no SATURATED here: an increment of 0 is a free slice, not a failure.
 * The same greedy with scaling as cfmm_split_paths: every pool family's exact-output cost is convex and non-decreasing up to
 * the pool's capacity and +inf beyond, and so is a path's; the cheapest-increment greedy is optimal for such costs on each
 * round's grid, and the step back leaves at most K slices for the next round.  THE CONTRACT IS THE SEARCH, not "the global
 * optimum".
 * So the answer is a pure function of the market, the order and `rounds` -- not of launch geometry (option
 * "split_max_blocks") or of how orders are batched.  With K = 1 the single share is B bit for bit.  On a CFMM_SPLIT_OK order
 * cfmm_quote_path_out on path k at path_amount_out[k] answers path_amount_in[k] bit for bit, and the shares sum to B to the
 * rounding of their sum.
 * WHAT UNOBTAINABLE MEANS, AND DOES NOT.  It is the search's verdict on its grid, not a theorem about the paths.  In round 1
 * a path takes only whole slices of B/63: path k can hold floor(cap_k / (B/63)) of them where cap_k is what it can give, so
 * round 1 hands out all 63 whenever sum_k (cap_k * 63/B - 1) >= 63, that is whenever the paths jointly give at least
 * B * (1 + K/63).  An order whose paths jointly give less than that may be refused though a finer allocation exists.  Later
 * rounds are not covered by that derivation (the slices are finer, but a share never goes below its restart point); what they
 * do was measured, below.
 * What the search finds.  A numpy run of this contract on 4000 random orders (tests/test_split_paths_out_cpu.py: K = 1 .. 8
 * ProductTwoCoin chains of 1 .. 3 hops; a product chain composes to out = a*x / (b + c*x), so buying y through it costs
 * b*y / (a - c*y) up to the capacity a/c, with marginal a*b / (a - c*y)^2, solved for the multiplier by bisection; B drawn
 * from 0.003 to 3 times the joint capacity) gave, on the orders below the joint capacity that every round count answers
 * CFMM_SPLIT_OK, as the relative EXCESS of total_in over the optimum, worst / 99th percentile / median:
 *     1 round 6.5 / 1.9e-1 / 1e-16          2 rounds 4.0e-1 / 2.6e-3 / 1e-16      3 rounds 4.0e-1 / 1.1e-4 / 1e-16
 *     4 rounds 4.0e-1 / 1.5e-6 / 1e-16      5 rounds 4.0e-1 / 1.5e-8 / 0          6 rounds 4.0e-1 / 1.4e-10 / 0
 * THE WORST CASE STALLS after round 2, and it is large: it belongs to orders within a few per cent of their joint capacity,
 * where a path's cost b*y / (a - c*y) is steep without bound, so the slice by which round 1 overfills a path (a share never
 * goes below its restart point: cfmm_amd_split.h says why that is up to K-1 slices) costs a multiple of the optimum.  On the
 * orders whose paths jointly give at least 2 B the worst excess is 4.8e-2, 4.5e-4, 2.7e-4 after 1, 2, 3 rounds and 2.7e-4 from
 * then on.  Shares within 2.4e-2 * B of the optimum's for all orders and within 1.2e-6 * B for 99 % of them at 5 rounds;
 * |sum of shares - B| <= 3.2e-16 * B at every round count.
 * The grid-feasibility limit, measured: of the 3347 orders of the sample below their joint capacity 18 were reported
 * CFMM_SPLIT_UNOBTAINABLE, every one of them in round 1 and the same 18 at every round count 1 .. 8 (no later round refused an
 * order that round 1 had served); the largest joint capacity / B among them was 1.0581, which is 0.9698 of that order's
 * 1 + K/63, and no order above 1.0581 was refused; the smallest joint capacity / B of a served order was 1.0092.
 * The Python default is rounds = 5, as cfmm_split_paths'.
 *   path_amount_out, path_amount_in   [n_paths]
 *   total_in, status                  [count]
 * Everything is checked before anything is enqueued, with cfmm_split_paths' checks and texts under this entry's name:
 * cfmm_quote_path's checks of the paths; order_first[0] == 0, non-decreasing, order_first[count] == n_paths; 1 ..
 * CFMM_MAX_SPLIT_PATHS paths per order; amount_out[g] finite and >= 0; rounds in 1 .. CFMM_MAX_SPLIT_ROUNDS; no null array;
 * and NO POOL (segment, row) OCCURS TWICE AMONG ALL HOPS OF ONE ORDER'S PATHS ("cfmm_split_paths_out: order 3: paths 0 and 2
 * share pool (segment 1, row 17)").  A failure is CFMM_ERR_INVALID_ARG, names the order, and the path and hop where there is
 * one, and leaves the outputs untouched.  Synchronous on the context's stream; read-only exactly as cfmm_quote; count == 0 is
 * a no-op; large-market mode needs nothing special; on a context sharded with cfmm_set_peers or RCCL the call is local to the
 * rank.  A MULTI-DEVICE CONTEXT runs the search on the host through cfmm_quote_path_out's parent path, one call of
 * 64 * n_paths paths per round, with the grid and greedy arithmetic of the kernel: the same bits.
 * Options: "split_max_blocks" caps this entry's grid too (the same bits either way); "split_ns" and "split_launches" describe
 * the latest call of EITHER split entry.
 * Executing: cfmm_swap_order_out (include/cfmm_amd_order.h) takes order_first, the path arrays and path_amount_out unchanged and
 * buys every order all or nothing across its paths, with one limit on its total cost; cfmm_swap_path_out on the order's paths at
 * path_amount_out, with path_amount_in as the limits, buys the paths one by one, each all or nothing on its own.
 * OUT OF SCOPE: paths that share pools. */
int cfmm_split_paths_out(cfmm_ctx* ctx, int64_t count, const int64_t* order_first, const double* amount_out, int64_t n_paths,
                         int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                         const int32_t* hop_coin_in, const int32_t* hop_coin_out, int32_t rounds, double* path_amount_out,
                         double* path_amount_in, double* total_in, int32_t* status);

/* The same on device arrays, asynchronous on the context's stream, single-device contexts only: cfmm_split_paths_dev's rule.
 * Only the scalars (count >= 0, n_paths >= 1 where count > 0, max_hops, rounds) and the null pointers are checked.  An order
 * whose path range is not 1 .. CFMM_MAX_SPLIT_PATHS paths inside 0 .. n_paths, that has a path with n_hops outside
 * 1 .. max_hops or an out-of-range hop, or whose amount is not a valid number, yields CFMM_SPLIT_NAN with NaN total for that
 * order alone; its path outputs are written as NaN where its path range is valid and left untouched otherwise.  Indices are
 * clamped before any read; neighbouring orders are unaffected.  SHARED POOLS ARE THE CALLER'S RESPONSIBILITY here. */
int cfmm_split_paths_out_dev(cfmm_ctx* ctx, int64_t count, const int64_t* d_order_first, const double* d_amount_out,
                             int64_t n_paths, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                             const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                             int32_t rounds, double* d_path_amount_out, double* d_path_amount_in, double* d_total_in,
                             int32_t* d_status);

#ifdef __cplusplus
}
#endif
#endif
