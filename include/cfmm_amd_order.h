/* cfmm_amd_order.h -- executing split orders on the device, each order all or nothing ACROSS its paths: the last link of
 * find -> split -> execute, in both directions.  Same library, same context, same conventions as cfmm_amd.h; the orders are
 * cfmm_amd_split.h's (which this header includes through cfmm_amd_split_out.h), the paths cfmm_swap_path's. */
#ifndef CFMM_AMD_ORDER_H
#define CFMM_AMD_ORDER_H

#include "cfmm_amd_path_out.h"
#include "cfmm_amd_split_out.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status[g] of an order */
#define CFMM_ORDER_APPLIED 0         /* every path of the order moved its pools */
#define CFMM_ORDER_LIMIT 1           /* the total misses the order's limit: nothing moved, the total is the sum */
#define CFMM_ORDER_REFUSED 2         /* some path has a refusing hop: nothing moved, the total is NaN */
#define CFMM_ORDER_UNOBTAINABLE 3    /* exact output only: some path answers +inf: nothing moved, the total is +inf */
/* path_status[p]: CFMM_PATH_APPLIED, CFMM_PATH_REFUSED, CFMM_SWAP_UNOBTAINABLE of cfmm_amd.h, or */
#define CFMM_ORDER_PATH_HELD 4       /* the path itself passes, but its order was not applied */

/* EXECUTE ORDERS, EACH OVER ITS 1 .. CFMM_MAX_SPLIT_PATHS PATHS, ALL OR NOTHING PER ORDER, ONE LIMIT ON THE ORDER'S TOTAL.
 * The paths are cfmm_swap_path's hop-major arrays for n_paths paths (hop k of path p at k*n_paths + p), order_first is
 * cfmm_split_paths': order g owns the paths order_first[g] .. order_first[g+1] - 1.  What cfmm_split_paths returned --
 * path_amount_in beside the arrays it was given -- can be passed in unchanged.
 * THE CONTRACT IS THE SERIAL EXECUTION.  For g = 0 .. count-1, in this order, on the market as the applied orders before g
 * left it:
 *   1. every path k of the order is walked as cfmm_swap_path walks it before it applies anything: the amounts carry
 *      cfmm_quote_path's bits, the refusal tests are cfmm_swap's.  path_amount_out[p] and hop_out are written exactly as
 *      cfmm_swap_path writes them for a path that is below its limit or refused (NaN from a refusing hop on);
 *   2. total = y_0 + y_1 + ... in increasing k, the first term taken as it is -- the sum cfmm_split_paths forms, so on an
 *      unmoved market total_out[g] is cfmm_split_paths' total_out bit for bit;
 *   3. the status, with the precedence refused > unobtainable > limit:
 *        CFMM_ORDER_REFUSED       some path has a refusing hop; total_out[g] is NaN
 *        CFMM_ORDER_LIMIT         !(total >= min_total_out[g]); total_out[g] is the sum
 *        CFMM_ORDER_APPLIED       otherwise
 *   4. only an APPLIED order moves anything: every hop of every one of its paths leaves its pool exactly where
 *      cfmm_swap_path leaves it.  A hop that carries 0 moves no bit.
 * path_status[p] (optional): CFMM_PATH_APPLIED the path moved; CFMM_PATH_REFUSED this path refuses; CFMM_ORDER_PATH_HELD the
 * path itself passes, but its order was not applied.
 *   path_amount_in, path_amount_out, path_status   [n_paths]
 *   min_total_out (or NULL: no limit), total_out, status   [count]
 *   hop_out   [max_hops][n_paths], or NULL
 * Everything is checked before anything is enqueued: cfmm_swap_path's checks of the paths (a pool at most once in a path,
 * amounts finite and >= 0), cfmm_split_paths' checks of order_first (order_first[0] == 0, non-decreasing,
 * order_first[count] == n_paths, 1 .. CFMM_MAX_SPLIT_PATHS paths per order), min_total_out[g] finite and >= 0, and NO POOL
 * (segment, row) OCCURS TWICE AMONG ALL HOPS OF ONE ORDER'S PATHS ("cfmm_swap_order: order 1: paths 0 and 2 share pool
 * (segment 1, row 17)"): inside an order the paths are walked against one market, so a shared pool would be counted twice.
 * A failure is CFMM_ERR_INVALID_ARG, names the order, and the path (numbered within the order) and hop where there is one,
 * and moves nothing.
 * How it runs: the host cuts the batch into waves of orders that share no pool (an order's wave is the first in which all
 * its pools are free; AN ORDER THAT TURNS OUT NOT TO BE APPLIED STILL HOLDS ITS POOLS FOR ITS WAVE), uploads everything once
 * in wave order and launches one kernel per wave, eight lanes per order.  It waits between waves only behind a wave with a
 * UniV3 hop, whose pools (of applied orders only) move through cfmm_pools_set_prices' apply path.  A batch of pool-disjoint
 * orders is one launch.
 * LIMITS.  Host pointers only.  Single-device contexts only: a multi-device context answers CFMM_ERR_UNSUPPORTED before
 * anything moves.  An order's paths share no pool; at most CFMM_MAX_SPLIT_PATHS paths per order.  count == 0 is a no-op that
 * invalidates nothing.  Otherwise a state change as cfmm_swap_path: the trades on the device are invalidated, an armed route
 * is cancelled.
 * Options: "swap_refused" the orders of the latest call that were not applied, "swap_launches" its waves, "swap_ns" (under
 * "time_kernels") the sum of its kernel spans; read-write "order_max_blocks" (>= 1) caps the grid, a test and measurement
 * switch like "split_max_blocks": the same bits either way.
 * OUT OF SCOPE: orders whose own paths share pools; all-or-nothing across devices; a device-pointer form; per-path limits
 * inside an order; partial fills. */
int cfmm_swap_order(cfmm_ctx* ctx, int64_t count, const int64_t* order_first, int64_t n_paths, int32_t max_hops,
                    const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
                    const int32_t* hop_coin_out, const double* path_amount_in, const double* min_total_out,
                    double* path_amount_out, double* hop_out, double* total_out, int32_t* path_status, int32_t* status);

/* The exact-output twin: what cfmm_split_paths_out returned, executed.  path_amount_out[p] is wanted from path p's LAST hop;
 * every path is walked as cfmm_swap_path_out walks it (cfmm_quote_path_out's bits from the last hop to the first; a refusing
 * hop writes NaN from itself towards hop 0, a hop that cannot give that much +inf); path_amount_in[p] is what path p asks
 * for and hop_in[k] the amount to tender to hop k; total = the sum of the path inputs in increasing k, cfmm_split_paths_out's
 * total_in bit for bit on an unmoved market.  Status, refused > unobtainable > limit:
 *     CFMM_ORDER_REFUSED        some path has a refusing hop; total_in[g] is NaN
 *     CFMM_ORDER_UNOBTAINABLE   some path answers +inf; total_in[g] is +inf
 *     CFMM_ORDER_LIMIT          !(total <= max_total_in[g]); total_in[g] is the sum
 *     CFMM_ORDER_APPLIED        otherwise: every hop leaves its pool where cfmm_swap_path_out leaves it
 * path_status[p] may also be CFMM_SWAP_UNOBTAINABLE: this path cannot give the amount.  Everything else is cfmm_swap_order's. */
int cfmm_swap_order_out(cfmm_ctx* ctx, int64_t count, const int64_t* order_first, int64_t n_paths, int32_t max_hops,
                        const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
                        const int32_t* hop_coin_out, const double* path_amount_out, const double* max_total_in,
                        double* path_amount_in, double* hop_in, double* total_in, int32_t* path_status, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
