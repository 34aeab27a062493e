/* cfmm_amd_path_out.h -- the exact-output form of cfmm_swap_path, an addition to cfmm_amd.h (same library, same context,
 * same conventions; include it after or instead of cfmm_amd.h, which it includes).  The status codes are cfmm_swap_out's
 * CFMM_SWAP_* of cfmm_amd.h. */
#ifndef CFMM_AMD_PATH_OUT_H
#define CFMM_AMD_PATH_OUT_H

#include "cfmm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exact-output swap PATHS that MOVE their pools, each path all or nothing: "buy exactly amount_out through A -> B -> C,
 * revert if it costs more than max_amount_in".  The path arguments and checks are cfmm_swap_path's, the refusal of a pool
 * named twice in one path included; the amounts are cfmm_quote_path_out's; max_amount_in (NULL: no limit, else [count],
 * each finite and >= 0), hop_in and status may be NULL.
 * The paths are applied IN QUERY ORDER: path p sees the market as the APPLIED paths among 0 .. p-1 left it.  The path is
 * walked from its last hop to its first: y_H = amount_out[p], y_k = cfmm_quote_out(hop k, y_{k+1}).  For every path, applied
 * or over the limit, amount_in[p] = y_0 and every hop_in[k*count+p] = y_k are, bit for bit, what cfmm_quote_path_out answers
 * on that market.  At each hop the state R_in + γ·y_k, R_out − y_{k+1} -- on UniV3 the price cfmm_swap of y_k rests at -- is
 * tested with cfmm_swap's refusal conditions.  A hop with y_{k+1} == 0 has y_k == +0.0 and moves nothing.  status[p]:
 *   CFMM_SWAP_APPLIED       applied                    amount_in[p] the answer, hop_in the hop amounts
 *   CFMM_SWAP_UNOBTAINABLE  a hop answers +inf         that hop, every earlier hop and amount_in[p] are +inf (cfmm_quote_path_out's rule)
 *   CFMM_SWAP_REFUSED       a hop's state is refused   amount_in[p] NaN; hop_in holds the amounts of the hops behind the
 *                                                      refusing one, NaN from it towards hop 0
 *   CFMM_SWAP_OVER_LIMIT    !(y_0 <= max_amount_in[p]) amount_in[p] the quote it would have cost, hop_in the hop amounts
 * In the last three cases no pool of the path changes a bit.  An applied path then leaves each hop's pool exactly where
 * cfmm_swap_out of (that hop, y_{k+1}) leaves it; UniV3 pools are moved by the host.  The call therefore equals chaining
 * cfmm_swap_out hop by hop (last hop first), path by path, in answers and in final state.  Unused hop_in slots are NaN.
 * "swap_refused" is the number of paths whose status is not CFMM_SWAP_APPLIED.  The call returns CFMM_OK in all four cases.
 * Everything else -- the protocol of a state change, the ordering of paths that share pools, "swap_launches", "swap_ns",
 * CFMM_ERR_UNSUPPORTED on a multi-device context before anything moves -- is cfmm_swap_path's. */
int cfmm_swap_path_out(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                       const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out,
                       const double* amount_out, const double* max_amount_in, double* amount_in, double* hop_in,
                       int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
