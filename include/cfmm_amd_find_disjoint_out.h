/* cfmm_amd_find_disjoint_out.h -- several swap paths per order that share no pool, found on the device FOR A WANTED OUTPUT: the
 * exact-output twin of cfmm_amd_find_disjoint.h, which it includes (same library, same context, same conventions).  The status
 * codes are cfmm_find_path's CFMM_FOUND*; the limit on max_paths is CFMM_MAX_SPLIT_PATHS. */
#ifndef CFMM_AMD_FIND_DISJOINT_OUT_H
#define CFMM_AMD_FIND_DISJOINT_OUT_H

#include "cfmm_amd_find_disjoint.h"
#include "cfmm_amd_find_out.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE LINK BETWEEN cfmm_find_path_out (one path) AND cfmm_split_paths_out (a wanted amount bought through up to 8 paths that
 * share no pool): "I want amount_out of token_out and pay in token_in -- which routes are there?"  cfmm_find_disjoint_paths'
 * contract with the direction turned.  For every query q, up to max_paths (1 .. CFMM_MAX_SPLIT_PATHS) paths from token_in[q]
 * to token_out[q] of at most max_hops hops such that NO POOL (segment, row) OCCURS IN TWO OF THEM, in the form
 * cfmm_split_paths_out, cfmm_quote_path_out and cfmm_swap_path_out take:
 *   for round r = 0 .. max_paths-1:
 *     path r of query q is exactly cfmm_find_path_out's answer for (token_in[q], token_out[q], amount_out[q], max_hops) -- the
 *     LAYERED search backwards from token_out, the SMALLEST layer entry of token_in, the FEWEST hops that attain it, walked
 *     FORWARD from token_in through the SMALLEST (segment, row, coin_in, coin_out) that attains each layer entry bit for bit,
 *     every hop quoted against the pool as it stands (include/cfmm_amd_find_out.h states it in full) -- on the market WITHOUT
 *     every pool that a path of rounds 0 .. r-1 OF THE SAME QUERY uses.  Such a pool is absent both when the layers are built
 *     and when the walk is claimed.
 * The same amount_out[q] probes every round.  A path that cannot give amount_out[q] alone is never found: a caller who means
 * to buy B through K paths should probe with about B / K, the size a share will have, not with B -- with B the very order
 * that needs splitting finds nothing.
 * The GREEDY successive-best contract, as cfmm_find_disjoint_paths'.  What follows from it:
 *   - max_paths == 1 is cfmm_find_path_out bit for bit, and slot 0 is cfmm_find_path_out's answer whatever max_paths is.
 *   - cfmm_quote_path_out on path r at amount_out[q] answers amount_in[r][q] bit for bit.
 *   - amount_in[r+1][q] >= amount_in[r][q]: each round minimises over a subset of the round before.
 *   - The found paths occupy slots 0 .. n_paths[q]-1; the others carry CFMM_FOUND_NONE, n_hops 0, hops -1 and
 *     cfmm_find_path_out's none value: +inf, or +0.0 where amount_out[q] is 0.
 *   - No (segment, row) occurs in two paths of one query; a walk that visits a pool twice within itself keeps its slot with
 *     CFMM_FOUND_REPEATS and its pools are banned like any other's.
 *   - The answer is a pure function of the market and the query: not of chunking, of option "find_lds" or of batching.
 * Indexing, layout, checks (with this entry's name: "cfmm_find_disjoint_paths_out: query 12: amount_out must be ..."), scratch
 * bound and options are cfmm_find_disjoint_paths'.  Read-only.  Synchronous on the context's stream; count == 0 is a no-op; a
 * context without pools answers CFMM_FOUND_NONE everywhere; A MULTI-DEVICE CONTEXT answers CFMM_ERR_UNSUPPORTED.
 *   n_paths                                      [count]
 *   amount_in, n_hops, status                    [max_paths][count]
 *   hop_seg, hop_row, hop_coin_in, hop_coin_out  [max_paths][max_hops][count]
 * OUT OF SCOPE: a device-pointer variant; executing inside the call (cfmm_split_paths_out sizes the shares,
 * cfmm_swap_path_out executes them). */
int cfmm_find_disjoint_paths_out(cfmm_ctx* ctx, int64_t count, int32_t max_paths, int32_t max_hops, const int32_t* token_in,
                                 const int32_t* token_out, const double* amount_out, int32_t* n_paths, double* amount_in,
                                 int32_t* n_hops, int32_t* status, int32_t* hop_seg, int64_t* hop_row, int32_t* hop_coin_in,
                                 int32_t* hop_coin_out);

#ifdef __cplusplus
}
#endif
#endif
