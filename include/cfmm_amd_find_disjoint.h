/* cfmm_amd_find_disjoint.h -- several swap paths per order that share no pool, found on the device: an addition to cfmm_amd.h
 * (same library, same context, same conventions; include it after or instead of cfmm_amd.h).  The status codes are
 * cfmm_find_path's CFMM_FOUND* of cfmm_amd.h; the limit on max_paths is CFMM_MAX_SPLIT_PATHS of cfmm_amd_split.h, which this
 * header includes. */
#ifndef CFMM_AMD_FIND_DISJOINT_H
#define CFMM_AMD_FIND_DISJOINT_H

#include "cfmm_amd.h"
#include "cfmm_amd_split.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE LINK BETWEEN cfmm_find_path (one path) AND cfmm_split_paths (an order spread over up to 8 paths that share no pool):
 * "I have amount_in of token_in and want token_out -- which routes are there?"  For every query q, up to max_paths
 * (1 .. CFMM_MAX_SPLIT_PATHS) paths from token_in[q] to token_out[q] of at most max_hops (1 .. CFMM_MAX_PATH_HOPS) hops such that
 * NO POOL (segment, row) OCCURS IN TWO OF THEM, in the form cfmm_split_paths, cfmm_quote_path and cfmm_swap_path take.
 * THE CONTRACT IS SUCCESSIVE LAYERED SEARCH WITH A GROWING BAN SET, on the market as it stands on the device:
 *   for round r = 0 .. max_paths-1:
 *     path r of query q is exactly cfmm_find_path's answer for (token_in[q], token_out[q], amount_in[q], max_hops) -- the
 *     LAYERED search, the largest layer entry of token_out, the FEWEST hops that attain it, walked back through the SMALLEST
 *     (segment, row, coin_in, coin_out) that attains each layer entry bit for bit, every hop quoted against the pool as it
 *     stands (include/cfmm_amd.h states it in full) -- on the market WITHOUT every pool that a path of rounds 0 .. r-1 OF THE
 *     SAME QUERY uses.  Such a pool is absent both when the layers are built and when the walk is claimed: a banned pool whose
 *     quote ties a layer entry bit for bit is not a hop.
 * The same amount_in[q] probes every round: the paths are the best ones FOR THAT AMOUNT.  A caller who means to split an
 * amount A over K paths may well probe with A / K, the size a share will have, rather than with A.
 * This is the GREEDY successive-best contract -- the best path, then the best one that avoids it, and so on -- not "the K best
 * paths overall", not node-disjoint paths and not a maximum flow: a first path may use a pool whose absence costs two later ones.
 * What follows from it:
 *   - max_paths == 1 is cfmm_find_path bit for bit, and slot 0 is cfmm_find_path's answer whatever max_paths is.
 *   - cfmm_quote_path on path r at amount_in[q] answers amount_out[r][q] bit for bit: a ban changes which pools are seen, not
 *     how one is quoted.
 *   - amount_out[r+1][q] <= amount_out[r][q]: each round maximises over a subset of the round before.
 *   - The found paths occupy slots 0 .. n_paths[q]-1.  Once a round finds nothing every later one finds nothing (and costs no
 *     quote); those slots carry CFMM_FOUND_NONE, n_hops 0, amount_out 0.0 and hops -1.  n_paths[q] counts the slots whose
 *     status is not CFMM_FOUND_NONE.
 *   - No (segment, row) occurs in two paths of one query.  What a round finds is a WALK, as in cfmm_find_path, and may visit a
 *     pool twice within itself: such a path keeps its slot with CFMM_FOUND_REPEATS (cfmm_split_paths and cfmm_swap_path would
 *     refuse it), its pools are banned like any other's, and the search goes on.
 *   - The answer is a pure function of the market and the query: not of how queries are chunked, of option "find_lds", of how
 *     queries are batched in a call, or of the order atomics arrive in.
 * Indexing: path r of query q lies at r*count + q; hop k of path r at (r*max_hops + k)*count + q -- cfmm_find_path's hop-major
 * layout with one more outer dimension, so slot r alone is a valid set of cfmm_quote_path arrays for all queries.
 *   n_paths                                      [count]
 *   amount_out, n_hops, status                   [max_paths][count]
 *   hop_seg, hop_row, hop_coin_in, hop_coin_out  [max_paths][max_hops][count]
 * cfmm_find_path's checks apply, with its texts ("cfmm_find_disjoint_paths: query 12: token_in 70 out of range ..."), and
 * max_paths outside 1 .. CFMM_MAX_SPLIT_PATHS or a null n_paths are refused too; everything is checked before anything is
 * enqueued, a failure is CFMM_ERR_INVALID_ARG and leaves the outputs untouched.  Read-only exactly as cfmm_quote.  Synchronous on
 * the context's stream (one synchronisation, at the end); count == 0 is a no-op; a context without pools answers CFMM_FOUND_NONE
 * everywhere; large-market mode needs nothing special.  A MULTI-DEVICE CONTEXT answers CFMM_ERR_UNSUPPORTED, as cfmm_find_path.
 * Scratch: cfmm_find_path's layers plus one ban row of ceil(pools / 64) words per query of a chunk, together within 256 MiB
 * (larger calls run in chunks of queries, at least one query each, with the same results).  The read-only options
 * "find_launches", "find_relax_ns", "find_walk_ns" and the per-layer ones describe the latest call of any find entry, summed
 * over the rounds; "find_round_relax_ns_<r>" and "find_round_walk_ns_<r>" (r = 1 .. 8) are this entry's spans round by round.
 * OUT OF SCOPE: a device-pointer variant; executing inside the call (cfmm_split_paths sizes the
 * shares, cfmm_swap_path executes them). */
int cfmm_find_disjoint_paths(cfmm_ctx* ctx, int64_t count, int32_t max_paths, int32_t max_hops, const int32_t* token_in,
                             const int32_t* token_out, const double* amount_in, int32_t* n_paths, double* amount_out,
                             int32_t* n_hops, int32_t* status, int32_t* hop_seg, int64_t* hop_row, int32_t* hop_coin_in,
                             int32_t* hop_coin_out);

#ifdef __cplusplus
}
#endif
#endif
