// find_checks.h -- internal, host only, HIP-free: the checks of a batch of cfmm_find_path queries before anything is enqueued,
// and the rule that cuts a call into chunks of queries (abi_find_path.cpp).  Like path_checks.h they take plain arrays and
// write the refusal's text into a caller's buffer, so a host program without a device or a context can exercise them
// (tests/native/find_checks_host.cpp, find_disjoint_checks_host.cpp).  A refusal names the QUERY.  cfmm_find_path_out takes the same checks: its given amount
// arrives as `amount_in` and is called by the name passed as `amount` ("amount_out") in the refusal.
#pragma once

#include "../../include/cfmm_amd.h"
#include "../../include/cfmm_amd_split.h"   // CFMM_MAX_SPLIT_PATHS: the limit on cfmm_find_disjoint_paths' max_paths

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace cfmm {

// The layers of one chunk, (max_hops + 1) x queries x n_tokens words of 8 bytes, stay within this budget: a design choice --
// the size of the Infinity Cache, so that a layer that is being relaxed and the one it is relaxed from can stay on chip.
// Results do not depend on it.
constexpr int64_t kFindScratchBudget = 256ll << 20;
// queries of one chunk beyond which no budget asks to go: gridDim.y of the per-pool launches is 65535 rows of 64 queries
constexpr int64_t kFindMaxChunk = 1 << 20;

// queries per chunk for a market of n_tokens: as many as the budget holds, at least one (a single query of a market whose
// layers exceed the budget still runs, over the budget)
inline int64_t find_chunk_queries(int64_t n_tokens, int32_t max_hops, int64_t budget = kFindScratchBudget)
{
    const int64_t per_query = (int64_t)(max_hops + 1) * (n_tokens < 1 ? 1 : n_tokens) * 8;
    const int64_t fit = budget / per_query;
    return fit < 1 ? 1 : (fit > kFindMaxChunk ? kFindMaxChunk : fit);
}

inline int check_find(const char* who, int64_t n_tokens, int64_t count, int32_t max_hops, const int32_t* token_in,
                      const int32_t* token_out, const double* amount_in, const void* amount_out, const void* n_hops, const void* hop_seg,
                      const void* hop_row, const void* hop_coin_in, const void* hop_coin_out, const void* status, char* msg, size_t len,
                      const char* amount = "amount_in")
{
    if (count < 0) {
        std::snprintf(msg, len, "%s: count must be >= 0", who);
        return CFMM_ERR_INVALID_ARG;
    }
    if (max_hops < 1 || max_hops > CFMM_MAX_PATH_HOPS) {
        std::snprintf(msg, len, "%s: max_hops must be 1 .. %d (got %d)", who, CFMM_MAX_PATH_HOPS, (int)max_hops);
        return CFMM_ERR_INVALID_ARG;
    }
    if (count == 0) return CFMM_OK;
    if (!token_in || !token_out || !amount_in || !amount_out || !n_hops || !hop_seg || !hop_row || !hop_coin_in || !hop_coin_out || !status) {
        std::snprintf(msg, len, "%s: null query array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    for (int64_t q = 0; q < count; ++q) {
        if (token_in[q] < 0 || token_in[q] >= n_tokens) {
            std::snprintf(msg, len, "%s: query %lld: token_in %d out of range (the market has %lld tokens)", who, (long long)q,
                          (int)token_in[q], (long long)n_tokens);
            return CFMM_ERR_INVALID_ARG;
        }
        if (token_out[q] < 0 || token_out[q] >= n_tokens) {
            std::snprintf(msg, len, "%s: query %lld: token_out %d out of range (the market has %lld tokens)", who, (long long)q,
                          (int)token_out[q], (long long)n_tokens);
            return CFMM_ERR_INVALID_ARG;
        }
        if (!(amount_in[q] >= 0.0) || !std::isfinite(amount_in[q])) {
            std::snprintf(msg, len, "%s: query %lld: %s must be finite and >= 0", who, (long long)q, amount);
            return CFMM_ERR_INVALID_ARG;
        }
    }
    return CFMM_OK;
}

// ---- cfmm_find_disjoint_paths (include/cfmm_amd_find_disjoint.h) ----
// words of one query's ban row: one bit per pool of the market
inline int64_t find_ban_words(int64_t pools) { return pools < 1 ? 1 : (pools + 63) / 64; }

// find_chunk_queries with the ban row: the layers PLUS the ban row of one query within the same budget, at least one query
inline int64_t find_disjoint_chunk_queries(int64_t n_tokens, int32_t max_hops, int64_t pools, int64_t budget = kFindScratchBudget)
{
    const int64_t per_query = ((int64_t)(max_hops + 1) * (n_tokens < 1 ? 1 : n_tokens) + find_ban_words(pools)) * 8;
    const int64_t fit = budget / per_query;
    return fit < 1 ? 1 : (fit > kFindMaxChunk ? kFindMaxChunk : fit);
}

// check_find's checks and texts under the new entry's name, with max_paths in front of max_hops; a null n_paths is refused with
// the other null arrays (it takes status's place in check_find's test)
inline int check_find_disjoint(const char* who, int64_t n_tokens, int64_t count, int32_t max_paths, int32_t max_hops,
                               const int32_t* token_in, const int32_t* token_out, const double* amount_in, const void* n_paths,
                               const void* amount_out, const void* n_hops, const void* status, const void* hop_seg, const void* hop_row,
                               const void* hop_coin_in, const void* hop_coin_out, char* msg, size_t len, const char* amount = "amount_in")
{
    if (count >= 0 && (max_paths < 1 || max_paths > CFMM_MAX_SPLIT_PATHS)) {
        std::snprintf(msg, len, "%s: max_paths must be 1 .. %d (got %d)", who, CFMM_MAX_SPLIT_PATHS, (int)max_paths);
        return CFMM_ERR_INVALID_ARG;
    }
    return check_find(who, n_tokens, count, max_hops, token_in, token_out, amount_in, amount_out, n_hops, hop_seg, hop_row, hop_coin_in,
                      hop_coin_out, count > 0 && !n_paths ? nullptr : status, msg, len, amount);
}

} // namespace cfmm
