// path_checks.h -- internal, host only, HIP-free: the checks of a batch of swap paths (cfmm_quote_path / cfmm_quote_path_out,
// abi_quote_path.cpp) before anything is enqueued.  They take the market as a plain array of {kind, m, n_coins} per segment
// and write the refusal's text into a caller's buffer, so a host program without a device or a context can exercise them
// (tests/native/path_checks_host.cpp).  A refusal names the path AND the hop.
#pragma once

#include "../../include/cfmm_amd.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace cfmm {

struct PathSegInfo {
    int32_t kind;      // CFMM_KIND_*
    int64_t m;         // pools of the segment
    int32_t n_coins;   // coins per pool (2 for the two-coin kinds and UniV3)
};

// the scalars both the host-pointer and the device-pointer entries check
inline int check_path_scalars(const char* who, int64_t count, int32_t max_hops, char* msg, size_t len)
{
    if (count < 0) {
        std::snprintf(msg, len, "%s: count must be >= 0", who);
        return CFMM_ERR_INVALID_ARG;
    }
    if (max_hops < 1 || max_hops > CFMM_MAX_PATH_HOPS) {
        std::snprintf(msg, len, "%s: max_hops must be 1 .. %d (got %d)", who, CFMM_MAX_PATH_HOPS, (int)max_hops);
        return CFMM_ERR_INVALID_ARG;
    }
    return CFMM_OK;
}

// Every path of a host-pointer call.  The hop arrays are hop-major: hop k of path p at k*count + p; slots at k >= n_hops[p]
// are not looked at.  exact_out: the given amount is the wanted output (it enters at the path's LAST hop), else the input.
inline int check_paths(const char* who, bool exact_out, const PathSegInfo* segs, int64_t nseg, int64_t count,
                       int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                       const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* given, char* msg, size_t len)
{
    const int rc = check_path_scalars(who, count, max_hops, msg, len);
    if (rc != CFMM_OK) return rc;
    if (count > 0 && (!n_hops || !hop_seg || !hop_row || !hop_coin_in || !hop_coin_out || !given)) {
        std::snprintf(msg, len, "%s: null path array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    for (int64_t p = 0; p < count; ++p) {
        const int nh = n_hops[p];
        if (nh < 1 || nh > max_hops) {
            std::snprintf(msg, len, "%s: path %lld: n_hops %d out of range (1 .. %d)", who, (long long)p, nh, (int)max_hops);
            return CFMM_ERR_INVALID_ARG;
        }
        for (int k = 0; k < nh; ++k) {
            const int64_t at = (int64_t)k * count + p;
            const int32_t seg = hop_seg[at];
            if (seg < 0 || seg >= nseg) {
                std::snprintf(msg, len, "%s: path %lld, hop %d: segment %d out of range (the context has %lld)", who, (long long)p,
                              k, (int)seg, (long long)nseg);
                return CFMM_ERR_INVALID_ARG;
            }
            const PathSegInfo& s = segs[seg];
            const int64_t row = hop_row[at];
            if (row < 0 || row >= s.m) {
                std::snprintf(msg, len, "%s: path %lld, hop %d: row %lld out of range (segment %d has %lld pools)", who,
                              (long long)p, k, (long long)row, (int)seg, (long long)s.m);
                return CFMM_ERR_INVALID_ARG;
            }
            const int ci = hop_coin_in[at], co = hop_coin_out[at];
            if (ci < 0 || ci >= s.n_coins) {
                std::snprintf(msg, len, "%s: path %lld, hop %d: coin_in %d out of range (pool has %d coins)", who, (long long)p, k,
                              ci, (int)s.n_coins);
                return CFMM_ERR_INVALID_ARG;
            }
            if (co < 0 || co >= s.n_coins) {
                std::snprintf(msg, len, "%s: path %lld, hop %d: coin_out %d out of range (pool has %d coins)", who, (long long)p,
                              k, co, (int)s.n_coins);
                return CFMM_ERR_INVALID_ARG;
            }
            if (ci == co) {
                std::snprintf(msg, len, "%s: path %lld, hop %d: coin_in and coin_out are both %d", who, (long long)p, k, ci);
                return CFMM_ERR_INVALID_ARG;
            }
        }
        if (!(given[p] >= 0.0) || !std::isfinite(given[p])) {
            std::snprintf(msg, len, "%s: path %lld, hop %d: %s must be finite and >= 0", who, (long long)p,
                          exact_out ? nh - 1 : 0, exact_out ? "amount_out" : "amount_in");
            return CFMM_ERR_INVALID_ARG;
        }
    }
    return CFMM_OK;
}

} // namespace cfmm
