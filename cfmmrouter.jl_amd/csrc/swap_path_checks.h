// swap_path_checks.h -- internal, host only, HIP-free: what cfmm_swap_path (abi_swap_path.cpp) checks beyond check_paths
// (path_checks.h), before anything is enqueued.  A path may name a pool (segment, row) only once -- the rule that lets a lane
// quote the whole path against the market as it stands and apply it afterwards -- and a limit, where one is given, is
// finite and >= 0.  Same conventions as path_checks.h: the refusal's text goes to a caller's buffer and names the path and
// the hops, so tests/native/swap_path_host.cpp can exercise them without a device.  To be called on paths that check_paths
// has accepted.
#pragma once

#include "../../include/cfmm_amd.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace cfmm {

inline int check_swap_paths(const char* who, int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                            const double* min_amount_out, char* msg, size_t len)
{
    for (int64_t p = 0; p < count; ++p) {
        const int nh = n_hops[p];
        for (int k = 1; k < nh; ++k)   // (at most 28 pairs)
            for (int j = 0; j < k; ++j) {
                const int64_t a = (int64_t)j * count + p, b = (int64_t)k * count + p;
                if (hop_seg[a] == hop_seg[b] && hop_row[a] == hop_row[b]) {
                    std::snprintf(msg, len, "%s: path %lld, hops %d and %d: row %lld of segment %d appears twice (a pool may appear only once in a path)",
                                  who, (long long)p, j, k, (long long)hop_row[a], (int)hop_seg[a]);
                    return CFMM_ERR_INVALID_ARG;
                }
            }
        if (min_amount_out && (!(min_amount_out[p] >= 0.0) || !std::isfinite(min_amount_out[p]))) {
            std::snprintf(msg, len, "%s: path %lld, hop %d: min_amount_out must be finite and >= 0", who, (long long)p, nh - 1);
            return CFMM_ERR_INVALID_ARG;
        }
    }
    return CFMM_OK;
}

} // namespace cfmm
