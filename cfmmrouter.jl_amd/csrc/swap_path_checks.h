// swap_path_checks.h -- internal, host only, HIP-free: what cfmm_swap_path and cfmm_swap_path_out (abi_swap_path.cpp; exact_out:
// the limit is max_amount_in, on the first hop's input) check beyond check_paths
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
                            const double* limit, char* msg, size_t len, bool exact_out = false)
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
        if (limit && (!(limit[p] >= 0.0) || !std::isfinite(limit[p]))) {   // (named at the hop the limited amount belongs to)
            std::snprintf(msg, len, "%s: path %lld, hop %d: %s must be finite and >= 0", who, (long long)p, exact_out ? 0 : nh - 1,
                          exact_out ? "max_amount_in" : "min_amount_out");
            return CFMM_ERR_INVALID_ARG;
        }
    }
    return CFMM_OK;
}

} // namespace cfmm
