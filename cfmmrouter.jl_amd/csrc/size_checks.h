// size_checks.h -- internal, host only, HIP-free: the checks of cfmm_size_path / cfmm_size_path_dev (abi_size_path.cpp) beyond
// those of the paths themselves, which stay path_checks.h's check_paths: the scalars, the limits and the values.  As there,
// a refusal's text goes into a caller's buffer, so a host program without a device or a context can exercise them
// (tests/native/size_checks_host.cpp).  A refusal of a path names the path AND the hop its amount enters (hop 0).
#pragma once

#include "path_checks.h"
#include "size_grid.h"

namespace cfmm {

// the scalars both entries check
inline int check_size_scalars(const char* who, int64_t count, int32_t max_hops, int32_t rounds, char* msg, size_t len)
{
    const int rc = check_path_scalars(who, count, max_hops, msg, len);
    if (rc != CFMM_OK) return rc;
    if (rounds < 1 || rounds > CFMM_MAX_SIZE_ROUNDS) {
        std::snprintf(msg, len, "%s: rounds must be 1 .. %d (got %d)", who, CFMM_MAX_SIZE_ROUNDS, (int)rounds);
        return CFMM_ERR_INVALID_ARG;
    }
    return CFMM_OK;
}

// ... and the arrays neither entry accepts null when there are paths (value_in / value_out may be null: 1.0)
inline int check_size_arrays(const char* who, int64_t count, const void* max_amount_in, const void* amount_in, const void* amount_out,
                             const void* gain, const void* status, char* msg, size_t len)
{
    if (count > 0 && (!max_amount_in || !amount_in || !amount_out || !gain || !status)) {
        std::snprintf(msg, len, "%s: null path array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    return CFMM_OK;
}

// every path's limit and values of a host-pointer call (the arrays are known not to be null where they must not be)
inline int check_size_amounts(const char* who, int64_t count, const double* max_amount_in, const double* value_in,
                              const double* value_out, char* msg, size_t len)
{
    for (int64_t p = 0; p < count; ++p) {
        if (!size_limit_ok(max_amount_in[p])) {
            std::snprintf(msg, len, "%s: path %lld, hop 0: max_amount_in must be finite and >= 0", who, (long long)p);
            return CFMM_ERR_INVALID_ARG;
        }
        if (value_in && !size_value_ok(value_in[p])) {
            std::snprintf(msg, len, "%s: path %lld, hop 0: value_in must be finite and > 0", who, (long long)p);
            return CFMM_ERR_INVALID_ARG;
        }
        if (value_out && !size_value_ok(value_out[p])) {
            std::snprintf(msg, len, "%s: path %lld, hop 0: value_out must be finite and > 0", who, (long long)p);
            return CFMM_ERR_INVALID_ARG;
        }
    }
    return CFMM_OK;
}

} // namespace cfmm
