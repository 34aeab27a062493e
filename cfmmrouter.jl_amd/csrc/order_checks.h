// order_checks.h -- internal, host only, HIP-free: the checks of cfmm_swap_order / cfmm_swap_order_out (abi_swap_order.cpp;
// include/cfmm_amd_order.h) before anything is enqueued.  Nothing here is new: the paths are checked as cfmm_swap_path checks
// them (path_checks.h check_paths, swap_path_checks.h check_swap_paths), the orders as cfmm_split_paths checks them
// (split_checks.h: the path ranges, and the rule that no pool occurs twice among the hops of one order's paths, with its
// text), and a limit, where one is given, is finite and >= 0.  As there, a refusal's text goes into a caller's buffer, so a
// host program without a device or a context can exercise them (tests/native/order_checks_host.cpp).  A refusal names the
// order, and the path (numbered within the order) and hop where there is one.
#pragma once

#include "split_checks.h"
#include "swap_path_checks.h"

namespace cfmm {

// All of a call's checks, in the order the contract lists them.  `segs`: the market as check_paths takes it.  given / limit /
// answer / total: path_amount_in, min_total_out, path_amount_out, total_out of cfmm_swap_order; path_amount_out, max_total_in,
// path_amount_in, total_in of cfmm_swap_order_out (exact_out).
inline int check_orders(const char* who, bool exact_out, const PathSegInfo* segs, int64_t nseg, int64_t count, const int64_t* order_first,
                        int64_t n_paths, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                        const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* given, const double* limit,
                        const void* answer, const void* total, const void* status, char* msg, size_t len)
{
    int rc = check_path_scalars(who, count, max_hops, msg, len);
    if (rc != CFMM_OK) return rc;
    if (n_paths < 0 || (count > 0 && n_paths < 1)) {
        std::snprintf(msg, len, "%s: n_paths must be >= %d (got %lld)", who, count > 0 ? 1 : 0, (long long)n_paths);
        return CFMM_ERR_INVALID_ARG;
    }
    if (count > 0 && (!order_first || !total || !status)) {
        std::snprintf(msg, len, "%s: null order array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    if (count > 0 && (!n_hops || !hop_seg || !hop_row || !hop_coin_in || !hop_coin_out || !given || !answer)) {
        std::snprintf(msg, len, "%s: null path array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    // (check_split_orders wants an amount per order: the orders have none of their own, so it is given zeros)
    const std::vector<double> zeros((size_t)(count > 0 ? count : 0), 0.0);
    if ((rc = check_split_orders(who, count, order_first, zeros.data(), n_paths, msg, len)) != CFMM_OK) return rc;
    if (count == 0) return CFMM_OK;
    rc = check_paths(who, exact_out, segs, nseg, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, given, msg, len);
    if (rc == CFMM_OK) rc = check_swap_paths(who, n_paths, n_hops, hop_seg, hop_row, nullptr, msg, len, exact_out);
    if (rc != CFMM_OK) {
        split_name_order(who, count, order_first, msg, len);
        return rc;
    }
    if ((rc = check_split_pools(who, count, order_first, n_paths, n_hops, hop_seg, hop_row, msg, len)) != CFMM_OK) return rc;
    if (limit)
        for (int64_t g = 0; g < count; ++g)
            if (!(limit[g] >= 0.0) || !std::isfinite(limit[g])) {
                std::snprintf(msg, len, "%s: order %lld: %s must be finite and >= 0", who, (long long)g, exact_out ? "max_total_in" : "min_total_out");
                return CFMM_ERR_INVALID_ARG;
            }
    return CFMM_OK;
}

} // namespace cfmm
