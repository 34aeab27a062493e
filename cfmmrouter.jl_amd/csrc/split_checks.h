// split_checks.h -- internal, host only, HIP-free: the checks of cfmm_split_paths / cfmm_split_paths_dev and of their
// exact-output twins cfmm_split_paths_out / cfmm_split_paths_out_dev, the same checks under the other name (abi_split_paths.cpp)
// beyond those of the paths themselves, which stay path_checks.h's check_paths: the scalars, the orders' path ranges and
// amounts, and the rule that no pool occurs twice among the hops of one order's paths.  As there, a refusal's text goes into a
// caller's buffer, so a host program without a device or a context can exercise them (tests/native/split_checks_host.cpp).
// A refusal names the order, and the path (numbered within the order) and hop where there is one.
#pragma once

#include "path_checks.h"
#include "split_grid.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace cfmm {

// the scalars both entries check
inline int check_split_scalars(const char* who, int64_t count, int64_t n_paths, int32_t max_hops, int32_t rounds, char* msg, size_t len)
{
    const int rc = check_path_scalars(who, count, max_hops, msg, len);
    if (rc != CFMM_OK) return rc;
    if (n_paths < 0 || (count > 0 && n_paths < 1)) {
        std::snprintf(msg, len, "%s: n_paths must be >= %d (got %lld)", who, count > 0 ? 1 : 0, (long long)n_paths);
        return CFMM_ERR_INVALID_ARG;
    }
    if (rounds < 1 || rounds > CFMM_MAX_SPLIT_ROUNDS) {
        std::snprintf(msg, len, "%s: rounds must be 1 .. %d (got %d)", who, CFMM_MAX_SPLIT_ROUNDS, (int)rounds);
        return CFMM_ERR_INVALID_ARG;
    }
    return CFMM_OK;
}

// ... and the arrays neither entry accepts null when there are orders
inline int check_split_arrays(const char* who, int64_t count, const void* order_first, const void* amount_in, const void* n_hops,
                              const void* hop_seg, const void* hop_row, const void* hop_coin_in, const void* hop_coin_out,
                              const void* path_amount_in, const void* path_amount_out, const void* total_out, const void* status,
                              char* msg, size_t len)
{
    if (count > 0 && (!order_first || !amount_in || !path_amount_in || !path_amount_out || !total_out || !status)) {
        std::snprintf(msg, len, "%s: null order array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    if (count > 0 && (!n_hops || !hop_seg || !hop_row || !hop_coin_in || !hop_coin_out)) {
        std::snprintf(msg, len, "%s: null path array", who);
        return CFMM_ERR_INVALID_ARG;
    }
    return CFMM_OK;
}

// every order's path range and amount of a host-pointer call (the arrays are known not to be null)
// (`amount_name`: what the entry calls the amount -- cfmm_split_paths_out's is amount_out)
inline int check_split_orders(const char* who, int64_t count, const int64_t* order_first, const double* amount_in, int64_t n_paths,
                              char* msg, size_t len, const char* amount_name = "amount_in")
{
    if (count == 0) {
        if (n_paths != 0) {
            std::snprintf(msg, len, "%s: %lld paths belong to no order (count is 0)", who, (long long)n_paths);
            return CFMM_ERR_INVALID_ARG;
        }
        return CFMM_OK;
    }
    if (order_first[0] != 0) {
        std::snprintf(msg, len, "%s: order 0: order_first[0] must be 0 (got %lld)", who, (long long)order_first[0]);
        return CFMM_ERR_INVALID_ARG;
    }
    for (int64_t g = 0; g < count; ++g) {
        const int64_t lo = order_first[g], hi = order_first[g + 1];
        if (hi < lo) {
            std::snprintf(msg, len, "%s: order %lld: order_first decreases (%lld after %lld)", who, (long long)g, (long long)hi, (long long)lo);
            return CFMM_ERR_INVALID_ARG;
        }
        if (hi > n_paths) {
            std::snprintf(msg, len, "%s: order %lld: its paths end at %lld, beyond n_paths %lld", who, (long long)g, (long long)hi,
                          (long long)n_paths);
            return CFMM_ERR_INVALID_ARG;
        }
        if (hi - lo < 1 || hi - lo > CFMM_MAX_SPLIT_PATHS) {
            std::snprintf(msg, len, "%s: order %lld: %lld paths (an order has 1 .. %d)", who, (long long)g, (long long)(hi - lo),
                          CFMM_MAX_SPLIT_PATHS);
            return CFMM_ERR_INVALID_ARG;
        }
        if (!split_amount_ok(amount_in[g])) {
            std::snprintf(msg, len, "%s: order %lld: %s must be finite and >= 0", who, (long long)g, amount_name);
            return CFMM_ERR_INVALID_ARG;
        }
    }
    if (order_first[count] != n_paths) {
        std::snprintf(msg, len, "%s: order_first[count] must be n_paths %lld (got %lld)", who, (long long)n_paths,
                      (long long)order_first[count]);
        return CFMM_ERR_INVALID_ARG;
    }
    return CFMM_OK;
}

// check_paths names a path by its number in the call; a split names the order and the path within it.  Rewrites
// "<who>: path P..." in msg as "<who>: order G: path P - order_first[G]..." (the orders are known to be valid).
inline void split_name_order(const char* who, int64_t count, const int64_t* order_first, char* msg, size_t len)
{
    char head[96];
    std::snprintf(head, sizeof head, "%s: path ", who);
    const size_t hl = std::strlen(head);
    if (std::strncmp(msg, head, hl) != 0) return;
    char* rest = nullptr;
    const long long p = std::strtoll(msg + hl, &rest, 10);
    const int64_t* at = std::upper_bound(order_first, order_first + count + 1, (int64_t)p);
    const int64_t g = (at - order_first) - 1;
    if (g < 0 || g >= count) return;
    const std::string tail(rest);
    std::snprintf(msg, len, "%s: order %lld: path %lld%s", who, (long long)g, (long long)(p - order_first[g]), tail.c_str());
}

// No pool (segment, row) twice among all hops of one order's paths (a path's own hops included: the paths are quoted against
// the standing market, so a second visit would ignore the first).  The orders and the paths are known to be valid.
inline int check_split_pools(const char* who, int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops,
                             const int32_t* hop_seg, const int64_t* hop_row, char* msg, size_t len)
{
    struct Visit {
        int32_t seg;
        int64_t row;
        int path;
    };
    std::vector<Visit> v;
    for (int64_t g = 0; g < count; ++g) {
        v.clear();
        for (int64_t p = order_first[g]; p < order_first[g + 1]; ++p)
            for (int k = 0; k < n_hops[p]; ++k) v.push_back({hop_seg[(int64_t)k * n_paths + p], hop_row[(int64_t)k * n_paths + p], (int)(p - order_first[g])});
        // at most 64 visits: the first repeat in (path, hop) order, by comparing every pair
        for (size_t i = 1; i < v.size(); ++i)
            for (size_t h = 0; h < i; ++h)
                if (v[h].seg == v[i].seg && v[h].row == v[i].row) {
                    std::snprintf(msg, len, "%s: order %lld: paths %d and %d share pool (segment %d, row %lld)", who, (long long)g,
                                  v[h].path, v[i].path, (int)v[i].seg, (long long)v[i].row);
                    return CFMM_ERR_INVALID_ARG;
                }
    }
    return CFMM_OK;
}

// All of a host-pointer call's checks, in the order the contract lists them.  `segs`: the market as check_paths takes it.
inline int check_split(const char* who, const PathSegInfo* segs, int64_t nseg, int64_t count, const int64_t* order_first,
                       const double* amount_in, int64_t n_paths, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                       const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, int32_t rounds,
                       const void* path_amount_in, const void* path_amount_out, const void* total_out, const void* status, char* msg,
                       size_t len, const char* amount_name = "amount_in")
{
    int rc;
    if ((rc = check_split_scalars(who, count, n_paths, max_hops, rounds, msg, len)) ||
        (rc = check_split_arrays(who, count, order_first, amount_in, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, path_amount_in,
                                 path_amount_out, total_out, status, msg, len)) ||
        (rc = check_split_orders(who, count, order_first, amount_in, n_paths, msg, len, amount_name)))
        return rc;
    if (count == 0) return CFMM_OK;
    // (check_paths wants an amount per path: the paths have none of their own, so it is given zeros)
    const std::vector<double> zeros((size_t)n_paths, 0.0);
    rc = check_paths(who, false, segs, nseg, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, zeros.data(), msg, len);
    if (rc != CFMM_OK) {
        split_name_order(who, count, order_first, msg, len);
        return rc;
    }
    return check_split_pools(who, count, order_first, n_paths, n_hops, hop_seg, hop_row, msg, len);
}

} // namespace cfmm
