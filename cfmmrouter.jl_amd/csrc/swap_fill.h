// swap_fill.h -- internal, host only, HIP-free: what the driver of the executing path entries (abi_swap_path.cpp
// swap_paths_run: cfmm_swap_path(_out), cfmm_swap_order(_out)) does to plain host arrays -- the caller's columns into launch
// order, the answers back into the caller's order, and the rule by which a UniV3 pool follows a landing price (abi_swap.cpp
// uses that one too).  tests/native/path_rig_host.cpp builds this for the CPU.
// OWNERS: the units that are applied all or nothing and that the planner (swap_path_waves.h) orders -- the orders, or with
// order_first null the paths themselves.  An owner's paths stay together in launch order, so a wave is one span of the
// owners and one span of the paths.
#pragma once

#include "swap_path_waves.h"

#include <cstring>

namespace cfmm {

// the caller's hop columns, hop-major for n paths (hop k of path p at k*n + p; slots at k >= n_hops[p] are not looked at)
struct HopCols {
    const int32_t *n_hops, *seg;
    const int64_t* row;
    const int32_t *coin_in, *coin_out;
};

// Where a UniV3 pool whose swap lands at price `landing` goes: out of liquidity on that side it rests at the first tick's
// upper price `top`; a pool that comes to rest where it stands -- the bits of `current`: amount 0, no liquidity -- does not
// move (-0.0 and +0.0 are different bits).  True: it moves to `to`.
inline bool univ3_landing(double landing, double top, double current, double& to)
{
    to = landing > top ? top : landing;
    return std::memcmp(&to, &current, sizeof to) != 0;
}

// The columns in launch order (stage_layout.h SwapPathStage's i32 / row / amt): n_hops and the three int32 hop columns, hop_row
// and behind it -- for orders -- order_first [owners + 1] (where the owner at position j starts in the launch order), the
// given amounts and behind them the limits of the owners, where given.  The slots a path does not use are zeroed (never read
// by the kernel).
inline void fill_launch_order(const SwapPathPlan& plan, const int64_t* order_first, size_t n, size_t H, const HopCols& in, const double* given,
                              const double* limit, int32_t* h_i32, long long* h_i64, double* h_amt)
{
    const size_t nh = n * H, owners = plan.perm.size();
    int32_t *h_seg = h_i32 + n, *h_ci = h_seg + nh, *h_co = h_ci + nh;
    long long* h_first = order_first ? h_i64 + nh : nullptr;
    std::memset(h_seg, 0, 3 * nh * sizeof(int32_t));
    std::memset(h_i64, 0, nh * sizeof(long long));
    size_t at = 0;
    for (size_t j = 0; j < owners; ++j) {
        const size_t g = (size_t)plan.perm[j];
        if (h_first) h_first[j] = (long long)at;
        if (limit) h_amt[n + j] = limit[g];
        const size_t q1 = order_first ? (size_t)order_first[g + 1] : g + 1;
        for (size_t q = order_first ? (size_t)order_first[g] : g; q < q1; ++q, ++at) {
            h_i32[at] = in.n_hops[q];
            h_amt[at] = given[q];
            for (size_t k = 0; k < (size_t)in.n_hops[q]; ++k) {
                h_seg[k * n + at] = in.seg[k * n + q];
                h_i64[k * n + at] = in.row[k * n + q];
                h_ci[k * n + at] = in.coin_in[k * n + q];
                h_co[k * n + at] = in.coin_out[k * n + q];
            }
        }
    }
    if (h_first) h_first[owners] = (long long)at;   // == n
}

// The inverse, on what came back (SwapPathStage's out / status / hops: the paths' [n], then -- for orders -- the owners'):
// every path's answer, status and hop amounts and every order's total and status go where the caller has them.  path_status,
// hop_ans: null where the caller does not want them; total / status: the orders' (null without orders).  Returns the owners
// that were not applied (status 0 is APPLIED in every entry).
inline int64_t scatter_to_caller(const SwapPathPlan& plan, const int64_t* order_first, size_t n, size_t H, const double* h_out,
                                 const int32_t* h_status, const double* h_hops, double* answer, int32_t* path_status, double* hop_ans,
                                 double* total, int32_t* status)
{
    const size_t owners = plan.perm.size();
    int64_t refused = 0;
    size_t p = 0;
    for (size_t j = 0; j < owners; ++j) {
        const size_t g = (size_t)plan.perm[j];
        if (order_first) {
            total[g] = h_out[n + j];
            status[g] = h_status[n + j];
        }
        refused += h_status[(order_first ? n : 0) + j] != 0;
        const size_t q1 = order_first ? (size_t)order_first[g + 1] : g + 1;
        for (size_t q = order_first ? (size_t)order_first[g] : g; q < q1; ++q, ++p) {
            answer[q] = h_out[p];
            if (path_status) path_status[q] = h_status[p];
            if (hop_ans)
                for (size_t k = 0; k < H; ++k) hop_ans[k * n + q] = h_hops[k * n + p];
        }
    }
    return refused;
}

} // namespace cfmm
