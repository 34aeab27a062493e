// swap_order_kernels.h -- cfmm_swap_order / cfmm_swap_order_out (include/cfmm_amd_order.h): orders that MOVE their pools, each
// all or nothing ACROSS its K <= 8 paths.  EIGHT LANES PER ORDER, ONE LANE PER PATH SLOT, eight orders per wavefront;
// wavefronts grid-stride over the orders of one wave (orders that share no pool: swap_order_waves.h).  Lane j of a group owns
// path first + j where j < K and otherwise carries nothing: no hop, no store.
//   1. Each lane runs pass 1 of its path: swap_path_kernel's / swap_path_out_kernel's loop with hop_try UNCHANGED
//      (swap_path_kernels.h), so the amounts carry cfmm_quote_path's / cfmm_quote_path_out's bits, the refusals are cfmm_swap's
//      and the hop amounts are written as those kernels write them for a path that does not pass.
//   2. The group combines in registers: whether any path refuses (or cannot give its amount) is a ballot masked to the group's
//      eight bits; the total is eight width-8 lane reads added in increasing k, the first term taken as it is -- the serial
//      sum split_paths_kernel forms, never a tree.
//   3. The limit test and the status are computed on group-uniform values.
//   4. Pass 2 (apply_hop) runs in each lane that owns a path of an applied order.
// No LDS, no atomic, no barrier, no float reduction in memory.  Every lane stays active through every cross-lane step: the
// order loop's bound is wavefront-uniform (a group behind the wave's last order repeats that order's reads and stores
// nothing), the hop loops rejoin before step 2.  An order with a bad path range or a bad n_hops takes the same instructions
// and is marked REFUSED with NaN; every index is clamped before any read (split_paths_kernel's rule).
#pragma once

#include "../../include/cfmm_amd_split.h"
#include "swap_path_kernels.h"

namespace cfmm {

constexpr int kOrderLanes = 8;   // lanes per order = CFMM_MAX_SPLIT_PATHS
static_assert(kOrderLanes == CFMM_MAX_SPLIT_PATHS && 64 % kOrderLanes == 0, "one lane per path slot, whole groups per wavefront");

// What a lane knows of its order before it walks: the order (clamped), its path (clamped) and whether it owns one
struct OrderLane {
    int64_t g, p;   // the order, clamped into the wave; the lane's path, clamped into the arrays
    int K;          // paths of the order (0: a bad range)
    bool live;      // the group has an order of its own
    bool range_ok;
    bool mine;      // the lane owns path p
};
__device__ __forceinline__ OrderLane order_lane(const SwapOrderArgs& a, int64_t g, int j)
{
    OrderLane o;
    o.live = g < a.orders;
    o.g = o.live ? g : a.orders - 1;
    // the path range, tested before it is used (the difference is taken only of two values inside 0 .. count)
    long long first = a.order_first[o.g];
    const long long end = a.order_first[o.g + 1];
    o.range_ok = first >= 0 && end <= a.p.count && end > first && end - first <= kOrderLanes;
    o.K = o.range_ok ? (int)(end - first) : 0;
    first = o.range_ok ? first : 0;
    o.mine = o.live && j < o.K;
    o.p = first + (j < o.K ? j : 0);
    return o;
}

// y_0 + y_1 + ... + y_{K-1} of the group, in increasing k, on every lane of the group (K is group-uniform)
__device__ __forceinline__ double order_total(double y, int K)
{
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < kOrderLanes; ++k) {
        const double yk = __shfl(y, k, kOrderLanes);
        if (k < K) total = k == 0 ? yk : total + yk;
    }
    return total;
}

// whether `flag` holds in some lane of this lane's group of eight
__device__ __forceinline__ bool order_any(bool flag, int lane)
{
    const unsigned long long group = 0xffull << (lane & ~(kOrderLanes - 1));
    return (__ballot(flag) & group) != 0;
}

// exact input: the lane's walk is swap_path_kernel's pass 1, the statuses are kOrder* / kPath* / kOrderPathHeld
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void swap_order_kernel(SwapOrderArgs a)
{
    static_assert(BLOCK % 64 == 0, "whole wavefronts");
    constexpr int kPerBlock = BLOCK / kOrderLanes, kPerWave = 64 / kOrderLanes;
    const double nan = __builtin_nan("");
    const int lane = (int)(threadIdx.x % 64), j = lane % kOrderLanes;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const int64_t step = (int64_t)gridDim.x * kPerBlock;
    for (int64_t g0 = (int64_t)blockIdx.x * kPerBlock + wave * kPerWave; g0 < a.orders; g0 += step) {
        const OrderLane o = order_lane(a, g0 + lane / kOrderLanes, j);
        const int64_t p = o.p;
        int nh = a.p.n_hops[p];
        const double given = a.p.amount_in[p];
        double x = given;
        int status = kPathApplied;
        if (nh < 1 || nh > a.p.max_hops) {   // (the host has refused such a call; nothing is evaluated)
            nh = 0;
            x = nan;
            status = kPathRefused;
        }
        if (!o.mine) nh = 0;
        int k = 0;
        for (; k < nh && status == kPathApplied; ++k) {
            const int64_t at = (int64_t)k * a.p.stride + p;
            double r;
            if (hop_try<false>(a.p, at, x, r)) {
                x = r;
            } else {
                x = nan;
                status = kPathRefused;
            }
            a.p.hops[at] = x;
        }
        if (o.mine)
            for (; k < a.p.max_hops; ++k) a.p.hops[(int64_t)k * a.p.stride + p] = nan;   // behind a refusing hop, and the unused slots
        // the group's verdict, on group-uniform values
        const bool refused = order_any(o.mine && status == kPathRefused, lane) || !o.range_ok;
        const double sum = order_total(o.mine ? x : 0.0, o.K);
        const double total = refused ? nan : sum;
        int32_t verdict = kOrderApplied;
        if (refused) verdict = kOrderRefused;
        else if (a.limit && !(total >= a.limit[o.g])) verdict = kOrderLimit;
        if (o.live && j == 0) {
            a.total[o.g] = total;
            a.status[o.g] = verdict;
        }
        if (o.mine) {
            a.p.amount_out[p] = x;
            a.p.status[p] = status == kPathRefused ? kPathRefused : (verdict == kOrderApplied ? kPathApplied : kOrderPathHeld);
        }
        if (!o.mine || verdict != kOrderApplied) nh = 0;   // (no `continue`: every lane reaches the loop's end together)
        double amt = given;
        for (k = 0; k < nh; ++k) {
            const int64_t at = (int64_t)k * a.p.stride + p;
            const double out = a.p.hops[at];
            if (amt != 0.0) apply_hop(a.p, at, amt, out);
            amt = out;
        }
    }
}

// exact OUTPUT, on the same arguments with the roles of the amounts exchanged (sweep.h): the lane's walk is
// swap_path_out_kernel's pass 1, from the last hop to the first; a path that answers +inf makes the order kOrderUnobtainable
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void swap_order_out_kernel(SwapOrderArgs a)
{
    static_assert(BLOCK % 64 == 0, "whole wavefronts");
    constexpr int kPerBlock = BLOCK / kOrderLanes, kPerWave = 64 / kOrderLanes;
    const double nan = __builtin_nan("");
    const int lane = (int)(threadIdx.x % 64), j = lane % kOrderLanes;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const int64_t step = (int64_t)gridDim.x * kPerBlock;
    for (int64_t g0 = (int64_t)blockIdx.x * kPerBlock + wave * kPerWave; g0 < a.orders; g0 += step) {
        const OrderLane o = order_lane(a, g0 + lane / kOrderLanes, j);
        const int64_t p = o.p;
        int nh = a.p.n_hops[p];
        const double want = a.p.amount_in[p];
        double y = want;
        int status = kSwapApplied;
        if (nh < 1 || nh > a.p.max_hops) {   // (the host has refused such a call; nothing is evaluated)
            nh = 0;
            y = nan;
            status = kSwapRefused;
        }
        if (!o.mine) nh = 0;
        if (o.mine)
            for (int k = nh; k < a.p.max_hops; ++k) a.p.hops[(int64_t)k * a.p.stride + p] = nan;   // the unused slots
        int k = nh - 1;
        for (; k >= 0 && status == kSwapApplied; --k) {
            const int64_t at = (int64_t)k * a.p.stride + p;
            double r;
            if (!hop_try<true>(a.p, at, y, r)) {
                y = nan;
                status = kSwapRefused;
            } else {
                y = r;
                if (r == __builtin_inf()) status = kSwapUnobtainable;
            }
            a.p.hops[at] = y;
        }
        for (; k >= 0; --k) a.p.hops[(int64_t)k * a.p.stride + p] = y;   // towards hop 0 of a hop that refused (NaN) or cannot give (+inf)
        // the group's verdict, on group-uniform values
        const bool refused = order_any(o.mine && status == kSwapRefused, lane) || !o.range_ok;
        const bool unobtainable = order_any(o.mine && status == kSwapUnobtainable, lane);
        const double sum = order_total(o.mine ? y : 0.0, o.K);
        const double total = refused ? nan : (unobtainable ? __builtin_inf() : sum);
        int32_t verdict = kOrderApplied;
        if (refused) verdict = kOrderRefused;
        else if (unobtainable) verdict = kOrderUnobtainable;
        else if (a.limit && !(total <= a.limit[o.g])) verdict = kOrderLimit;
        if (o.live && j == 0) {
            a.total[o.g] = total;
            a.status[o.g] = verdict;
        }
        if (o.mine) {
            a.p.amount_out[p] = y;
            a.p.status[p] = status != kSwapApplied ? status : (verdict == kOrderApplied ? kPathApplied : kOrderPathHeld);
        }
        if (!o.mine || verdict != kOrderApplied) nh = 0;   // (no `continue`: every lane reaches the loop's end together)
        double out = want;
        for (k = nh - 1; k >= 0; --k) {
            const int64_t at = (int64_t)k * a.p.stride + p;
            const double in = a.p.hops[at];
            if (out != 0.0) apply_hop(a.p, at, in, out);
            out = in;
        }
    }
}

} // namespace cfmm

// (the next kernels of the translation unit: the include chain of sweep_kernels.hip goes on from here)
#include "rate_kernels.h"
