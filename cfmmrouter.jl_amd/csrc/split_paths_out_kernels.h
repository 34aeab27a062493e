// split_paths_out_kernels.h -- cfmm_split_paths_out: a wanted amount bought through an order's K <= 8 paths by the greedy
// search of include/cfmm_amd_split_out.h.  split_paths_kernel's shape (split_paths_kernels.h): ONE WAVEFRONT PER ORDER, ONE
// LANE PER GRID POINT, wavefronts grid-stride over the orders; the order number is made scalar, so the path range, the hop
// records, the segment records, the kind switch of path_step and the pools' state are wave-uniform; eight registers per
// per-path quantity through split_get / split_set; the greedy's 63 steps are split_out_grid.h's split_out_greedy -- the host's
// text -- run by every lane on wave-uniform values, a winner's next increment fetched with split_take.  No LDS, no scratch, no
// atomics, no barrier.
// Per round lane j carries the share x[k][j] BACKWARDS through the hops of path k, from the last to the first, with
// path_step<true> of quote_path_kernels.h, UNCHANGED, and with quote_path_out_kernel's rule that +inf and NaN pass through
// unevaluated.  The lanes of one wavefront carry different amounts, so some stand at +inf while others do not: the skip is a
// PREDICATE around the hop (`if (c < inf)` on the lane's own value), and the hop loop's bounds stay wave-uniform.  There is
// no cross-lane operation inside a hop; every lane is active again at the __shfl_down behind the loop and through the greedy.
// An invalid order (split_paths_kernel's list) takes the same instructions with a NaN amount and is marked at the end.  The
// path range is tested before it is used and path_step clamps every index before any read: the kernel never reads out of
// bounds.  Lane 0 writes the outputs.
#pragma once

#include "split_out_grid.h"
#include "split_paths_kernels.h"

namespace cfmm {

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void split_paths_out_kernel(SplitArgs a)
{
    static_assert(BLOCK % CFMM_SPLIT_POINTS == 0, "whole wavefronts");
    constexpr int kWaves = BLOCK / CFMM_SPLIT_POINTS;
    constexpr int KMAX = CFMM_MAX_SPLIT_PATHS;
    const int j = (int)(threadIdx.x % CFMM_SPLIT_POINTS);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CFMM_SPLIT_POINTS));
    const int64_t step = (int64_t)gridDim.x * kWaves;
    const int rounds = a.rounds;
    const double nan = __builtin_nan("");
    for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < a.orders; g += step) {
        // the path range, tested before it is used (the difference is taken only of two values inside 0 .. count)
        long long first = a.order_first[g];
        const long long end = a.order_first[g + 1];
        const bool range_ok = first >= 0 && end <= a.p.count && end > first && end - first <= KMAX;
        const int K = range_ok ? (int)(end - first) : 0;
        first = range_ok ? first : 0;
        const double amount = a.amount[g];
        bool valid = range_ok && split_amount_ok(amount);
        for (int k = 0; k < K; ++k) {
            const int nh = a.p.n_hops[first + k];
            valid = valid && nh >= 1 && nh <= a.p.max_hops;
        }
        const double B = valid ? amount : nan;   // (an invalid order: every grid point NaN, no hop evaluated)
        double base[KMAX], x[KMAX], c[KMAX], d[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) base[k] = x[k] = c[k] = d[k] = 0.0;
        int n[KMAX];
        double rem = B;
        int bad = kSplitOutClean;
        for (int r = 0; r < rounds; ++r) {
            const double s = split_slice(rem);
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const int64_t p = first + k;
                const int nh = valid ? a.p.n_hops[p] : 0;
                const double xk = split_point(split_get(base, k), s, rem, j);
                double ck = xk;
                for (int h = nh - 1; h >= 0; --h)
                    if (ck < __builtin_inf()) ck = path_step<true>(a.p, (int64_t)h * a.p.count + p, ck);   // (+inf and NaN pass through)
                split_set(x, k, xk);
                split_set(c, k, ck);
                split_set(d, k, __shfl_down(ck, 1, CFMM_SPLIT_POINTS) - ck);   // lane 63's is never asked for
            }
            bad = split_out_greedy(K, [&](int k, int at) { return split_take(d, k, at); }, n, bad);
            if (r + 1 < rounds) {
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) {
                        base[k] = __shfl(x[k], split_back(n[k]), CFMM_SPLIT_POINTS);
                        sum = k == 0 ? base[k] : sum + base[k];
                    }
                rem = split_rem(B, sum);
            }
        }
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                x[k] = __shfl(x[k], n[k], CFMM_SPLIT_POINTS);
                c[k] = __shfl(c[k], n[k], CFMM_SPLIT_POINTS);
                total = k == 0 ? c[k] : total + c[k];
            }
        if (K == 0) total = nan;
        if (j == 0) {
            const int32_t st = split_out_status(bad, B, total);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {
                    a.p.answer[first + k] = split_out_written_share(st, x[k]);
                    a.path_out[first + k] = split_out_written_cost(st, c[k]);
                }
            a.total[g] = split_out_written_cost(st, total);
            a.status[g] = st;
        }
    }
}

} // namespace cfmm

// (what came after this header is included from here, behind everything above: find_path_kernels.h's rule)
#include "swap_order_kernels.h"
