// split_paths_kernels.h -- cfmm_split_paths: an order's amount spread over its K <= 8 paths by the greedy search of
// include/cfmm_amd_split.h.  ONE WAVEFRONT PER ORDER, ONE LANE PER GRID POINT; wavefronts grid-stride over the orders.
// The order number is made scalar (readfirstlane), so everything that describes the order -- its path range, each path's hop
// records, the segment records, the kind switch of path_step, the pools' state -- is wave-uniform: no divergence on the kind,
// the pool loads are broadcasts.  Per round lane j carries x[k][j] (split_grid.h split_point) through the hops of path k with
// path_step<false> of quote_path_kernels.h, UNCHANGED, so an amount's bits are cfmm_quote's, for k = 0 .. K-1 in ONE rolled
// loop (one copy of path_step's text); what path k gave is put into registers x[k], y[k] through eight selects on constant
// indices (split_grid.h split_set), so no array is indexed by a variable and nothing goes to scratch.  Lane j then holds every path's increment
// y[k][j+1] - y[k][j], and the greedy's 63 steps are split_grid.h's split_greedy -- the host's text -- run by every lane on
// wave-uniform values: a step compares the K next increments, and fetches the winner's new one from lane n_k with a
// uniform-index lane read (split_take: split_get's select over k, then __shfl).  No LDS, no atomics, no barrier, no global float
// reduction; the result is the serial greedy because it IS the serial greedy.
// Every lane stays active through every cross-lane step: the loops below have wave-uniform bounds, and an order that is
// invalid (a path range that is not 1 .. 8 paths inside the arrays, an n_hops outside 1 .. max_hops, a bad hop, an amount that
// is no valid number) takes the same instructions -- its amount is made NaN, path_step's rule carries the NaN -- and is marked
// at the end.  The path range is tested before it is used and path_step clamps every index before any read: the kernel never
// reads out of bounds.  Lane 0 writes the outputs.
#pragma once

#include "quote_path_kernels.h"
#include "split_grid.h"

namespace cfmm {

static_assert(CFMM_SPLIT_POINTS == 64, "one grid point per lane of a wave64 wavefront");

// lane `lane`'s v[k], k wave-uniform (split_grid.h split_get: a select over the eight registers, then one lane read)
__device__ __forceinline__ double split_take(const double (&v)[CFMM_MAX_SPLIT_PATHS], int k, int lane)
{
    return __shfl(split_get(v, k), lane, CFMM_SPLIT_POINTS);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void split_paths_kernel(SplitArgs a)
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
        const double A = valid ? amount : nan;   // (an invalid order: every grid point NaN, no hop evaluated on a number)
        double base[KMAX], x[KMAX], y[KMAX], d[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) base[k] = x[k] = y[k] = d[k] = 0.0;
        int n[KMAX];
        double rem = A;
        bool any_nan = false, last_flat = false;
        for (int r = 0; r < rounds; ++r) {
            const double s = split_slice(rem);
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const int64_t p = first + k;
                const int nh = valid ? a.p.n_hops[p] : 0;
                const double xk = split_point(split_get(base, k), s, rem, j);
                double yk = xk;
                for (int h = 0; h < nh; ++h) yk = path_step<false>(a.p, (int64_t)h * a.p.count + p, yk);
                split_set(x, k, xk);
                split_set(y, k, yk);
                split_set(d, k, __shfl_down(yk, 1, CFMM_SPLIT_POINTS) - yk);   // lane 63's is never asked for
            }
            const int flags = split_greedy(K, [&](int k, int at) { return split_take(d, k, at); }, n);
            any_nan = any_nan || (flags & kSplitStepNan) != 0;
            last_flat = (flags & kSplitStepFlat) != 0;
            if (r + 1 < rounds) {
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) {
                        base[k] = __shfl(x[k], split_back(n[k]), CFMM_SPLIT_POINTS);
                        sum = k == 0 ? base[k] : sum + base[k];
                    }
                rem = split_rem(A, sum);
            }
        }
        double total = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                x[k] = __shfl(x[k], n[k], CFMM_SPLIT_POINTS);
                y[k] = __shfl(y[k], n[k], CFMM_SPLIT_POINTS);
                total = k == 0 ? y[k] : total + y[k];
            }
        if (K == 0) total = nan;
        if (j == 0) {
            const int32_t st = split_status(any_nan, last_flat, A, total);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {
                    a.p.answer[first + k] = split_written(st, x[k]);
                    a.path_out[first + k] = split_written(st, y[k]);
                }
            a.total[g] = split_written(st, total);
            a.status[g] = st;
        }
    }
}

} // namespace cfmm

// (what came after this header is included from here, behind everything above: find_path_kernels.h's rule)
#include "find_disjoint_kernels.h"
