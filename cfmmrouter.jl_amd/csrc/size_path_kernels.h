// size_path_kernels.h -- cfmm_size_path: the input of a path that maximises its gain, by the bracketing search of
// include/cfmm_amd_size_path.h.  ONE WAVEFRONT PER PATH, ONE LANE PER TRIAL SIZE; wavefronts grid-stride over the paths.
// The path number is made scalar (readfirstlane), so everything that describes the path -- its hop records, the segment
// records, the kind switch of path_step, the pool's state -- is wave-uniform: no divergence on the kind, the pool loads are
// broadcasts.  Per round lane j carries x_j (size_grid.h size_trial) through the hops with path_step<false> of
// quote_path_kernels.h, UNCHANGED, so an amount's bits are cfmm_quote's; the arg-max over (gain, j) is a six-step butterfly
// under the total order size_better, whose result cannot depend on the order of the steps; the winner's two neighbours are
// read from their lanes and are the next bracket.  No LDS, no atomics, no barrier, no global float reduction.
// Every lane stays active through every cross-lane step: the loops below have wave-uniform bounds, and a path that is invalid
// (n_hops outside 1 .. max_hops, a bad hop, a limit or a value that is no valid number) or whose gains are all NaN takes the
// same instructions -- its limit is made NaN, path_step's rule carries the NaN -- and is marked at the end.  path_step clamps
// every index before any read: the kernel never reads out of bounds.  Lane 0 writes the four outputs.
// A path's hop records (at most 8 x 20 bytes) are read through path_step's own loads: their addresses are wave-uniform and
// nothing is stored between a path's first round and its last, so after the first round they come from the cache.
#pragma once

#include "quote_path_kernels.h"
#include "size_grid.h"

namespace cfmm {

static_assert(CFMM_SIZE_POINTS == 64, "one trial size per lane of a wave64 wavefront");

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void size_path_kernel(SizeArgs a)
{
    static_assert(BLOCK % CFMM_SIZE_POINTS == 0, "whole wavefronts");
    constexpr int kWaves = BLOCK / CFMM_SIZE_POINTS;
    const int j = (int)(threadIdx.x % CFMM_SIZE_POINTS);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CFMM_SIZE_POINTS));
    const int64_t step = (int64_t)gridDim.x * kWaves;
    const int rounds = a.rounds;
    for (int64_t p = (int64_t)blockIdx.x * kWaves + wave; p < a.p.count; p += step) {
        int nh = a.p.n_hops[p];
        const double max_in = a.p.given[p];
        const double vi = a.value_in ? a.value_in[p] : 1.0;
        const double vo = a.value_out ? a.value_out[p] : 1.0;
        bool valid = size_limit_ok(max_in) && size_value_ok(vi) && size_value_ok(vo);
        if (nh < 1 || nh > a.p.max_hops) {
            nh = 0;
            valid = false;
        }
        // (an invalid path: both ends NaN, so that trial size 0 is no number either)
        double lo = valid ? 0.0 : __builtin_nan(""), hi = valid ? max_in : __builtin_nan("");
        double bx = lo, by = lo, bg = lo;
        bool any_nan = false;
        for (int r = 0; r < rounds; ++r) {
            const double x = size_trial(lo, hi, j);
            double y = x;
            for (int k = 0; k < nh; ++k) y = path_step<false>(a.p, (int64_t)k * a.p.count + p, y);
            const double g = size_gain(vi, vo, x, y);
            // the arg-max: after six exchanges every lane holds the same (bg, bj)
            bg = g;
            int bj = j;
            for (int m = 1; m < CFMM_SIZE_POINTS; m <<= 1) {
                const double og = __shfl_xor(bg, m, CFMM_SIZE_POINTS);
                const int oj = __shfl_xor(bj, m, CFMM_SIZE_POINTS);
                if (size_better(og, oj, bg, bj)) {
                    bg = og;
                    bj = oj;
                }
            }
            any_nan = any_nan || bg != bg;
            lo = __shfl(x, size_left(bj), CFMM_SIZE_POINTS);
            hi = __shfl(x, size_right(bj), CFMM_SIZE_POINTS);
            bx = __shfl(x, bj, CFMM_SIZE_POINTS);
            by = __shfl(y, bj, CFMM_SIZE_POINTS);
        }
        if (j == 0) {
            const SizeAnswer s = size_answer(any_nan, max_in, bx, by, bg);
            a.p.answer[p] = s.amount_in;
            a.amount_out[p] = s.amount_out;
            a.gain[p] = s.gain;
            a.status[p] = s.status;
        }
    }
}

} // namespace cfmm

// (what came after this header is included from here, behind everything above: find_path_kernels.h's rule)
#include "split_paths_kernels.h"
