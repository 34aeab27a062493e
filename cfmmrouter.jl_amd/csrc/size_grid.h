// size_grid.h -- internal, host AND device, HIP-free: the arithmetic of cfmm_size_path's bracketing search (the contract:
// include/cfmm_amd_size_path.h) -- the trial sizes of a round, the gain of one, the order the arg-max is taken in, the next
// bracket and the status.  ONE TEXT for the kernel (size_path_kernels.h), for the parent path of a multi-device context
// (abi_size_path.cpp) and for the stand-alone host program of the tests (tests/native/size_checks_host.cpp), so the three
// cannot differ in a rounding.  Every operation is rounded on its own: the translation units are compiled with
// -ffp-contract=off, and nothing here is written as a fused form.
#pragma once

#include "../../include/cfmm_amd_size_path.h"

#ifdef __HIP__   /* the device translation unit */
#define CFMM_SIZE_HD __host__ __device__
#else
#define CFMM_SIZE_HD
#endif

namespace cfmm {

// trial size j of the bracket [lo, hi]: the two ends exactly, min(lo + (hi - lo) * (j / 63), hi) between them -- never above
// hi, and non-decreasing in j (a product by a larger correctly rounded factor is never smaller).  A NaN end gives NaN.
CFMM_SIZE_HD inline double size_trial(double lo, double hi, int j)
{
    if (j <= 0) return lo;
    if (j >= CFMM_SIZE_POINTS - 1) return hi;
    const double t = (double)j / (double)(CFMM_SIZE_POINTS - 1);
    const double w = hi - lo;
    const double d = w * t;
    const double x = lo + d;
    return x < hi ? x : hi;
}

// gain of tendering x for y: value_out * y - value_in * x, a product, a product and a difference
CFMM_SIZE_HD inline double size_gain(double value_in, double value_out, double x, double y)
{
    const double a = value_out * y;
    const double b = value_in * x;
    return a - b;
}

// the total order of the arg-max over (gain, trial index): a larger gain first, compared as numbers (+0.0 == -0.0); then the
// smaller index; a NaN behind every number (among NaNs the smaller index).  Total, so a reduction in any order ends at the
// same pair.
CFMM_SIZE_HD inline bool size_better(double g1, int j1, double g2, int j2)
{
    const bool n1 = g1 != g1, n2 = g2 != g2;
    if (n1 || n2) return n1 == n2 ? j1 < j2 : n2;
    return g1 > g2 || (g1 == g2 && j1 < j2);
}

// the neighbours of the winner, whose trial sizes are the next bracket
CFMM_SIZE_HD inline int size_left(int j) { return j > 0 ? j - 1 : 0; }
CFMM_SIZE_HD inline int size_right(int j) { return j < CFMM_SIZE_POINTS - 1 ? j + 1 : CFMM_SIZE_POINTS - 1; }

// a limit or a value the search can start from: max_amount_in finite and >= 0, a value finite and > 0
CFMM_SIZE_HD inline bool size_limit_ok(double max_in) { return max_in >= 0.0 && max_in < __builtin_inf(); }
CFMM_SIZE_HD inline bool size_value_ok(double v) { return v > 0.0 && v < __builtin_inf(); }

// What the last round's winner (x, y, g) becomes.  any_nan: some round had no trial size whose gain is a number.
struct SizeAnswer {
    double amount_in, amount_out, gain;
    int32_t status;
};
CFMM_SIZE_HD inline SizeAnswer size_answer(bool any_nan, double max_in, double x, double y, double g)
{
    if (any_nan) {
        const double nan = __builtin_nan("");
        return {nan, nan, nan, CFMM_SIZED_NAN};
    }
    if (!(g > 0.0)) return {0.0, 0.0, 0.0, CFMM_SIZED_NONE};
    return {x, y, g, x == max_in ? CFMM_SIZED_AT_LIMIT : CFMM_SIZED};
}

} // namespace cfmm
