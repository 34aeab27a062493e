// split_grid.h -- internal, host AND device, HIP-free: the arithmetic of cfmm_split_paths' search (the contract:
// include/cfmm_amd_split.h) -- the grid points of a round, the order the greedy compares increments in, the greedy's 63 steps,
// the step back and the answer / status rule.  ONE TEXT for the kernel (split_paths_kernels.h), for the parent path of a
// multi-device context (abi_split_paths.cpp) and for the stand-alone host program of the tests
// (tests/native/split_checks_host.cpp), so the three cannot differ in a rounding or in a tie.  Every operation is rounded on
// its own: the translation units are compiled with -ffp-contract=off, and nothing here is written as a fused form.
#pragma once

#include "../../include/cfmm_amd_split.h"

#ifdef __HIP__   /* the device translation unit */
#define CFMM_SPLIT_HD __host__ __device__
#else
#define CFMM_SPLIT_HD
#endif

namespace cfmm {

// the slice of a round: rem / 63
CFMM_SPLIT_HD inline double split_slice(double rem) { return rem / (double)(CFMM_SPLIT_POINTS - 1); }

// grid point j of a path whose share so far is base: base + s * j (the product, then the sum) below the last point, which is
// base + rem -- the whole remainder, not 63 rounded slices of it.  A NaN remainder gives NaN.
CFMM_SPLIT_HD inline double split_point(double base, double s, double rem, int j)
{
    if (j >= CFMM_SPLIT_POINTS - 1) return base + rem;
    const double d = s * (double)j;
    return base + d;
}

// the total order of the greedy's arg-max over (increment, path): a larger increment first, compared as numbers
// (+0.0 == -0.0); then the smaller path; a NaN behind every number (among NaNs the smaller path)
CFMM_SPLIT_HD inline bool split_better(double d1, int k1, double d2, int k2)
{
    const bool n1 = d1 != d1, n2 = d2 != d2;
    if (n1 || n2) return n1 == n2 ? k1 < k2 : n2;
    return d1 > d2 || (d1 == d2 && k1 < k2);
}

// v[k] and v[k] = x for a k known only when the code runs, WITHOUT indexing the array by a variable: eight selects on constant
// indices, written out, so that on the device an array of per-path values is eight registers and never memory (the kernel's
// resource report shows no scratch and no LDS; with v[i] read inside the conditional it showed 144 bytes and 8 KiB)
static_assert(CFMM_MAX_SPLIT_PATHS == 8, "split_get / split_set / split_greedy are written out for eight paths");
template <class T>
CFMM_SPLIT_HD inline T split_get(const T (&v)[CFMM_MAX_SPLIT_PATHS], int k)
{
    // (every element is read first, unconditionally: a read inside a branch on k becomes one read through a selected address)
    const T v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5], v6 = v[6], v7 = v[7];
    T r = v0;
    r = k == 1 ? v1 : r;
    r = k == 2 ? v2 : r;
    r = k == 3 ? v3 : r;
    r = k == 4 ? v4 : r;
    r = k == 5 ? v5 : r;
    r = k == 6 ? v6 : r;
    r = k == 7 ? v7 : r;
    return r;
}
template <class T>
CFMM_SPLIT_HD inline void split_set(T (&v)[CFMM_MAX_SPLIT_PATHS], int k, T x)
{
    const T v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5], v6 = v[6], v7 = v[7];
    v[0] = k == 0 ? x : v0;
    v[1] = k == 1 ? x : v1;
    v[2] = k == 2 ? x : v2;
    v[3] = k == 3 ? x : v3;
    v[4] = k == 4 ? x : v4;
    v[5] = k == 5 ? x : v5;
    v[6] = k == 6 ? x : v6;
    v[7] = k == 7 ? x : v7;
}

// a step's candidate k: it replaces (db, best) where it is one of the order's paths and better
CFMM_SPLIT_HD inline void split_consider(int K, int k, double dk, double& db, int& best)
{
    if (k < K && split_better(dk, k, db, best)) {
        db = dk;
        best = k;
    }
}

// One round's greedy: 63 slices handed out one by one, each to the path whose next increment
//     inc(k, n_k) = y[k][n_k + 1] - y[k][n_k]
// is the best under split_better.  n[k] (k < K) receives the slices of path k; they sum to 63.  Returns kSplitStepNan: some
// step had no increment that is a number (it still hands its slice to path 0, so the instructions do not depend on the
// data); kSplitStepFlat: some step took an increment that is a number but not > 0.  `inc` is asked for a path's increment
// once per slice it receives, at (k, n) with n <= 62; paths at k >= K are never asked for.
constexpr int kSplitStepNan = 1, kSplitStepFlat = 2;
template <class INC>
CFMM_SPLIT_HD inline int split_greedy(int K, const INC& inc, int (&n)[CFMM_MAX_SPLIT_PATHS])
{
    double d[CFMM_MAX_SPLIT_PATHS];
    for (int k = 0; k < CFMM_MAX_SPLIT_PATHS; ++k) {
        n[k] = 0;
        d[k] = k < K ? inc(k, 0) : __builtin_nan("");
    }
    int flags = 0;
    for (int t = 0; t < CFMM_SPLIT_POINTS - 1; ++t) {
        int best = 0;
        double db = d[0];
        split_consider(K, 1, d[1], db, best);
        split_consider(K, 2, d[2], db, best);
        split_consider(K, 3, d[3], db, best);
        split_consider(K, 4, d[4], db, best);
        split_consider(K, 5, d[5], db, best);
        split_consider(K, 6, d[6], db, best);
        split_consider(K, 7, d[7], db, best);
        if (db != db) flags |= kSplitStepNan;
        else if (!(db > 0.0)) flags |= kSplitStepFlat;
        const int nb = split_get(n, best) + 1;
        split_set(n, best, nb);
        if (t < CFMM_SPLIT_POINTS - 2) split_set(d, best, inc(best, nb));
    }
    return flags;
}

// the step back between rounds: the grid point a share restarts from
CFMM_SPLIT_HD inline int split_back(int n) { return n > 0 ? n - 1 : 0; }
// ... and what is left to hand out, given the sum of the restarted shares in increasing k
CFMM_SPLIT_HD inline double split_rem(double amount, double base_sum)
{
    const double r = amount - base_sum;
    return r < 0.0 ? 0.0 : r;   // (a NaN stays one)
}

// an amount the search can start from: finite and >= 0
CFMM_SPLIT_HD inline bool split_amount_ok(double a) { return a >= 0.0 && a < __builtin_inf(); }

// The status of an order from what its rounds reported.  any_nan: a step of some round had no increment that is a number;
// last_flat: a step of the LAST round took an increment that is not > 0; total: y_0 + y_1 + ... in increasing k.  A total
// that is no number is CFMM_SPLIT_NAN as well: a path that quotes NaN everywhere (a bad hop of a device-pointer call) never
// receives a slice, but its output, and so the total, is NaN.
// CFMM_SPLIT_NAN writes NaN over the order's outputs, CFMM_SPLIT_NONE +0.0 (split_written).
CFMM_SPLIT_HD inline int32_t split_status(bool any_nan, bool last_flat, double amount, double total)
{
    if (any_nan || total != total) return CFMM_SPLIT_NAN;
    if (amount == 0.0 || !(total > 0.0)) return CFMM_SPLIT_NONE;
    return last_flat ? CFMM_SPLIT_SATURATED : CFMM_SPLIT_OK;
}
CFMM_SPLIT_HD inline double split_written(int32_t status, double v)
{
    return status == CFMM_SPLIT_NAN ? __builtin_nan("") : (status == CFMM_SPLIT_NONE ? 0.0 : v);
}

} // namespace cfmm
