// split_out_grid.h -- internal, host AND device, HIP-free: what cfmm_split_paths_out's search (the contract:
// include/cfmm_amd_split_out.h) has of its own besides split_grid.h -- the order the greedy compares increments in (the
// SMALLEST cost first), the greedy's 63 steps with the first-bad-step rule, and the answer / status rule.  The grid points, the
// step back, the remainder and the amount test are split_grid.h's (split_slice, split_point, split_back, split_rem,
// split_amount_ok), laid over the output.  ONE TEXT for the kernel (split_paths_out_kernels.h), for the parent path of a
// multi-device context (abi_split_paths.cpp) and for the stand-alone host program of the tests
// (tests/native/split_out_checks_host.cpp).  Nothing of split_grid.h changes: what cfmm_split_paths compiles to is as it was.
#pragma once

#include "../../include/cfmm_amd_split_out.h"
#include "split_grid.h"

namespace cfmm {

// the total order of the greedy's arg-min over (increment, path): a smaller increment first, compared as numbers
// (+0.0 == -0.0, and +inf is a number); then the smaller path; a NaN behind every number (among NaNs the smaller path)
CFMM_SPLIT_HD inline bool split_out_better(double d1, int k1, double d2, int k2)
{
    const bool n1 = d1 != d1, n2 = d2 != d2;
    if (n1 || n2) return n1 == n2 ? k1 < k2 : n2;
    return d1 < d2 || (d1 == d2 && k1 < k2);
}

CFMM_SPLIT_HD inline void split_out_consider(int K, int k, double dk, double& db, int& best)
{
    if (k < K && split_out_better(dk, k, db, best)) {
        db = dk;
        best = k;
    }
}

// What the FIRST step, in round and step order, whose taken increment is not finite was: nothing yet, an infinity (no path
// can give another slice), or no number.  Steps behind it do not count: behind a +inf step the path that took it shows
// inf - inf, which says nothing about the paths.
constexpr int kSplitOutClean = 0, kSplitOutInf = 1, kSplitOutNan = 2;

// One round's greedy: 63 slices handed out one by one, each to the path whose next increment
//     inc(k, n_k) = c[k][n_k + 1] - c[k][n_k]
// is the best under split_out_better.  n[k] (k < K) receives the slices of path k; they sum to 63.  `bad` is what the rounds
// before reported (kSplitOut*); returned is the same where it was not clean, and otherwise what this round's first step with a
// taken increment that is not finite was.  Every step runs whatever the steps before it took (a step without a number hands
// its slice to path 0), so the instructions do not depend on the data.  `inc` is asked as split_greedy asks it.
template <class INC>
CFMM_SPLIT_HD inline int split_out_greedy(int K, const INC& inc, int (&n)[CFMM_MAX_SPLIT_PATHS], int bad)
{
    double d[CFMM_MAX_SPLIT_PATHS];
    for (int k = 0; k < CFMM_MAX_SPLIT_PATHS; ++k) {
        n[k] = 0;
        d[k] = k < K ? inc(k, 0) : __builtin_nan("");
    }
    for (int t = 0; t < CFMM_SPLIT_POINTS - 1; ++t) {
        int best = 0;
        double db = d[0];
        split_out_consider(K, 1, d[1], db, best);
        split_out_consider(K, 2, d[2], db, best);
        split_out_consider(K, 3, d[3], db, best);
        split_out_consider(K, 4, d[4], db, best);
        split_out_consider(K, 5, d[5], db, best);
        split_out_consider(K, 6, d[6], db, best);
        split_out_consider(K, 7, d[7], db, best);
        const bool finite = db < __builtin_inf() && db > -__builtin_inf();   // (false of a NaN)
        const int now = finite ? kSplitOutClean : (db != db ? kSplitOutNan : kSplitOutInf);
        bad = bad == kSplitOutClean ? now : bad;
        const int nb = split_get(n, best) + 1;
        split_set(n, best, nb);
        if (t < CFMM_SPLIT_POINTS - 2) split_set(d, best, inc(best, nb));
    }
    return bad;
}

// The status of an order from what its rounds reported.  bad: split_out_greedy's, through all rounds; total: c_0 + c_1 + ...
// in increasing k.  A total that is no number with no bad step is CFMM_SPLIT_NAN as well: a path that quotes NaN everywhere
// never receives a slice, but its cost, and so the total, is NaN.
CFMM_SPLIT_HD inline int32_t split_out_status(int bad, double amount, double total)
{
    if (bad == kSplitOutInf) return CFMM_SPLIT_UNOBTAINABLE;
    if (bad == kSplitOutNan || total != total) return CFMM_SPLIT_NAN;
    return amount == 0.0 ? CFMM_SPLIT_NONE : CFMM_SPLIT_OK;
}
// what is written for a share (path_amount_out) ...
CFMM_SPLIT_HD inline double split_out_written_share(int32_t status, double v)
{
    return status == CFMM_SPLIT_NAN ? __builtin_nan("") : (status == CFMM_SPLIT_OK ? v : 0.0);
}
// ... and for a cost (path_amount_in, total_in)
CFMM_SPLIT_HD inline double split_out_written_cost(int32_t status, double v)
{
    if (status == CFMM_SPLIT_UNOBTAINABLE) return __builtin_inf();
    return status == CFMM_SPLIT_NAN ? __builtin_nan("") : (status == CFMM_SPLIT_OK ? v : 0.0);
}

} // namespace cfmm
