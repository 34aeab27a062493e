// split_search.h -- internal, host only, HIP-free: the search a multi-device parent runs on the host where a single context
// runs a kernel (abi_split_paths.cpp, abi_size_path.cpp).  Per round the 64 grid points of every path (point j of path p is
// path j*n_paths + p of the inner call, whose hop arrays -- GridPaths -- repeat the call's 64 times) are quoted in ONE call of
// a path-quoting entry; the rest is split_grid.h / split_out_grid.h, the text the kernels compile, so the answers are the same
// bits.  The quote is a callable (N, x, y) -> rc: a context passes cfmm_quote_path / cfmm_quote_path_out over GridPaths, a
// stand-alone program (tests/native/path_rig_host.cpp) a closed form.
#pragma once

#include "../../include/cfmm_amd_size_path.h"
#include "split_out_grid.h"

#include <cstring>
#include <vector>

namespace cfmm {

static_assert(CFMM_SIZE_POINTS == CFMM_SPLIT_POINTS, "one grid of paths serves both searches");

struct GridPaths {   // the call's hop arrays, 64 times
    std::vector<int32_t> nh, seg, cin, cot;
    std::vector<int64_t> row;
    GridPaths(int64_t n_paths, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* ci,
              const int32_t* co)
    {
        constexpr size_t J = CFMM_SPLIT_POINTS;
        const size_t n = (size_t)n_paths, H = (size_t)max_hops, N = J * n;
        nh.resize(N), seg.resize(H * N), cin.resize(H * N), cot.resize(H * N), row.resize(H * N);
        for (size_t j = 0; j < J; ++j) {
            std::memcpy(&nh[j * n], n_hops, n * sizeof(int32_t));
            for (size_t k = 0; k < H; ++k) {
                std::memcpy(&seg[k * N + j * n], hop_seg + k * n, n * sizeof(int32_t));
                std::memcpy(&row[k * N + j * n], hop_row + k * n, n * sizeof(int64_t));
                std::memcpy(&cin[k * N + j * n], ci + k * n, n * sizeof(int32_t));
                std::memcpy(&cot[k * N + j * n], co + k * n, n * sizeof(int32_t));
            }
        }
    }
};

// What the two directions of the split differ in: what a round's greedy reports and folds into the order's state, the status
// and the written values.  x is what is spread (cfmm_split_paths: path_amount_in; _out: the shares of the wanted output), y
// what the quote answers for it (path_amount_out; the costs).
struct SplitIn {
    struct State { bool any_nan = false, last_flat = false; };
    template <class INC>
    static void fold(State& s, int K, const INC& inc, int (&cnt)[CFMM_MAX_SPLIT_PATHS])
    {
        const int flags = split_greedy(K, inc, cnt);
        s.any_nan = s.any_nan || (flags & kSplitStepNan) != 0;
        s.last_flat = (flags & kSplitStepFlat) != 0;
    }
    static int32_t status(const State& s, double amount, double total) { return split_status(s.any_nan, s.last_flat, amount, total); }
    static double written_x(int32_t st, double v) { return split_written(st, v); }
    static double written_y(int32_t st, double v) { return split_written(st, v); }
};
struct SplitOut {
    struct State { int bad = kSplitOutClean; };
    template <class INC>
    static void fold(State& s, int K, const INC& inc, int (&cnt)[CFMM_MAX_SPLIT_PATHS]) { s.bad = split_out_greedy(K, inc, cnt, s.bad); }
    static int32_t status(const State& s, double amount, double total) { return split_out_status(s.bad, amount, total); }
    static double written_x(int32_t st, double v) { return split_out_written_share(st, v); }
    static double written_y(int32_t st, double v) { return split_out_written_cost(st, v); }
};

// `rounds` quotes of 64 x n_paths amounts, the greedy order by order.  Everything was checked by the caller; the answers are
// written only when every quote has succeeded (a failing quote's rc is returned, the message is the inner call's).
template <class Way, class Quote>
int split_search(const Quote& quote, int64_t count, const int64_t* order_first, const double* amount, int64_t n_paths, int32_t rounds,
                 double* path_x, double* path_y, double* total_y, int32_t* status)
{
    constexpr size_t J = CFMM_SPLIT_POINTS;
    const size_t n = (size_t)n_paths, N = J * n, G = (size_t)count;
    std::vector<double> base(n, 0.0), rem(amount, amount + G), x(N), y(N);
    std::vector<int> slices(n, 0);
    std::vector<typename Way::State> state(G);
    for (int r = 0; r < rounds; ++r) {
        for (size_t g = 0; g < G; ++g) {
            const double s = split_slice(rem[g]);
            for (size_t p = (size_t)order_first[g]; p < (size_t)order_first[g + 1]; ++p)
                for (size_t j = 0; j < J; ++j) x[j * n + p] = split_point(base[p], s, rem[g], (int)j);
        }
        if (const int rc = quote((int64_t)N, x.data(), y.data())) return rc;
        for (size_t g = 0; g < G; ++g) {
            const size_t first = (size_t)order_first[g];
            const int K = (int)(order_first[g + 1] - order_first[g]);
            int cnt[CFMM_MAX_SPLIT_PATHS];
            Way::fold(state[g], K, [&](int k, int at) { return y[(size_t)(at + 1) * n + first + (size_t)k] - y[(size_t)at * n + first + (size_t)k]; }, cnt);
            for (int k = 0; k < K; ++k) slices[first + (size_t)k] = cnt[k];
            if (r + 1 < rounds) {
                double sum = 0.0;
                for (int k = 0; k < K; ++k) {
                    const size_t p = first + (size_t)k;
                    base[p] = x[(size_t)split_back(cnt[k]) * n + p];
                    sum = k == 0 ? base[p] : sum + base[p];
                }
                rem[g] = split_rem(amount[g], sum);
            }
        }
    }
    for (size_t g = 0; g < G; ++g) {
        const size_t first = (size_t)order_first[g];
        const int K = (int)(order_first[g + 1] - order_first[g]);
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            const double yk = y[(size_t)slices[first + (size_t)k] * n + first + (size_t)k];
            total = k == 0 ? yk : total + yk;
        }
        const int32_t st = Way::status(state[g], amount[g], total);
        for (int k = 0; k < K; ++k) {
            const size_t p = first + (size_t)k, at = (size_t)slices[p] * n + p;
            path_x[p] = Way::written_x(st, x[at]);
            path_y[p] = Way::written_y(st, y[at]);
        }
        total_y[g] = Way::written_y(st, total);
        status[g] = st;
    }
    return CFMM_OK;
}

} // namespace cfmm
