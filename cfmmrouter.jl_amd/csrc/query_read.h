// query_read.h -- how a query kernel reads a query: the one statement of the refusal rule.  The device-pointer entries
// (cfmm_quote_dev, cfmm_quote_path_dev, cfmm_size_path_dev) take unchecked arrays, so NOTHING a query names is trusted, and
// the order below is the contract:
//   1. TEST   ok = the row, both coins (and, for a hop, the segment) lie in range, the coins differ, the amount is a
//             finite number >= 0;
//   2. CLAMP  every index is forced into its range, whatever the test said;
//   3. READ   pool state is read only through the clamped indices -- an invalid query quotes SOME pool of the segment;
//   4. POISON the caller answers NaN where !ok (and evaluates with amount 0, so that no formula sees a bad number).
// The kernels therefore never read or write out of bounds.  One reader per query shape: read_query for the single-pool
// entries (a QuoteArgs), read_hop for the path entries (a PathArgs or a SwapPathArgs).
#pragma once

#include <type_traits>

#include "sweep.h"

namespace cfmm {

__device__ __forceinline__ int clamp_coin(int c, int n) { return c < 0 ? 0 : (c >= n ? n - 1 : c); }

struct Query {
    long long row;
    int ci, co;
    double amt;   // as given: the caller evaluates with ok ? amt : 0.0
    bool ok;
};

// query q of a: its row (idx, or q itself), coin_in, coin_out (or 1 - coin_in) and amount
__device__ __forceinline__ Query read_query(const QuoteArgs& a, int64_t q)
{
    long long row = a.idx ? a.idx[q] : (long long)q;
    int ci = a.coin_in[q];
    int co = a.coin_out ? a.coin_out[q] : 1 - ci;
    const double amt = a.amount_in[q];
    const bool ok = row >= 0 && row < a.m && ci >= 0 && ci < a.n_coins && co >= 0 && co < a.n_coins && ci != co &&
                    amt >= 0.0 && amt < __builtin_inf();
    row = row < 0 ? 0 : (row >= a.m ? a.m - 1 : row);
    ci = clamp_coin(ci, a.n_coins);
    co = clamp_coin(co, a.n_coins);
    return Query{row, ci, co, amt, ok};
}

// the quotes' view of a record of either segment table
__device__ __forceinline__ const PathSeg& quote_view(const PathSeg& s) { return s; }
__device__ __forceinline__ const PathSeg& quote_view(const SwapPathSeg& t) { return t.s; }

template <class SEG>
struct Hop {
    const SEG& seg;   // the record of the (clamped) segment, its kind and its pools
    int kind;
    int64_t m;
    long long row;
    int ci, co;
    double amt;       // ok ? the amount given : 0.0
    bool ok;
};

// hop `at` (= k*stride + p) of the hop-major arrays of a, entered with (or asked for) amt.  A segment without pools has kind
// -1 and m 0: with_kind runs no body on it, so the row clamped to -1 is never used.
template <class ARGS>
__device__ __forceinline__ auto read_hop(const ARGS& a, int64_t at, double amt)
{
    using SEG = std::remove_cv_t<std::remove_pointer_t<decltype(a.segs)>>;
    int seg = a.hop_seg[at];
    long long row = a.hop_row[at];
    int ci = a.hop_coin_in[at];
    int co = a.hop_coin_out[at];
    bool ok = seg >= 0 && seg < a.nseg;
    seg = seg < 0 ? 0 : (seg >= a.nseg ? a.nseg - 1 : seg);
    const SEG& t = a.segs[seg];
    const int kind = quote_view(t).kind;
    const int nc = quote_view(t).n_coins;
    const int64_t m = quote_view(t).m;
    ok = ok && row >= 0 && row < m && ci >= 0 && ci < nc && co >= 0 && co < nc && ci != co && amt >= 0.0 && amt < __builtin_inf();
    row = row < 0 ? 0 : (row >= m ? m - 1 : row);
    ci = clamp_coin(ci, nc);
    co = clamp_coin(co, nc);
    return Hop<SEG>{t, kind, m, row, ci, co, ok ? amt : 0.0, ok};
}

} // namespace cfmm
