// rate_kernels.h -- cfmm_quote_rate / cfmm_quote_rate_dev and cfmm_quote_path_rate / cfmm_quote_path_rate_dev: the exact-input
// quote of quote_kernels.h / quote_path_kernels.h AND its marginal rate (rate_pool.h) from one read of the pool, ONE LANE PER
// QUERY (per path), grid-stride.  The amounts are quote_any<KIND, false>'s own -- the same function on the same operands, so
// amount_out and hop_out carry cfmm_quote's and cfmm_quote_path's bits -- and the rate reads the pool exactly as the quote does
// (the same addresses: the compiler keeps one load of each).  A read-only gather with two 8-byte stores per query; nothing
// is staged in LDS, no atomics, no state.  The refusal rule is query_read.h's: a bad query gets NaN in BOTH outputs.
#pragma once

#include "../../include/cfmm_amd.h"
#include "kind_switch.h"
#include "query_read.h"
#include "quote_kernels.h"
#include "quote_path_kernels.h"
#include "rate_pool.h"

namespace cfmm {

template <int KIND>
__device__ __forceinline__ double rate_any(const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, int64_t row, int ci, int co,
                                           double amt)
{
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        const double2 R = a.R[row];
        const double g = a.gamma[row];
        const double Ri = ci == 0 ? R.x : R.y, Ro = co == 0 ? R.x : R.y;
        if constexpr (KIND == CFMM_KIND_GEOMEAN) {
            const double2 w = a.w[row];
            return rate_weighted(Ri, Ro, ci == 0 ? w.x : w.y, co == 0 ? w.x : w.y, g, amt);
        } else if constexpr (KIND == CFMM_KIND_SOLIDLY) {
            return rate_solidly(Ri, Ro, g, amt);
        } else {
            return rate_product(Ri, Ro, g, amt);
        }
    } else if constexpr (KIND == CFMM_KIND_UNIV3) {
        return rate_univ3(u.cur_a[row], u.cur_b[row], u.cur_c[row], u.curR[row], u.walk[row], u.ticks, u.pg[row].y, ci, amt);
    } else {
        // coin-major columns: coin k of pool i at k·m + i
        const int64_t m = a.m;
        const double Ri = n.R[(int64_t)ci * m + row], Ro = n.R[(int64_t)co * m + row];
        const double g = n.glg[row].x;
        if constexpr (KIND == CFMM_KIND_WEIGHTED) {
            return rate_weighted(Ri, Ro, n.par[(int64_t)ci * m + row], n.par[(int64_t)co * m + row], g, amt);
        } else {
            const double2 ab = reinterpret_cast<const double2*>(n.par)[row];   // {α, log β}
            double srho;
            switch (n.n_coins) {
            case 2: srho = quote_sum_logs<2>(n.q, m, row); break;
            case 3: srho = quote_sum_logs<3>(n.q, m, row); break;
            case 4: srho = quote_sum_logs<4>(n.q, m, row); break;
            case 5: srho = quote_sum_logs<5>(n.q, m, row); break;
            case 6: srho = quote_sum_logs<6>(n.q, m, row); break;
            case 7: srho = quote_sum_logs<7>(n.q, m, row); break;
            default: srho = quote_sum_logs<8>(n.q, m, row); break;
            }
            return rate_curve(Ri, Ro, srho, ab.x, ab.y, g, amt);
        }
    }
}

// read_query (query_read.h) of a call without amounts -- the spot-price table: the same test, clamp and order, amount 0
__device__ __forceinline__ Query read_spot_query(const QuoteArgs& a, int64_t q)
{
    long long row = a.idx ? a.idx[q] : (long long)q;
    int ci = a.coin_in[q];
    int co = a.coin_out ? a.coin_out[q] : 1 - ci;
    const bool ok = row >= 0 && row < a.m && ci >= 0 && ci < a.n_coins && co >= 0 && co < a.n_coins && ci != co;
    row = row < 0 ? 0 : (row >= a.m ? a.m - 1 : row);
    ci = clamp_coin(ci, a.n_coins);
    co = clamp_coin(co, a.n_coins);
    return Query{row, ci, co, 0.0, ok};
}

// r.q.amount_in null: every amount is 0 (a uniform branch); r.q.amount_out may be null exactly then
template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void rate_kernel(RateArgs r, UniV3Pools u, NCoinPools n)
{
    const QuoteArgs& a = r.q;
    const bool spot = a.amount_in == nullptr;
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        const Query s = spot ? read_spot_query(a, q) : read_query(a, q);
        const double amt = s.ok ? s.amt : 0.0;
        const double out = quote_any<KIND, false>(a, u, n, s.row, s.ci, s.co, amt);
        const double rate = rate_any<KIND>(a, u, n, s.row, s.ci, s.co, amt);
        if (a.amount_out) a.amount_out[q] = s.ok ? out : __builtin_nan("");
        r.rate[q] = s.ok ? rate : __builtin_nan("");
    }
}

// path_hop (quote_path_kernels.h) with the hop's rate beside its amount: the same views, filled the same way
template <int KIND>
__device__ __forceinline__ double path_hop_rate(const PathSeg& s, int64_t m, int64_t row, int ci, int co, double amt, double& rate)
{
    QuoteArgs q{};
    UniV3Pools u{};
    NCoinPools n{};
    q.m = m;
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        q.R = s.R;
        q.gamma = s.gamma;
        if constexpr (KIND == CFMM_KIND_GEOMEAN) q.w = s.w;
    } else if constexpr (KIND == CFMM_KIND_UNIV3) {
        u.pg = s.pg;
        u.cur_a = s.cur_a;
        u.cur_b = s.cur_b;
        u.cur_c = s.cur_c;
        u.curR = s.curR;
        u.walk = s.walk;
        u.ticks = s.ticks;
    } else {
        n.R = s.nR;
        n.q = s.nq;
        n.glg = s.nglg;
        n.par = s.npar;
        n.n_coins = s.n_coins;
    }
    rate = rate_any<KIND>(q, u, n, row, ci, co, amt);
    return quote_one<KIND>(q, u, n, row, ci, co, amt);
}

// x_0 = amount_in, x_{k+1} = quote(hop k, x_k), r_k = rate(hop k, x_k); hops[k] = x_{k+1}, hop_rate[k] = r_k, rate = the left
// fold ((r_0·r_1)·r_2)..., each product rounded on its own.  A hop of rate 0 makes the path's rate 0; the hops behind it are
// still evaluated.  The refusals are quote_path_kernel's: a bad n_hops makes the whole path NaN with no hop evaluated, a bad
// hop poisons its amount AND its rate, and both then travel through the remaining hops.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void quote_path_rate_kernel(PathRateArgs r)
{
    const PathArgs& a = r.p;
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.count; p += step) {
        int nh = a.n_hops[p];
        double x = a.given[p];
        double fold = __builtin_nan("");
        if (nh < 1 || nh > a.max_hops) {
            nh = 0;
            x = __builtin_nan("");
        }
        for (int k = 0; k < nh; ++k) {
            const int64_t at = (int64_t)k * a.count + p;
            const auto h = read_hop(a, at, x);
            const PathSeg& s = h.seg;
            bool ok = h.ok;
            double out, rk;
            with_kind(h.kind, [&](auto K) { out = path_hop_rate<decltype(K)::value>(s, h.m, h.row, h.ci, h.co, h.amt, rk); },
                      [&] { out = 0.0; rk = 0.0; ok = false; });
            x = ok ? out : __builtin_nan("");
            rk = ok ? rk : __builtin_nan("");
            fold = k == 0 ? rk : fold * rk;
            if (a.hops) a.hops[at] = x;
            if (r.hop_rate) r.hop_rate[at] = rk;
        }
        for (int k = nh; k < a.max_hops; ++k) {
            const int64_t at = (int64_t)k * a.count + p;
            if (a.hops) a.hops[at] = __builtin_nan("");
            if (r.hop_rate) r.hop_rate[at] = __builtin_nan("");
        }
        a.answer[p] = x;
        r.rate[p] = fold;
    }
}

} // namespace cfmm

#include "swap_limit_kernels.h"
