// quote_kernels.h -- cfmm_quote / cfmm_quote_dev and cfmm_quote_out / cfmm_quote_out_dev: exact-input and exact-output swap
// quotes (quote_pool.h) of one segment, ONE LANE PER QUERY, grid-stride over the queries.  A read-only gather: per query the
// lane reads 8-24 bytes of query (coin_in, the amount, and coin_out / idx where given), the pool's record from the segment's
// own streams, and writes 8 bytes.  Nothing is staged in LDS (there are no prices), the kernel keeps no state, and the fee
// comes from where the segment keeps it (the gamma array of the two-coin kinds, UniV3Pools::pg, NCoinPools::glg).  Dense calls
// (idx == null: query q is row q) read every pool stream coalesced, exactly as the sweep does; sparse calls gather.
// The two directions are ONE body: quote_any<KIND, OUT> reads the pool and calls quote_X (OUT false: the amount out of `amt`
// in) or quote_out_X (OUT true: the amount to tender for `amt` out) -- QuoteArgs::amount_in carries the amount GIVEN,
// ::amount_out the answer.  A query whose row, coins or amount are out of range gets NaN by the rule of query_read.h.
#pragma once

#include "../../include/cfmm_amd.h"
#include "query_read.h"
#include "quote_pool.h"

namespace cfmm {

// Σ_k log R_k of Curve pool `row`: the coin count is a template argument behind the segment-uniform switch of sweep_ncoin
template <int N>
__device__ __forceinline__ double quote_sum_logs(const double* q, int64_t m, int64_t row)
{
    double lr[N];
#pragma unroll
    for (int k = 0; k < N; ++k) lr[k] = q[(int64_t)k * m + row];   // N independent loads, then the sum in coin order
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) s += lr[k];
    return s;
}

template <int KIND, bool OUT>
__device__ __forceinline__ double quote_any(const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, int64_t row, int ci,
                                            int co, double amt)
{
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        const double2 R = a.R[row];
        const double g = a.gamma[row];
        const double Ri = ci == 0 ? R.x : R.y, Ro = co == 0 ? R.x : R.y;
        if constexpr (KIND == CFMM_KIND_GEOMEAN) {
            const double2 w = a.w[row];
            if constexpr (OUT) return quote_out_weighted(Ri, Ro, ci == 0 ? w.x : w.y, co == 0 ? w.x : w.y, g, amt);
            else return quote_weighted(Ri, Ro, ci == 0 ? w.x : w.y, co == 0 ? w.x : w.y, g, amt);
        } else if constexpr (KIND == CFMM_KIND_SOLIDLY) {
            if constexpr (OUT) return quote_out_solidly(Ri, Ro, g, amt);
            else return quote_solidly(Ri, Ro, g, amt);
        } else {
            if constexpr (OUT) return quote_out_product(Ri, Ro, g, amt);
            else return quote_product(Ri, Ro, g, amt);
        }
    } else if constexpr (KIND == CFMM_KIND_UNIV3) {
        if constexpr (OUT) return quote_out_univ3(u.cur_a[row], u.cur_b[row], u.cur_c[row], u.curR[row], u.walk[row], u.ticks, u.pg[row].y, ci, amt);
        else return quote_univ3(u.cur_a[row], u.cur_b[row], u.cur_c[row], u.curR[row], u.walk[row], u.ticks, u.pg[row].y, ci, amt);
    } else {
        // coin-major columns: coin k of pool i at k·m + i
        const int64_t m = a.m;
        const double Ri = n.R[(int64_t)ci * m + row], Ro = n.R[(int64_t)co * m + row];
        const double g = n.glg[row].x;
        if constexpr (KIND == CFMM_KIND_WEIGHTED) {   // (nothing here depends on the coin count: no switch)
            if constexpr (OUT) return quote_out_weighted(Ri, Ro, n.par[(int64_t)ci * m + row], n.par[(int64_t)co * m + row], g, amt);
            else return quote_weighted(Ri, Ro, n.par[(int64_t)ci * m + row], n.par[(int64_t)co * m + row], g, amt);
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
            if constexpr (OUT) return quote_out_curve(Ri, Ro, srho, ab.x, ab.y, g, amt);
            else return quote_curve(Ri, Ro, srho, ab.x, ab.y, g, amt);
        }
    }
}

// the names the swap kernels and path_hop call the two directions by
template <int KIND>
__device__ __forceinline__ double quote_one(const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, int64_t row, int ci,
                                            int co, double amt) { return quote_any<KIND, false>(a, u, n, row, ci, co, amt); }
template <int KIND>
__device__ __forceinline__ double quote_out_one(const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, int64_t row, int ci,
                                                int co, double amt) { return quote_any<KIND, true>(a, u, n, row, ci, co, amt); }

template <int KIND, bool OUT>
__device__ __forceinline__ void quote_body(const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n)
{
    const int64_t step = (int64_t)gridDim.x * kQuoteBlock;
    for (int64_t q = (int64_t)blockIdx.x * kQuoteBlock + threadIdx.x; q < a.count; q += step) {
        const Query r = read_query(a, q);
        const double answer = quote_any<KIND, OUT>(a, u, n, r.row, r.ci, r.co, r.ok ? r.amt : 0.0);
        a.amount_out[q] = r.ok ? answer : __builtin_nan("");
    }
}

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void quote_kernel(QuoteArgs a, UniV3Pools u, NCoinPools n) { quote_body<KIND, false>(a, u, n); }

template <int KIND>
__global__ __launch_bounds__(kQuoteBlock) void quote_out_kernel(QuoteArgs a, UniV3Pools u, NCoinPools n) { quote_body<KIND, true>(a, u, n); }

} // namespace cfmm
