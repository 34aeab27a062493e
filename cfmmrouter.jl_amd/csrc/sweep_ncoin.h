// sweep_ncoin.h -- N-coin pools (weighted geometric mean, Curve) on the sweep's prologue and epilogue (sweep_core.h).
#pragma once

#include "curve_pool.h"
#include "sweep_core.h"

namespace cfmm {

// ---------------------------------------------------------------------------------------------
// N-coin pools: one lane per pool, coin-major columns (sweep.h NCoinPools), one launch per segment
// ---------------------------------------------------------------------------------------------
// The price of token t, from the LDS row stage_prices fills
__device__ __forceinline__ double lds_price(const SweepArgs& a, const SweepLds& L, int t)
{
    return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(L.vy) + ((size_t)t << a.v_shift));
}

// A pool inside its fee band: every Δ and Λ is +0.0
template <int N, bool MAT>
__device__ __forceinline__ void ncoin_no_trade(const NCoinPools& p, int64_t m, int64_t i)
{
    if (MAT) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            p.Delta[k * m + i] = 0.0;
            p.Lambda[k * m + i] = 0.0;
        }
    }
}

// Coin k of pool i trades (Δ, Λ) = (del, lam): stored by a materialising sweep, its terms of the dual sums, its netflow
// into this wavefront's LDS bins
template <bool MAT>
__device__ __forceinline__ void ncoin_emit(const NCoinPools& p, const SweepArgs& a, const SweepLds& L, int64_t m, int64_t i, int k,
                                           int tok, double lam, double del, double& sum_l, double& sum_d)
{
    if (MAT) {
        p.Delta[k * m + i] = del;
        p.Lambda[k * m + i] = lam;
    }
    const double v = lds_price(a, L, tok);
    sum_l += lam * v;     // src/router.jl:82  dot(Λ, v[Ai]) - dot(Δ, v[Ai])
    sum_d += del * v;
    const double f = lam - del;   // src/router.jl:99  G[Ai] .+= Λ .- Δ
    if (f != 0.0 || f != f) atomicAdd(&L.my_bins[tok], f);
}

// Weighted geometric-mean pools -- GeometricMean / Product, src/cfmms.jl:57-64 (no find_arb! there).
// maximise Σ v_k(λ_k − δ_k) s.t. Π (R_k + γδ_k − λ_k)^{w_k} >= Π R_k^{w_k}, δ, λ >= 0 (the problem of the find_arb!
// docstring, src/cfmms.jl:21-33).  With the multiplier μ = e^t the KKT conditions give, coin by coin,
//     R_k'(t) = R_k · exp(min(0, t − s_k^λ) + max(0, t − s_k^δ)),   s_k^λ = log(R_k v_k / w_k),  s_k^δ = s_k^λ − log γ,
// and t* is the root of the nondecreasing piecewise-linear G(t) = Σ w_k [min(0, t − s_k^λ) + max(0, t − s_k^δ)].
// No trade iff max s^λ <= min s^δ (the fee band: every trade is exactly +0.0).  Otherwise G is evaluated at its 2N
// breakpoints (no sort: N² clamp terms each), the root is bracketed by the largest breakpoint with G <= 0 and the smallest
// with G >= 0, and G is linear in between: t* = lo − G(lo) / slope, the slope being the summed weight of the terms live
// inside the bracket.  Trades: λ_k = −R_k·expm1(t* − s_k^λ) where t* < s_k^λ, δ_k = R_k·expm1(t* − s_k^δ) / γ where
// t* > s_k^δ.  Per pool there is no logarithm: log v is staged per token (SweepLds::lv), q_k = log(R_k / w_k) and log γ
// are prepared at upload.  N = 2 is the two-coin closed forms' problem (ProductTwoCoin at equal weights, GeometricMeanTwoCoin).
// The coin count is a template argument of the per-pool code (registers sized for exactly N) and a segment-uniform
// switch in the kernel.
template <int N, bool MAT>
__device__ __forceinline__ void weighted_pool(const NCoinPools& p, const SweepArgs& a, const SweepLds& L, int64_t i, double& acc)
{
    const int64_t m = a.m;
    double R[N], w[N], sl[N];   // (s^δ = s^λ − log γ and the prices are re-derived where needed: registers)
    int tok[N];
    const double2 gl = p.glg[i];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        R[k] = p.R[k * m + i];
        w[k] = p.par[k * m + i];
        sl[k] = p.q[k * m + i];
        tok[k] = p.tok[k * m + i];
    }
    double lmax = -__builtin_inf(), dmin = __builtin_inf(), wsum = 0.0;
    bool nan_in = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sl[k] += a.need_logv ? L.lv[tok[k]] : log(lds_price(a, L, tok[k]));
        nan_in = nan_in || sl[k] != sl[k];
        lmax = __builtin_fmax(lmax, sl[k]);
        dmin = __builtin_fmin(dmin, sl[k] - gl.y);
        wsum += w[k];
    }
    if (!nan_in && lmax <= dmin) {   // inside the fee band: no trade
        ncoin_no_trade<N, MAT>(p, m, i);
        return;
    }
    // bracket of the root of G among the 2N breakpoints
    double lo = -__builtin_inf(), glo = 0.0, hi = __builtin_inf(), ghi = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * N; ++j) {
        const double b = j < N ? sl[j] : sl[j - N] - gl.y;
        double G = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) G += w[k] * (__builtin_fmin(b - sl[k], 0.0) + __builtin_fmax(b - (sl[k] - gl.y), 0.0));
        if (G <= 0.0 && b > lo) { lo = b; glo = G; }
        if (G >= 0.0 && b < hi) { hi = b; ghi = G; }
    }
    double t;
    if (lo == -__builtin_inf()) {
        t = hi - ghi / wsum;            // below every breakpoint: every λ term live, slope Σw
    } else if (hi == __builtin_inf()) {
        t = lo - glo / wsum;            // above every breakpoint: every δ term live
    } else if (glo == 0.0 || !(lo < hi)) {
        t = glo == 0.0 ? lo : hi;       // a breakpoint is the root (or rounding crossed the bracket over)
    } else {
        const double mid = lo + 0.5 * (hi - lo);
        double slope = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) slope += (mid < sl[k] ? w[k] : 0.0) + (mid > sl[k] - gl.y ? w[k] : 0.0);
        t = slope > 0.0 ? __builtin_fmin(__builtin_fmax(lo - glo / slope, lo), hi) : lo;
    }
    if (nan_in) t = __builtin_nan("");
    const double rg = 1.0 / gl.x;
    double sum_l = 0.0, sum_d = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double lam = nan_in ? t : (t < sl[k] ? -(R[k] * expm1(t - sl[k])) : 0.0);
        const double sd = sl[k] - gl.y;
        const double del = nan_in ? t : (t > sd ? (R[k] * expm1(t - sd)) * rg : 0.0);
        ncoin_emit<MAT>(p, a, L, m, i, k, tok[k], lam, del, sum_l, sum_d);
    }
    acc += sum_l - sum_d;
}

// Curve (StableSwap) pools -- Curve{T}, src/cfmms.jl:66-70 (no find_arb! there): φ(R) = α·Σ R − β·Π R⁻¹.
// The solve (outer safeguarded Newton on E2, inner exact E1 root) is curve_pool.h's curve_solve, the derivation there.
// Prices come from the LDS row stage_prices fills (v itself: no log v row).  Trades: λ_k = −R_k·expm1(log r_k − ρ_k) for a
// coin that leaves, δ_k = R_k·expm1(log r_k − ρ_k)/γ for one that enters; a coin that does not trade has log r_k = ρ_k
// exactly, hence +0.0.
template <int N, bool MAT>
__device__ __forceinline__ void curve_pool(const NCoinPools& p, const SweepArgs& a, const SweepLds& L, int64_t i, double& acc)
{
    const int64_t m = a.m;
    double R[N], rho[N], v[N], lr[N];
    int tok[N];   // (v is re-read from LDS after the solve: fewer registers live across it)
    const double2 ab = reinterpret_cast<const double2*>(p.par)[i];
    const double2 gl = p.glg[i];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        R[k] = p.R[k * m + i];
        rho[k] = p.q[k * m + i];
        tok[k] = p.tok[k * m + i];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = lds_price(a, L, tok[k]);
    if (!curve_solve<N>(rho, R, v, ab.x, ab.y, gl.x, lr)) {   // inside the fee band: no trade
        ncoin_no_trade<N, MAT>(p, m, i);
        return;
    }
    const double rg = 1.0 / gl.x;
    double sum_l = 0.0, sum_d = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const bool nan_k = lr[k] != lr[k];
        const double em = expm1(lr[k] - rho[k]);
        const double lam = nan_k ? lr[k] : (lr[k] < rho[k] ? -(R[k] * em) : 0.0);
        const double del = nan_k ? lr[k] : (lr[k] > rho[k] ? (R[k] * em) * rg : 0.0);
        ncoin_emit<MAT>(p, a, L, m, i, k, tok[k], lam, del, sum_l, sum_d);
    }
    acc += sum_l - sum_d;
}

// The two families: the per-pool solve and the per-coin constant q that update_ncoin refreshes (the upload's expression)
struct WeightedFamily {
    template <int N, bool MAT>
    static __device__ __forceinline__ void pool(const NCoinPools& p, const SweepArgs& a, const SweepLds& L, int64_t i, double& acc)
    {
        weighted_pool<N, MAT>(p, a, L, i, acc);
    }
    static __device__ __forceinline__ double q_of(double r, const double* par, long long j) { return log(r / par[j]); }
};
struct CurveFamily {
    template <int N, bool MAT>
    static __device__ __forceinline__ void pool(const NCoinPools& p, const SweepArgs& a, const SweepLds& L, int64_t i, double& acc)
    {
        curve_pool<N, MAT>(p, a, L, i, acc);
    }
    static __device__ __forceinline__ double q_of(double r, const double*, long long) { return log(r); }
};

template <class F, int N, bool MAT>
__device__ __forceinline__ void ncoin_tiles(const NCoinPools& p, const SweepArgs& a, const SweepLds& L, int64_t i, int64_t step,
                                            int64_t left, double& acc)
{
    for (; left > 0; --left, i += step) F::template pool<N, MAT>(p, a, L, i, acc);
}

// One launch per N-coin segment; prologue (carve_lds, stage_prices: arm word, cancel, give-up report) and epilogue
// (finish_row: the partial row reduce_partials / reduce_gather fold) are the other families' own.  Ψ and acc: LDS bins of
// the wavefront, per-lane dual.
template <class F, bool MAT>
__global__ __launch_bounds__(kMidBlock) void sweep_ncoin(NCoinPools p, SweepArgs a)
{
    constexpr int BLOCK = kMidBlock;
    const SweepLds L = carve_lds<BLOCK, false>(a);
    const int staged = stage_prices<BLOCK, false>(a, L);
    const bool poison = (staged & kStageLive) == 0;
    const bool live = !poison || (staged & kStageGaveUp) != 0;
    if (staged & kStageGaveUp) report(a, kFlagGaveUp);
    double acc = 0.0;
    if (!poison) {
        const int64_t stride = (int64_t)gridDim.x * BLOCK;
        const int64_t i0 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
        const int64_t left = i0 < a.m ? (a.m - i0 + stride - 1) / stride : 0;
        const int64_t step = a.reverse ? -stride : stride;
        const int64_t i = a.reverse ? i0 + (left - 1) * stride : i0;
        switch (p.n_coins) {
        case 2: ncoin_tiles<F, 2, MAT>(p, a, L, i, step, left, acc); break;
        case 3: ncoin_tiles<F, 3, MAT>(p, a, L, i, step, left, acc); break;
        case 4: ncoin_tiles<F, 4, MAT>(p, a, L, i, step, left, acc); break;
        case 5: ncoin_tiles<F, 5, MAT>(p, a, L, i, step, left, acc); break;
        case 6: ncoin_tiles<F, 6, MAT>(p, a, L, i, step, left, acc); break;
        case 7: ncoin_tiles<F, 7, MAT>(p, a, L, i, step, left, acc); break;
        case 8: ncoin_tiles<F, 8, MAT>(p, a, L, i, step, left, acc); break;
        default: break;
        }
    }
    finish_row<BLOCK, false>(a, L, acc, (int)blockIdx.x, poison, live);
}

} // namespace cfmm
