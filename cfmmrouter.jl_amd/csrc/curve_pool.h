// curve_pool.h -- the per-pool solve of Curve (StableSwap) pools, src/cfmms.jl:66-70 (Curve{T}: R, γ, Ai, α, β; no
// find_arb! there).  Host + device code: sweep_ncoin<CurveFamily> (sweep_ncoin.h) runs it one lane per pool.
//
// Trading function φ(R) = α·Σ R_k − β·Π R_k⁻¹ (α >= 0, β > 0): StableSwap's invariant with D held fixed, α = A·nⁿ,
// β = D^{n+1}/nⁿ.  The problem of the find_arb! docstring (src/cfmms.jl:21-33): maximise Σ v_k(λ_k − δ_k) s.t.
// φ(R + γδ − λ) >= φ(R), δ, λ >= 0.  With r = R + γδ − λ, P = β/Π r (∂φ_k = α + P/r_k) and the multiplier ν = 1/x the
// KKT conditions decouple coin by coin once (x, P) are fixed:
//     log r_k = max(min(L − a_k^λ, ρ_k), L − a_k^δ),   L = log P, ρ_k = log R_k,
//     a_k^λ = log(v_k·x − α) (−inf where v_k·x <= α: the coin cannot leave),  a_k^δ = log(v_k·x/γ − α),
// leaving (E1) L + Σ log r_k = log β and (E2) α·Σ(r_k − R_k) − (P − P₀) = 0, P₀ = β/Π R_k (φ(r) = φ(R), never evaluated
// as φ itself: it cancels).
//
// Outer unknown s = log(v_min·x/γ − α), the δ-term of the cheapest coin: with c_k = v_k/v_min >= 1 every term is
//     v_k·x/γ − α = c_k·eˢ + α·(c_k − 1),        v_k·x − α = γ·c_k·eˢ + α·(γ·c_k − 1),
// sums of non-negative parts and one difference formed from (v_k − v_min) and the exact 1 − γ: no cancellation against α
// in stiff pools (large α, prices near each other), where the terms are tiny next to α.  s ranges over all of R.
// Inner (E1 for a given s): the left side is nondecreasing and piecewise linear in L with 2N breakpoints ρ_k + a_k; it is
// evaluated at each (N² clamp terms, no sort), the root is bracketed and interpolated exactly (weighted_pool's method).
// Outer (E2, decreasing in s): Newton on s with the analytic derivative (the active set is fixed between breakpoints),
// safeguarded by the bracket the iterates build, bisection when a step leaves it or does not halve the last one, bracket
// expansion by doubling steps until E2 changes sign.  A lane stops once E2 holds to its own rounding (4·(N + 2)·eps of the
// size of its terms) or the step / bracket is down to the last bits of s; kCurveMaxIter caps it.  (Stopping on the
// residual matters for speed, not accuracy: a lane that bisects its bracket down to the last bit runs ~60 steps, and a
// wavefront runs at the pace of its slowest lane.)
// No trade iff max_k γ·∇φ_k(R)/v_k <= min_k ∇φ_k(R)/v_k (the fee band): every trade is exactly +0.0.
// Range: the band check and the start form P₀/R_k = exp(log β − Σρ − ρ_k) in linear space.  The upload refuses a pool with
// α > 0 where one of them lies outside e^±kCurveLogRange (curve_in_range), and gives a pool with α = 0 -- Product, whose
// trades do not depend on β -- a log β that centres them instead (curve_solve_lbeta).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace cfmm {

constexpr int kCurveMaxIter = 64;
constexpr double kCurveLogRange = 600.0;
constexpr double kCurveFarStart = 64.0;   // log α − log(P₀/R_ref) beyond which the solve starts midway between them
constexpr double kCurveReach = 16.0;      // longest Newton step before the bracket closes, in units of the doubling step
constexpr double kCurveSMax = 680.0;      // |s| the iterates keep to: eˢ·c_k stays finite for price ratios up to e^29

// Host: false iff some |log(P₀/R_k)| = |lbeta − Σρ − ρ_k| exceeds kCurveLogRange (or is NaN).
inline bool curve_in_range(double lbeta, const double* rho, int n)
{
    double sr = 0.0;
    for (int k = 0; k < n; ++k) sr += rho[k];
    for (int k = 0; k < n; ++k)
        if (!(std::fabs(lbeta - sr - rho[k]) <= kCurveLogRange)) return false;
    return true;
}

// Host: log β as curve_solve takes it.  Unchanged, except at α = 0 outside the range: Σρ + mean ρ, which puts every
// log(P₀/R_k) at mean ρ − ρ_k (the same level sets ΠR = const, hence the same trades).
inline double curve_solve_lbeta(double alpha, double lbeta, const double* rho, int n)
{
    if (alpha != 0.0 || curve_in_range(lbeta, rho, n)) return lbeta;
    double sr = 0.0;
    for (int k = 0; k < n; ++k) sr += rho[k];
    return sr + sr / n;
}

// Returns false inside the fee band (no trade).  Otherwise lr[k] = log r_k at the optimum (exactly ρ_k for a coin that
// does not trade).  A NaN price gives NaN everywhere (as the other families propagate it).
template <int N>
__host__ __device__ inline bool curve_solve(const double (&rho)[N], const double (&R)[N], const double (&v)[N], double alpha,
                                            double lbeta, double gamma, double (&lr)[N])
{
    double sr = 0.0, vmin = __builtin_inf();
    int ref = 0;
    bool nan_in = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sr += rho[k];
        nan_in = nan_in || v[k] != v[k];
        if (v[k] < vmin) { vmin = v[k]; ref = k; }
    }
    const double L0 = lbeta - sr;
    if (nan_in) {
#pragma unroll
        for (int k = 0; k < N; ++k) lr[k] = __builtin_nan("");
        return true;
    }
    // fee band at R: ∇φ_k = α + P₀/R_k
    double bhi = -__builtin_inf(), blo = __builtin_inf();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double q = (alpha + exp(L0 - rho[k])) / v[k];
        bhi = __builtin_fmax(bhi, gamma * q);
        blo = __builtin_fmin(blo, q);
    }
    if (bhi <= blo) return false;
    const double omg = 1.0 - gamma;   // exact for γ in [1/2, 1]
    double c[N], e[N];                // c_k = v_k / v_min, e_k = (v_k − v_min) / v_min
#pragma unroll
    for (int k = 0; k < N; ++k) {
        c[k] = v[k] / vmin;
        e[k] = (v[k] - vmin) / vmin;
    }
    double s = L0 - rho[ref];   // eˢ = P₀/R_ref: the cheapest coin at the edge of entering
    // A pool far from the product regime (α ≫ P₀/R_ref: near constant sum) drains one coin, to r ≈ P/(α·δ) for its price
    // offset δ; E1 then puts s* a fraction (N − 1)/N of the way from log(P₀/R_ref) to log α (up to log δ / N): start there,
    // not hundreds of units off
    if (alpha > 0.0) {
        const double la = log(alpha);
        if (la - s > kCurveFarStart) s += (la - s) * ((N - 1.0) / N);
    }
    double lo = -__builtin_inf(), hi = __builtin_inf(), step = 1.0, dx_old = __builtin_inf();
    for (int it = 0; it < kCurveMaxIter; ++it) {
        // ---- state at s: the terms, E1's root L, log r, E2 and its derivative
        const double es = exp(s);
        double ad[N], al[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double td = c[k] * es + alpha * e[k];
            const double tl = gamma * c[k] * es + alpha * (e[k] - omg * c[k]);
            ad[k] = log(td);
            al[k] = tl > 0.0 ? log(tl) : -__builtin_inf();
        }
        double flo = -__builtin_inf(), gflo = 0.0, fhi = __builtin_inf(), gfhi = 0.0;
        // (a rolled loop over the breakpoints, each picked from the register arrays by selects: unrolled, the 2N
        //  independent sums are all scheduled at once and spill at N = 8)
#pragma unroll 1
        for (int j = 0; j < 2 * N; ++j) {
            double b = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                b = j == k ? rho[k] + al[k] : b;
                b = j == k + N ? rho[k] + ad[k] : b;
            }
            if (b == -__builtin_inf()) continue;
            double G = b - lbeta;
#pragma unroll
            for (int k = 0; k < N; ++k) G += __builtin_fmax(__builtin_fmin(b - al[k], rho[k]), b - ad[k]);
            if (G <= 0.0 && b > flo) { flo = b; gflo = G; }
            if (G >= 0.0 && b < fhi) { fhi = b; gfhi = G; }
        }
        double L;
        if (flo != -__builtin_inf() && (gflo == 0.0 || !(flo < fhi))) {
            L = gflo == 0.0 ? flo : fhi;   // a breakpoint is the root (or rounding crossed the bracket over)
        } else {
            const bool below = flo == -__builtin_inf();
            const double probe = below ? fhi - 1.0 : fhi == __builtin_inf() ? flo + 1.0 : flo + 0.5 * (fhi - flo);
            double slope = 1.0;
#pragma unroll
            for (int k = 0; k < N; ++k) slope += (probe < rho[k] + al[k] ? 1.0 : 0.0) + (probe > rho[k] + ad[k] ? 1.0 : 0.0);
            L = below ? fhi - gfhi / slope : flo - gflo / slope;
            if (!below && fhi != __builtin_inf()) L = __builtin_fmin(__builtin_fmax(L, flo), fhi);
        }
        // E2 and dE2/ds = −P·L' + α·Σ_live r_k·(L' − a_k'), L' = Σ_live a_k' / (1 + #live) (E1 differentiated)
        double h = 0.0, habs = 0.0, sda = 0.0, nact = 0.0, sr_live = 0.0, srda = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            lr[k] = __builtin_fmax(__builtin_fmin(L - al[k], rho[k]), L - ad[k]);
            const double dr = R[k] * expm1(lr[k] - rho[k]);   // r_k − R_k
            h += dr;
            habs += R[k] + __builtin_fabs(dr);
            const bool in = lr[k] > rho[k], out = lr[k] < rho[k];
            // a_k' of the live branch (a_k^δ: c·eˢ / t^δ, a_k^λ: γ·c·eˢ / t^λ)
            const double da = in ? c[k] * es * exp(-ad[k]) : out ? gamma * c[k] * es * exp(-al[k]) : 0.0;
            sda += da;
            nact += (in || out) ? 1.0 : 0.0;
            sr_live += (in || out) ? R[k] + dr : 0.0;
            srda += (R[k] + dr) * da;
        }
        const double dP = exp(L0) * expm1(L - L0);
        h = alpha * h - dP;
        habs = alpha * habs + exp(L0) + __builtin_fabs(dP);   // the size of E2's terms: its rounding noise is ~N·eps of it
        const double dL = sda / (1.0 + nact);
        const double dh = alpha * (dL * sr_live - srda) - exp(L) * dL;
        // ---- safeguarded Newton step on E2 (decreasing in s)
        if (__builtin_fabs(h) <= 4.0 * (N + 2) * __DBL_EPSILON__ * habs) break;   // E2 holds to its own rounding
        if (h > 0.0) lo = s; else hi = s;
        double sn = s - h / dh;
        const bool bracketed = lo != -__builtin_inf() && hi != __builtin_inf();
        // (before the bracket closes, a Newton step longer than kCurveReach·step -- E2 is flat where few coins are live --
        //  or one that leaves |s| <= kCurveSMax is a doubling step instead: beyond it eˢ overflows, and a state built from
        //  infinite terms reads as converged with no trade)
        if (!(sn > lo && sn < hi) || (bracketed && !(2.0 * __builtin_fabs(sn - s) <= dx_old)) ||
            (!bracketed && !(__builtin_fabs(sn - s) <= kCurveReach * step && __builtin_fabs(sn) <= kCurveSMax))) {
            if (bracketed) {
                sn = lo + 0.5 * (hi - lo);
            } else {
                sn = h > 0.0 ? s + step : s - step;   // expand towards the sign change
                sn = __builtin_fmin(__builtin_fmax(sn, -kCurveSMax), kCurveSMax);
                step *= 2.0;
            }
        }
        dx_old = __builtin_fabs(sn - s);
        if (dx_old <= 4.0 * __DBL_EPSILON__ * __builtin_fmax(1.0, __builtin_fabs(s)) ||
            (bracketed && hi - lo <= 4.0 * __DBL_EPSILON__ * __builtin_fmax(1.0, __builtin_fabs(lo))))
            break;
        s = sn;
    }
    return true;
}

} // namespace cfmm
