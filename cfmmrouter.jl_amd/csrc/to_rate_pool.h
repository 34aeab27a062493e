// to_rate_pool.h -- the inverse of rate_pool.h: the amount at which a pool's marginal rate has fallen to a limit, one function
// per pool kind.  Host + device code: to_rate_kernel (to_rate_kernels.h) and swap_limit_kernel (swap_limit_kernels.h) run them
// one lane per query; tests/native/to_rate_host.cpp builds them for the CPU.
//
// For a pool as it stands, local coin positions in != out and a limit r (finite, > 0):
//     to_rate_X(state, in, out, r) = sup { a >= 0 : rate_X(state, in, out, a) >= r },     {0} where the set is empty,
// rate_X the right derivative of the exact-input quote (rate_pool.h), non-increasing in a on every family.  Consequences:
//   * the answer is exactly +0.0 where the spot rate is already <= r; that is decided by comparing r with the family's own
//     rate_X(state, .., 0.0), so cfmm_quote_rate at amount 0 and this function agree on which side of the limit a pool is;
//   * UniV3: a limit that falls inside an empty tick's price range (between the end of one record and the start of the next)
//     answers the boundary in front of it, Σδmax of the next record over γ;
//   * UniV3: a limit below the rate at the end of the direction's last tick answers the direction's whole capacity, the
//     closing record's Σδmax/γ -- the value cfmm_quote_out(cfmm_quote(.)) reports (the same additions: Σδmax_e + δmax_e IS
//     Σδmax_{e+1});
//   * an answer that overflows a double is +inf;
//   * a NaN in the state or the limit propagates (every early return is taken on a comparison that a NaN fails).
// The pool rests at r only to rounding: rate_X(to_rate_X(r)) may lie an ulp-scale amount on either side of r.
//
// Forms, s = the spot rate, x′ = R_in + γa, d = (s − r)/r > 0 (the difference of two nearby doubles is exact):
//   Product             x′/R_in = √(s/r):               a = R_in·(d/(√(1 + d) + 1))/γ
//   weighted (N >= 2)   x′/R_in = (s/r)^{1/(1 + w)}:    a = R_in·expm1(log1p(d)/(1 + w))/γ, w = w_in/w_out
//   Solidly             u = y′/x′ with p(u) = r/γ, p(u) = u(3 + u²)/(1 + 3u²) -- tanh's triple-angle formula: with ρ = r/γ,
//                       u = tanh(atanh(ρ)/3) for ρ < 1, 1/tanh(atanh(1/ρ)/3) for ρ > 1 (p(1/u) = 1/p(u)), 1 at ρ = 1.  x³y + xy³
//                       = x⁴(u + u³) is kept, so (x′/R_in)⁴ = (t₀ + t₀³)/(u + u³), t₀ = R_out/R_in, and the ratio minus one is
//                       expm1(log1p((t₀ − u)(1 + t₀² + t₀u + u²)/(u + u³))/4): t₀ − u, not a difference of cubes
//   Curve               no closed form.  a -> rate_curve is monotone; the root of rate_curve(a) = r is bracketed in a itself:
//                       from the Product answer a₀ the bracket grows (or shrinks) by factors of 4, 16, 256, ... until the rate
//                       straddles r, a wide bracket is halved on the logarithmic scale until its ends are within a factor
//                       of 4, then the Illinois variant of regula falsi with a bisection step whenever the secant point
//                       leaves the bracket.  Every evaluation is rate_curve ITSELF, so the answer is an a the search visited
//                       with cfmm_quote_rate's rate >= r − ulp(r).  The search is a pure function of the inputs (no lane, launch
//                       geometry or batching enters) and ends at a point whose rate is within 2^-52·r of r (beyond it the
//                       differences are rounding noise of rate_curve) or when the bracket's ends are neighbours;
//                       kToRateCurveIters caps the evaluations of rate_curve.  If the cap is hit the answer is the bracket's
//                       LOWER end: an amount whose rate is still >= r, at most the bracket's width below the supremum
//                       (+0.0 if the bracket was never closed from below).  The same holds where an evaluation INSIDE the search
//                       is no number (far out R_in/x′ underflows and rate_curve forms 0·inf): the search ends there with its
//                       lower end; only a NaN in the state or the limit, seen at the spot rate or the first point, propagates
//   UniV3               rate = γ·k/(s_in + d)² inside a record, continuous across adjacent live ticks.  The current tick as
//                       rate_univ3 handles it (it holds liquidity and the limit is reached inside it: its own (k, s_in));
//                       else the largest record e of the direction's list whose START rate γk_e/s_in,e² is above r, by
//                       bisection on the record fields alone (quote_univ3's search shape); inside it d_local =
//                       s_in·(d/(√(1 + d) + 1)) with d = (start − r)/r, clamped to [0, δmax_e]; a = (Σδmax_e + d_local)/γ
#pragma once

#include "rate_pool.h"

namespace cfmm {

// √(1 + d) − 1 for d >= 0 without the difference
__host__ __device__ inline double to_rate_sqrt1pm1(double d) { return d / (sqrt(1.0 + d) + 1.0); }

__host__ __device__ inline double to_rate_product(double Ri, double Ro, double g, double r)
{
    const double s = rate_product(Ri, Ro, g, 0.0);
    if (s <= r) return 0.0;
    const double d = (s - r) / r;
    return (Ri * to_rate_sqrt1pm1(d)) / g;
}

__host__ __device__ inline double to_rate_weighted(double Ri, double Ro, double wi, double wo, double g, double r)
{
    const double s = rate_weighted(Ri, Ro, wi, wo, g, 0.0);
    if (s <= r) return 0.0;
    const double d = (s - r) / r;
    const double wr = wi / wo;
    return (Ri * expm1(log1p(d) / (1.0 + wr))) / g;
}

// u > 0 with u(3 + u²)/(1 + 3u²) = rho
__host__ __device__ inline double to_rate_solidly_u(double rho)
{
    if (rho < 1.0) return tanh(atanh(rho) / 3.0);
    if (rho > 1.0) return 1.0 / tanh(atanh(1.0 / rho) / 3.0);
    return rho;   // 1, or a NaN
}

__host__ __device__ inline double to_rate_solidly(double Ri, double Ro, double g, double r)
{
    const double s = rate_solidly(Ri, Ro, g, 0.0);
    if (s <= r) return 0.0;
    const double u = to_rate_solidly_u(r / g);
    const double t0 = Ro / Ri;
    const double q = ((t0 - u) * ((1.0 + t0 * t0) + (t0 * u + u * u))) / (u * (1.0 + u * u));
    const double a = (Ri * expm1(0.25 * log1p(q))) / g;
    // (r within rounding of s: u may land above t₀; the contract there is +0.0)
    return a < 0.0 ? 0.0 : a;
}

constexpr int kToRateCurveIters = 128;   // evaluations of rate_curve per query, at most

// iters (may be null): the evaluations of rate_curve the search made
__host__ __device__ inline double to_rate_curve(double Ri, double Ro, double srho, double alpha, double lbeta, double g, double r,
                                                int* iters = nullptr)
{
    if (iters) *iters = 1;
    const double s = rate_curve(Ri, Ro, srho, alpha, lbeta, g, 0.0);
    if (s <= r) return 0.0;
    if (!(s > r)) return s + r;   // a NaN in the state or the limit
    // the Product answer: exact at α = 0, the start of the bracket otherwise
    double hi = (Ri * to_rate_sqrt1pm1((s - r) / r)) / g;
    double lo = 0.0, flo = s - r;
    int n = 1;
    double fhi = rate_curve(Ri, Ro, srho, alpha, lbeta, g, hi) - r;
    ++n;
    if (!(fhi == fhi)) return fhi;
    const double noise = 0x1p-52 * r;
    if (fhi >= -noise && fhi <= noise) {   // (α = 0: the Product answer is the answer)
        if (iters) *iters = n;
        return hi;
    }
    if (fhi > 0.0) {
        // grow until the rate is at or below the limit: by 4, 16, 256, ... (the factor squares, up to 2^64)
        double f = 4.0;
        while (fhi > 0.0 && n < kToRateCurveIters) {
            lo = hi;
            flo = fhi;
            hi = f * hi;
            f = f < 0x1p32 ? f * f : 0x1p64;
            if (!(hi < __builtin_inf())) {
                if (iters) *iters = n;
                return __builtin_inf();
            }
            fhi = rate_curve(Ri, Ro, srho, alpha, lbeta, g, hi) - r;
            ++n;
        }
        if (!(fhi <= 0.0)) {   // the cap was hit, or the rate is no number out there (R_in/x′ underflows against P₀·R_out/y′): the lower end
            if (iters) *iters = n;
            return lo;
        }
    } else {
        // shrink, by the same factors, until the rate is above the limit again (or the amount underflows: lo stays 0)
        double f = 0.25;
        while (n < kToRateCurveIters) {
            const double c = f * hi;
            f = f > 0x1p-32 ? f * f : 0x1p-64;
            if (!(c > 0.0)) break;
            const double fc = rate_curve(Ri, Ro, srho, alpha, lbeta, g, c) - r;
            ++n;
            if (!(fc == fc)) break;   // (no number: the bracket stays what it is)
            if (fc > 0.0) {
                lo = c;
                flo = fc;
                break;
            }
            hi = c;
            fhi = fc;
        }
    }
    // flo > 0 >= fhi on lo < hi.  A wide bracket is first halved on the logarithmic scale (the rate falls like a power of a)
    while (lo > 0.0 && hi > 4.0 * lo && n < kToRateCurveIters) {
        const double c = sqrt(lo) * sqrt(hi);
        const double fc = rate_curve(Ri, Ro, srho, alpha, lbeta, g, c) - r;
        ++n;
        if (!(fc == fc)) break;   // (no number: the search ends with the bracket it has)
        if (fc > 0.0) {
            lo = c;
            flo = fc;
        } else {
            hi = c;
            fhi = fc;
        }
    }
    // Illinois: the secant point; the end that stays twice in a row has its value halved.  A point whose rate is within an
    // ulp of the limit ends the search: beyond it the differences are rounding noise of rate_curve
    int side = 0;
    double flo_w = flo, fhi_w = fhi;
    while (n < kToRateCurveIters) {
        double c = hi - (fhi_w * (hi - lo)) / (fhi_w - flo_w);
        if (!(c > lo && c < hi)) c = lo + 0.5 * (hi - lo);
        if (!(c > lo && c < hi)) break;   // the ends are neighbours
        const double fc = rate_curve(Ri, Ro, srho, alpha, lbeta, g, c) - r;
        ++n;
        if (!(fc == fc)) break;   // (no number: the search ends with the bracket it has)
        if (fc >= -noise && fc <= noise) {
            lo = c;
            break;
        }
        if (fc > 0.0) {
            lo = c;
            flo_w = fc;
            if (side == -1) fhi_w = 0.5 * fhi_w;
            side = -1;
        } else {
            hi = c;
            fhi_w = fc;
            if (side == 1) flo_w = 0.5 * flo_w;
            side = 1;
        }
    }
    if (iters) *iters = n;
    return lo;
}

// inside a record that starts at rate `start` > r: the part of δ′ that brings it to r
__host__ __device__ inline double to_rate_univ3_tick(double k, double s_in, double dmax, double g, double r)
{
    const double start = rate_univ3_tick(k, s_in, g, 0.0);
    const double d = s_in * to_rate_sqrt1pm1((start - r) / r);
    // clamped to [0, δmax]; written so that a NaN stays NaN
    return d < 0.0 ? 0.0 : (d > dmax ? dmax : d);
}
__host__ __device__ inline double to_rate_univ3(double2 cur_a, double2 cur_b, double cur_c, double2 curR, int4 walk,
                                                const TickRec* ticks, double g, int in, double r)
{
    const double s = rate_univ3(cur_a, cur_b, cur_c, curR, walk, ticks, g, in, 0.0);
    if (s <= r) return 0.0;
    if (!(s > r)) return s + r;   // a NaN in the state or the limit
    const double k = cur_a.x;
    const double s_in = in == 0 ? cur_a.y : cur_b.x;
    const double dmax = in == 0 ? cur_b.y : cur_c;
    if (k != 0.0 && 0.0 < dmax) {
        // the current tick, where rate_univ3 reads the spot rate: the limit is reached inside it, or it drains
        const double start = rate_univ3_tick(k, s_in, g, 0.0);
        const double d = s_in * to_rate_sqrt1pm1((start - r) / r);
        if (d < dmax) return (d < 0.0 ? 0.0 : d) / g;
    }
    const TickRec* list = ticks + (in == 0 ? walk.x : walk.z);
    const int cnt = in == 0 ? walk.y : walk.w;        // records 0 .. cnt-1 are ticks, record cnt closes the list
    // the largest e in [0, cnt) whose start rate is above r; none: the boundary in front of record 0 (the current tick's
    // δmax, or 0), which with cnt == 0 is the closing record's sum -- the whole capacity
    int lo = -1, hi = cnt;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        const TickRec m = list[mid];
        if (rate_univ3_tick(m.ks.x, m.ks.y, g, 0.0) > r) lo = mid;
        else hi = mid;
    }
    if (lo < 0) return list[0].psum.x / g;
    const TickRec e = list[lo];
    return (e.psum.x + to_rate_univ3_tick(e.ks.x, e.ks.y, e.dt.x, g, r)) / g;
}

} // namespace cfmm
