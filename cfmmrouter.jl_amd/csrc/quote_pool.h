// quote_pool.h -- exact-input swap quotes and, below them, their inverses (exact-output), one function per pool kind.  Host + device code: quote_kernel (quote_kernels.h)
// runs them one lane per query; tests/native/quote_host.cpp builds them for the CPU.
//
// What is generalised: forward_trade(Δ, cfmm::UniV3), src/cfmms.jl:398-449, the reference's only quote.  For every kind:
// given the pool's state as the device holds it, the local coin positions in != out and the tendered amount a >= 0, the
// result is the largest out >= 0 with φ(R + γ·a·e_in − out·e_out) = φ(R) -- the constraint of src/cfmms.jl:26-31 (fee on the
// input) met with equality.  a == 0 gives exactly +0.0; a NaN in the state or the amount propagates.  No function iterates
// (UniV3 searches its walk list on the running sums the records carry: at most 7 probes for 64 ticks).
//
//   Product             out = R_o·(x/(R_i + x)),  x = γa
//   weighted (N >= 2)   out = −R_o·expm1(−(w_i/w_o)·log1p(x/R_i))               (Product N-coin: equal weights)
//   Solidly             frame of the tendered coin: x′ = R_i + x, u = y′/x′ solves u³ + u = c,
//                       c = t₀(1 + t₀²)·(R_i/x′)⁴, t₀ = R_o/R_i (k = φ(R) is never formed: DESIGN §3.0c); Cardano
//                       u = s − 1/(3s), s = cbrt(c/2 + hypot(c/2, 27^-½)), then TWO Newton steps on u³ + u − c: for small
//                       c (a large amount, or t₀ small) the two terms of Cardano's form cancel to rounding noise of the
//                       size of s, far above the root.  The cubic is linear to O(u³) there, so the first step lands on
//                       the root to the precision of the NOISE's last bit (the step subtracts two numbers of that size:
//                       measured 77 units of the bound at t₀ = 1e-18 with one step) and the second to the root's own;
//                       out = R_o − u·x′
//   Curve               D fixed, only r_i and r_o move: α·y² − C·y − B = 0 in y = r_o, C = α(R_o − x) − P₀,
//                       B = P₀·R_o·R_i/x′, P₀ = β/ΠR = exp(log β − Σ log R).  Solved for out = R_o − y itself -- the same
//                       quadratic shifted by R_o: α·o² − E·o + G = 0 with E = α(R_o + x) + P₀ > 0 and
//                       G = R_o·x·(α + P₀/x′) >= 0, both sums of non-negative terms, and the discriminant of both is
//                       C² + 4αB = h².  out = 2G/(E + h): no difference of nearly equal numbers for either sign of C,
//                       G = 0 at a = 0, and at α = 0 it is R_o·x/x′, the Product quote.
//   UniV3               below
#pragma once

#include "sweep.h"

#include <cmath>

namespace cfmm {

__host__ __device__ inline double quote_product(double Ri, double Ro, double g, double a)
{
    const double x = g * a;
    return Ro * (x / (Ri + x));
}

__host__ __device__ inline double quote_weighted(double Ri, double Ro, double wi, double wo, double g, double a)
{
    const double x = g * a;
    // 0 − expm1(·), not a negation: at a == 0 the result is +0.0 whichever zero the library's expm1 returns for −0.0
    return Ro * (0.0 - expm1(-((wi / wo) * log1p(x / Ri))));
}

__host__ __device__ inline double quote_solidly(double Ri, double Ro, double g, double a)
{
    const double x = g * a;
    const double xp = Ri + x;
    const double t0 = Ro / Ri, r = Ri / xp, r2 = r * r;
    const double c = (t0 * (t0 * t0 + 1.0)) * (r2 * r2);
    const double hc = 0.5 * c;
    const double s = cbrt(hc + hypot(hc, 0.19245008972987526));   // 27^-½
    double u = s - 1.0 / (3.0 * s);
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const double uu = u * u;
        u = u - (u * (uu + 1.0) - c) / (3.0 * uu + 1.0);
    }
    const double out = Ro - u * xp;
    // (a == 0: u = t₀ to rounding, so the difference is noise of either sign; the contract is +0.0)
    return a == 0.0 ? 0.0 : (out < 0.0 ? 0.0 : out);
}

// srho = Σ_k log R_k over ALL coins of the pool, lbeta = log β as the upload keeps it (NCoinPools::q, ::par)
__host__ __device__ inline double quote_curve(double Ri, double Ro, double srho, double alpha, double lbeta, double g, double a)
{
    const double x = g * a;
    const double xp = Ri + x;
    const double P0 = exp(lbeta - srho);
    const double C = alpha * (Ro - x) - P0;
    const double B = (P0 * Ro) * (Ri / xp);
    const double h = hypot(C, 2.0 * (sqrt(alpha) * sqrt(B)));
    const double E = alpha * (Ro + x) + P0;
    const double G = (Ro * x) * (alpha + P0 / xp);
    return (2.0 * G) / (E + h);
}

// UniV3.  The reference walks tick by tick, subtracting each tick's capacity from the amount and adding its reserve to the
// result (trade_through_pools, src/cfmms.jl:416-434).  The walk records (sweep.h TickRec) carry the running sums
// {Σδmax, ΣR_out} of everything before them, so the walk is a search plus one closed form: with δ′ = γa,
//   * the current tick holds liquidity and δ′ < its δmax: forward_amount of the current tick (:410-413);
//   * else the record e of the pool's list with Σδmax_e <= δ′ < Σδmax_e + δmax_e, found by bisection on Σδmax (nondecreasing
//     along a list), and out = ΣR_out_e + min(R_out_e, s_out_e − k_e/(s_in_e + (δ′ − Σδmax_e)));
//   * δ′ reaches the closing record: the list is exhausted, out = its ΣR_out ("We've exhausted all liquidity", :432); the
//     unused input is not reported, as in the reference.
// The last tick of a ladder has lower price 0, hence δmax = +inf: it absorbs any amount.  Each tick's contribution is
// clamped to [0, R_out].  Coin 0 in walks the price-falling list (walk.x, walk.y: get_upper_pools), coin 1 in the
// price-rising one (walk.z, walk.w: the flipped lower pools), :444-448.  `ticks` is the segment's record array.
__host__ __device__ inline double quote_univ3_tick(double k, double s_in, double s_out, double rout, double d)
{
    const double l = s_out - k / (s_in + d);   // forward_amount, :411
    // min(R_out, λ), floored at 0; written so that a NaN λ stays NaN
    return l < 0.0 ? 0.0 : (l > rout ? rout : l);
}
__host__ __device__ inline double quote_univ3(double2 cur_a, double2 cur_b, double cur_c, double2 curR, int4 walk,
                                              const TickRec* ticks, double g, int in, double a)
{
    const double d = g * a;
    if (a == 0.0) return 0.0;
    if (d != d) return d;
    const double k = cur_a.x;
    const double s_in = in == 0 ? cur_a.y : cur_b.x, s_out = in == 0 ? cur_b.x : cur_a.y;
    const double dmax = in == 0 ? cur_b.y : cur_c, rout = in == 0 ? curR.y : curR.x;
    if (k != 0.0 && d < dmax) return quote_univ3_tick(k, s_in, s_out, rout, d);
    const TickRec* list = ticks + (in == 0 ? walk.x : walk.z);
    const int cnt = in == 0 ? walk.y : walk.w;        // records 0 .. cnt-1 are ticks, record cnt closes the list
    // largest e in [0, cnt] with Σδmax_e <= δ′ (record 0 qualifies: its sum is the current tick's δmax, or 0)
    int lo = 0, hi = cnt + 1;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (list[mid].psum.x <= d) lo = mid;
        else hi = mid;
    }
    const TickRec e = list[lo];
    if (lo == cnt) return e.psum.y;
    return e.psum.y + quote_univ3_tick(e.ks.x, e.ks.y, e.dt.y, e.rout, d - e.psum.x);
}

// ---- exact-OUTPUT quotes (cfmm_quote_out): the inverse of the functions above -----------------------------------------------
// Given the wanted amount o >= 0 of the coin out, the result is the smallest a >= 0 with φ(R + γ·a·e_in − o·e_out) = φ(R).
// o == 0 gives exactly +0.0; the result is +inf where no finite input yields o (o >= R_o on the reserve kinds; on UniV3 an o
// beyond the direction's total, or equal to a total that is only approached because the last tick has δmax = +inf); a NaN in
// the state or in o propagates.  No function iterates (UniV3: the same search, on ΣR_out instead of Σδmax).
//
//   Product             a = R_i·o / ((R_o − o)·γ)
//   weighted (N >= 2)   x = R_i·expm1(−(w_o/w_i)·log1p(−o/R_o)), a = x/γ
//   Solidly             frame of the coin taken: y′ = R_o − o, u = x′/y′ solves the same cubic u³ + u = c with
//                       c = s₀(1 + s₀²)·(R_o/y′)⁴, s₀ = R_i/R_o (k = φ(R) is never formed); Cardano and two Newton steps as
//                       in quote_solidly (solidly_cubic below is that function's text, kept apart so that the forward
//                       kernel's code stays what it was).  x₀ = u·y′ − R_i subtracts two numbers of the size of R_i: its few
//                       u·R_i of noise depend on the library's cbrt and hypot (the host build measured 3.1 units where numpy's
//                       measured 0.79, on `balanced`).  So x₀, floored at 0, only STARTS two Newton steps on the cubic in x
//                       that φ(R_i + x, y′) − φ(R_i, y′) = φ(R_i, R_o) − φ(R_i, y′) is once both sides are expanded:
//                       x·(x² + 3R_i·x + 3R_i² + y′²) = Q, Q = R_i·o·(R_i² + R_o² + R_o·y′ + y′²)/y′ -- every coefficient a
//                       sum of positive terms, convex and increasing on x >= 0, so Newton from any start >= 0 stays above
//                       the root and the error of a step is that of its small correction; a = x/γ
//   Curve               D fixed: α·x² + E′·x − G′ = 0 in x = γa, E′ = α(R_i − o) + P₀, G′ = R_i·o·(α + P₀/y), y = R_o − o,
//                       P₀ = exp(log β − Σ log R).  h′ = hypot(E′, 2√α√G′); E′ >= 0: x = 2G′/(E′ + h′); E′ < 0 (o > R_i + P₀/α):
//                       x = (h′ − E′)/(2α), a sum of two positive numbers.  α = 0: E′ = P₀ > 0 and x = R_i·o/y, the Product answer
//   UniV3               below
__host__ __device__ inline double quote_out_product(double Ri, double Ro, double g, double o)
{
    if (o >= Ro) return __builtin_inf();
    return (Ri * o) / ((Ro - o) * g);
}

__host__ __device__ inline double quote_out_weighted(double Ri, double Ro, double wi, double wo, double g, double o)
{
    if (o == 0.0) return 0.0;   // (log1p(−0) = −0 and expm1 of either zero: the contract is +0.0 with any library)
    if (o >= Ro) return __builtin_inf();
    return (Ri * expm1(-((wo / wi) * log1p(-(o / Ro))))) / g;
}

// the real root of u³ + u = c, c >= 0: quote_solidly's Cardano + two Newton steps
__host__ __device__ inline double solidly_cubic(double c)
{
    const double hc = 0.5 * c;
    const double s = cbrt(hc + hypot(hc, 0.19245008972987526));   // 27^-½
    double u = s - 1.0 / (3.0 * s);
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const double uu = u * u;
        u = u - (u * (uu + 1.0) - c) / (3.0 * uu + 1.0);
    }
    return u;
}

__host__ __device__ inline double quote_out_solidly(double Ri, double Ro, double g, double o)
{
    if (o == 0.0) return 0.0;
    if (o >= Ro) return __builtin_inf();
    const double yp = Ro - o;
    const double s0 = Ri / Ro, r = Ro / yp, r2 = r * r;
    const double c = (s0 * (s0 * s0 + 1.0)) * (r2 * r2);
    const double u = solidly_cubic(c);
    double x = u * yp - Ri;   // off by a few u·R_i: two numbers of the size of R_i
    x = x < 0.0 ? 0.0 : x;
    // polished on the cubic in x itself, whose coefficients are sums of positive terms
    const double A = 3.0 * Ri, B = 3.0 * (Ri * Ri) + yp * yp;
    const double Q = ((Ri * o) * ((Ri * Ri + Ro * Ro) + (Ro * yp + yp * yp))) / yp;
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const double p = (x + A) * x + B;
        x = x - (x * p - Q) / (p + x * (2.0 * x + A));
    }
    return (x < 0.0 ? 0.0 : x) / g;
}

__host__ __device__ inline double quote_out_curve(double Ri, double Ro, double srho, double alpha, double lbeta, double g, double o)
{
    if (o == 0.0) return 0.0;
    if (o >= Ro) return __builtin_inf();
    const double y = Ro - o;
    const double P0 = exp(lbeta - srho);
    const double E = alpha * (Ri - o) + P0;
    const double G = (Ri * o) * (alpha + P0 / y);
    const double h = hypot(E, 2.0 * (sqrt(alpha) * sqrt(G)));
    const double x = E < 0.0 ? (h - E) / (2.0 * alpha) : (2.0 * G) / (E + h);
    return x / g;
}

// UniV3: the inverse walk.  The records carry ΣR_out of everything before them (psum.y), nondecreasing along a list, so
//   * the current tick holds liquidity and o < its R_out: forward_amount inverted in the current tick;
//   * else the largest e in [0, cnt] with ΣR_out_e <= o, by bisection; a non-closing e: a = (Σδmax_e + d)/γ with d the
//     inverse of s_out − k/(s_in + d) = o − ΣR_out_e in tick e, clamped to [0, δmax_e];
//   * e closes the list: o equal to its sum is reached with Σδmax/γ (+inf when the last tick's δmax is: the total is only
//     approached), a larger o by no input: +inf.
// The inverse in a tick is s_in·o_t/(s_out − o_t), not k/(s_out − o_t) − s_in: the latter subtracts two numbers of the size of
// s_in when o_t is small; the former relies on k = s_in·s_out, which the prepared constants meet to rounding (both are roots
// of k times or over the same price: univ3_pool.h) -- a relative perturbation of d of a few u.
__host__ __device__ inline double quote_out_univ3_tick(double s_in, double s_out, double dmax, double ot)
{
    const double d = (s_in * ot) / (s_out - ot);
    // clamped to [0, δmax]; written so that a NaN stays NaN
    return d < 0.0 ? 0.0 : (d > dmax ? dmax : d);
}
__host__ __device__ inline double quote_out_univ3(double2 cur_a, double2 cur_b, double cur_c, double2 curR, int4 walk,
                                                  const TickRec* ticks, double g, int in, double o)
{
    if (o == 0.0) return 0.0;
    if (o != o) return o;
    const double k = cur_a.x;
    const double s_in = in == 0 ? cur_a.y : cur_b.x, s_out = in == 0 ? cur_b.x : cur_a.y;
    const double dmax = in == 0 ? cur_b.y : cur_c, rout = in == 0 ? curR.y : curR.x;
    if (k != 0.0 && o < rout) return quote_out_univ3_tick(s_in, s_out, dmax, o) / g;
    const TickRec* list = ticks + (in == 0 ? walk.x : walk.z);
    const int cnt = in == 0 ? walk.y : walk.w;        // records 0 .. cnt-1 are ticks, record cnt closes the list
    // largest e in [0, cnt] with ΣR_out_e <= o (record 0 qualifies: its sum is the current tick's R_out, or 0)
    int lo = 0, hi = cnt + 1;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (list[mid].psum.y <= o) lo = mid;
        else hi = mid;
    }
    const TickRec e = list[lo];
    if (lo == cnt) return o == e.psum.y ? e.psum.x / g : (o > e.psum.y ? __builtin_inf() : __builtin_nan(""));
    return (e.psum.x + quote_out_univ3_tick(e.ks.y, e.dt.y, e.dt.x, o - e.psum.y)) / g;
}

} // namespace cfmm
