// quote_pool.h -- exact-input swap quotes, one function per pool kind.  Host + device code: quote_kernel (quote_kernels.h)
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

} // namespace cfmm
