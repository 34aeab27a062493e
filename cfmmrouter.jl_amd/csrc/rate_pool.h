// rate_pool.h -- marginal rates of the exact-input quotes of quote_pool.h, one function per pool kind.  Host + device code:
// rate_kernel (rate_kernels.h) runs them one lane per query beside the quote itself; tests/native/rate_host.cpp builds them
// for the CPU.
//
// rate_X(state, in, out, a) is the RIGHT derivative of a -> quote_X(state, in, out, a) at a: with x = γa, x′ = R_i + x and
// y′ = R_o − out the state the trade leaves, γ·∂φ/∂R_in ÷ ∂φ/∂R_out there.  At a == 0 it is the pool's spot rate, fee included.
// A NaN in the state or the amount propagates.  Every function takes what its quote takes and forms the intermediates it
// shares with the quote by the quote's own expressions, so that a caller that evaluates both pays for them once.  No function
// iterates beyond what the quote does.
//
//   Product             γ·(R_i/x′)·(R_o/x′): two quotients below 1 and one product, no square that could overflow
//   weighted (N >= 2)   γ·(w_i/w_o)·(y′/x′) with y′ = R_o·exp(−(w_i/w_o)·log1p(x/R_i)) -- y′ from the invariant, never as
//                       R_o − out: a large trade leaves y′ far below the rounding of R_o
//   Solidly             γ·p(u), p(u) = u(3 + u²)/(1 + 3u²), u = y′/x′ the root quote_solidly solves for (solidly_cubic is
//                       that function's text); p is increasing with p′ <= 3, so the root's relative error passes through
//                       amplified by at most 3
//   Curve               φ = αΣR − β/ΠR: γ·(α + P′/x′)/(α + P′/y′), P′ = β/ΠR′ = P₀·(R_i/x′)·(R_o/y′), P₀ as quote_curve
//                       forms it.  y′ is the positive root of the quote's quadratic α·y² − C·y − B = 0 taken in the form
//                       without a difference: C < 0: 2B/(h − C), else (C + h)/(2α); at α = 0 (C = −P₀ < 0) this is
//                       B/P₀ = R_o·R_i/x′, the Product state
//   UniV3               the record quote_univ3's search lands on, with d = γa: inside a tick with (k, s_in) and d_local
//                       = d − Σδmax, γ·k/(s_in + d_local)²; the clamp of the tick's contribution does not change it; the
//                       list exhausted: +0.0.  a == 0 takes NO early return: with d = 0 the same search lands on the
//                       first record of the direction that has capacity (ties in Σδmax go forward), which is the right
//                       derivative also when the current tick is empty; at an exact tick boundary Σδmax_e <= d makes it
//                       the next tick's rate
#pragma once

#include "quote_pool.h"

namespace cfmm {

__host__ __device__ inline double rate_product(double Ri, double Ro, double g, double a)
{
    const double x = g * a;
    const double xp = Ri + x;
    return g * ((Ri / xp) * (Ro / xp));
}

__host__ __device__ inline double rate_weighted(double Ri, double Ro, double wi, double wo, double g, double a)
{
    const double x = g * a;
    const double wr = wi / wo;
    const double yp = Ro * exp(-(wr * log1p(x / Ri)));
    return g * (wr * (yp / (Ri + x)));
}

__host__ __device__ inline double rate_solidly(double Ri, double Ro, double g, double a)
{
    const double x = g * a;
    const double xp = Ri + x;
    const double t0 = Ro / Ri, r = Ri / xp, r2 = r * r;
    const double c = (t0 * (t0 * t0 + 1.0)) * (r2 * r2);
    const double u = solidly_cubic(c);
    const double uu = u * u;
    return g * ((u * (3.0 + uu)) / (1.0 + 3.0 * uu));
}

__host__ __device__ inline double rate_curve(double Ri, double Ro, double srho, double alpha, double lbeta, double g, double a)
{
    const double x = g * a;
    const double xp = Ri + x;
    const double P0 = exp(lbeta - srho);
    const double C = alpha * (Ro - x) - P0;
    const double B = (P0 * Ro) * (Ri / xp);
    const double h = hypot(C, 2.0 * (sqrt(alpha) * sqrt(B)));
    const double yp = C < 0.0 ? (2.0 * B) / (h - C) : (C + h) / (2.0 * alpha);
    const double Pp = (P0 * (Ri / xp)) * (Ro / yp);
    return g * ((alpha + Pp / xp) / (alpha + Pp / yp));
}

__host__ __device__ inline double rate_univ3_tick(double k, double s_in, double g, double d)
{
    const double s = s_in + d;
    return g * (k / (s * s));
}
__host__ __device__ inline double rate_univ3(double2 cur_a, double2 cur_b, double cur_c, double2 curR, int4 walk,
                                             const TickRec* ticks, double g, int in, double a)
{
    const double d = g * a;
    if (d != d) return d;
    const double k = cur_a.x;
    const double s_in = in == 0 ? cur_a.y : cur_b.x;
    const double dmax = in == 0 ? cur_b.y : cur_c;
    if (k != 0.0 && d < dmax) return rate_univ3_tick(k, s_in, g, d);
    const TickRec* list = ticks + (in == 0 ? walk.x : walk.z);
    const int cnt = in == 0 ? walk.y : walk.w;        // records 0 .. cnt-1 are ticks, record cnt closes the list
    // quote_univ3's search: the largest e in [0, cnt] with Σδmax_e <= δ′
    int lo = 0, hi = cnt + 1;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (list[mid].psum.x <= d) lo = mid;
        else hi = mid;
    }
    if (lo == cnt) return 0.0;
    const TickRec e = list[lo];
    return rate_univ3_tick(e.ks.x, e.ks.y, g, d - e.psum.x);
}

} // namespace cfmm
