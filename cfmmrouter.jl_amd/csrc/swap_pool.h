// swap_pool.h -- the state a swap leaves behind: one function per piece and pool kind, and at the end swap_move / swap_store,
// which put the pieces together for every moving kernel (swap_kernel, swap_out_kernel, both swap-path kernels).  Host + device
// code: the kernels run them one lane per swap; tests/native/swap_host.cpp builds the pieces for the CPU.
//
// The amount that comes out is quote_pool.h's, unchanged: cfmm_swap's answer IS cfmm_quote's answer on the pool as it stands,
// by construction.  What is added here is the move R <- R + γΔ − Λ with Δ = a·e_in, Λ = out·e_out (src/cfmms.jl:26-31, the
// update cfmm_update_reserves applies), the refreshed prepared constants with the expressions of update_two_coin /
// update_ncoin (update_kernels.h), the validity test of the new state (pool_checks.h: what cfmm_pools_set_* refuses), and for
// UniV3 -- whose state is its price -- the price at which the swap comes to rest.
//
//   reserve kinds   R_in' = R_in + γ·a,  R_out' = R_out − out; each operation rounded on its own (-ffp-contract=off).
//                   Valid: both finite and > 0; Solidly: both inside [2^-kFastExp, 2^kFastExp]; Curve with α > 0: every
//                   |log β − Σ log R' − log R'_k| <= kCurveLogRange (swap_curve_in_range below).
//                   a == 0 moves nothing: the callers leave every bit of the pool, prepared constants included.
//   GeometricMean   {Q1, Q2} = {log γ + log η + log R2 + η·log R1, η·(log γ + log R1 − log η) + log R2}
//   weighted        q = log(R'/w) for the two coins that moved      Curve   q = log R' for the two coins that moved
//   UniV3           below
#pragma once

#include "../../include/cfmm_amd.h"
#include "quote_pool.h"

namespace cfmm {

// |x| in [2^-kFastExp, 2^kFastExp] (false for NaN, infinities, zero, denormals): fast_arith.h / univ3_pool.h's test on the
// exponent field, written on the value so that one text serves host and device
__host__ __device__ inline bool swap_in_window(double x)
{
    const double ax = x < 0.0 ? -x : x;
    return ax >= 0x1p-150 && ax < 0x1p151;
}
static_assert(kFastExp == 150, "swap_in_window spells the window's bounds out");

__host__ __device__ inline bool swap_finite_pos(double x) { return x > 0.0 && x < __builtin_inf(); }

// the reserves a swap of `a` for `out` leaves: {R_in', R_out'}
__host__ __device__ inline double2 swap_reserves(double Ri, double Ro, double g, double a, double out)
{
    return make_double2(Ri + g * a, Ro - out);
}

// what check_reserves (and, for Solidly, check_solidly_range) accepts
__host__ __device__ inline bool swap_reserves_valid(double2 rn, bool solidly)
{
    if (!(swap_finite_pos(rn.x) && swap_finite_pos(rn.y))) return false;
    return !solidly || (swap_in_window(rn.x) && swap_in_window(rn.y));
}

// GeometricMeanTwoCoin {Q1, Q2} of the reserves {r1, r2} in the POOL's coin order: update_two_coin's expressions
__host__ __device__ inline double2 swap_geomean_q(double g, double e, double r1, double r2)
{
    const double lg = log(g), le = log(e), l1 = log(r1), l2 = log(r2);
    return make_double2(((lg + le) + l2) + e * l1, e * ((lg + l1) - le) + l2);
}

__host__ __device__ inline double swap_weighted_q(double r, double w) { return log(r / w); }
__host__ __device__ inline double swap_curve_q(double r) { return log(r); }

// Curve, α > 0: curve_in_range (curve_pool.h) on the new logs.  q: the pool's log R column, coin k at q[k·stride]; the two
// coins that moved take their new logs qi, qo.  Two passes over the column and no array: the coin count is a run-time value.
__host__ __device__ inline bool swap_curve_in_range(double lbeta, const double* q, long long stride, int n, int ci, double qi,
                                                    int co, double qo)
{
    double sr = 0.0;
    for (int k = 0; k < n; ++k) sr += k == ci ? qi : (k == co ? qo : q[k * stride]);
    for (int k = 0; k < n; ++k) {
        const double t = lbeta - sr - (k == ci ? qi : (k == co ? qo : q[k * stride]));
        if (!((t < 0.0 ? -t : t) <= 600.0)) return false;   // kCurveLogRange
    }
    return true;
}

// UniV3: the price at which a swap of `a` of coin `in` comes to rest.  quote_univ3's own search finds where the swap lands:
//   * inside the current tick when it holds liquidity and δ′ = γa < its δmax: {k, s_in} of the current tick, d_t = δ′;
//   * else record e of the direction's walk list with Σδmax_e <= δ′, d_t = δ′ − Σδmax_e clamped to [0, δmax_e];
//   * δ′ reaches the closing record: the direction is exhausted and the pool rests at the far edge of its last non-empty
//     tick -- the list's last record, or the current tick when the list is empty -- i.e. that tick at d_t = δmax.
// There the tick holds s′ = s_in + d_t of the coin in (virtual reserves included), and since the prepared constants are
// sA = R1 + α = sqrt(k/p), sB = R2 + β = sqrt(k·p) (univ3_prepare_pool), the price is their inverse:
//   coin 0 in (price falling)  P = k/(s′·s′)          coin 1 in (price rising)  P = (s′·s′)/k
// a == 0, or a direction without any liquidity, leaves the price where it is (cp).  The host clamps P to the first tick's
// upper price and re-prepares the pool (abi_swap.cpp).
__host__ __device__ inline double swap_univ3_price(double cp, double2 cur_a, double2 cur_b, double cur_c, int4 walk,
                                                   const TickRec* ticks, double g, int in, double a)
{
    const double d = g * a;
    if (a == 0.0) return cp;
    if (d != d) return d;
    const double k = cur_a.x;
    const double s_in = in == 0 ? cur_a.y : cur_b.x;
    const double dmax = in == 0 ? cur_b.y : cur_c;
    double kk, ss, dt;
    if (k != 0.0 && d < dmax) {
        kk = k;
        ss = s_in;
        dt = d;
    } else {
        const TickRec* list = ticks + (in == 0 ? walk.x : walk.z);
        const int cnt = in == 0 ? walk.y : walk.w;
        int lo = 0, hi = cnt + 1;   // quote_univ3's bisection
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (list[mid].psum.x <= d) lo = mid;
            else hi = mid;
        }
        if (lo == cnt) {
            if (cnt > 0) {
                const TickRec e = list[cnt - 1];
                kk = e.ks.x;
                ss = e.ks.y;
                dt = e.dt.x;
            } else if (k != 0.0) {
                kk = k;
                ss = s_in;
                dt = dmax;
            } else {
                return cp;
            }
        } else {
            const TickRec e = list[lo];
            kk = e.ks.x;
            ss = e.ks.y;
            dt = d - e.psum.x;
            dt = dt < 0.0 ? 0.0 : (dt > e.dt.x ? e.dt.x : dt);
        }
    }
    const double sp = ss + dt;
    return in == 0 ? kk / (sp * sp) : (sp * sp) / kk;
}

// ---- the state after a swap, tested and stored: the one place where the pieces above are put together ----
// What swap_move reads and swap_store writes of a reserve-kind segment: the arrays the new state is computed from, as the quotes see
// them, and the same arrays again, writable.  Filled from a launch's own arguments (swap_kernel, swap_out_kernel) or from a
// record of the swap-path table.
struct SwapView {
    const double2* R;            // two-coin kinds: reserves, fees
    const double* gamma;
    const double* nR;            // weighted / Curve: the four columns of NCoinPools the quotes read, and the coin count
    const double* nq;
    const double2* nglg;
    const double* npar;
    int n_coins;
    double2* R_new;              // two-coin kinds: [m] reserves
    double2* Q_new;              // GeometricMean: [m] {Q1, Q2}, and η
    const double* eta;
    double* nR_new;              // weighted / Curve: [n_coins][m]
    double* nq_new;
    int* left_window;            // <- 1 when a new reserve lies outside [2^-kFastExp, 2^kFastExp], or null
};
__host__ __device__ __forceinline__ SwapView swap_view(const SwapArgs& s, const NCoinPools& n)
{
    return SwapView{s.q.R, s.q.gamma, n.R, n.q, n.glg, n.par, n.n_coins, s.R, s.Q, s.eta, s.ncR, s.ncq, s.left_window};
}
__host__ __device__ __forceinline__ SwapView swap_view(const SwapPathSeg& t)
{
    return SwapView{t.s.R, t.s.gamma, t.s.nR, t.s.nq, t.s.nglg, t.s.npar, t.s.n_coins, t.R, t.Q, t.eta, t.nR, t.nq, t.left_window};
}

// The state pool `row` of a reserve-kind segment of m pools is left in by a swap of amt > 0 of coin ci for out of coin co:
// swap_move computes it and, with TEST, says whether cfmm_pools_set_* accepts it (the refusal conditions of every moving
// entry); swap_store writes one that was accepted.  TEST false is for a caller that only stores (pass 2 of the path kernels,
// whose pass 1 saw the test pass on the same values): no test is evaluated, Curve's range test with its loads included, and
// `valid` is true.
struct SwapMove {
    double2 rn;                  // {R_in', R_out'}
    double g;                    // the fee it was computed with
    double qi, qo;               // weighted / Curve: the two coins' refreshed constants
    bool valid;
};
template <int KIND, bool TEST = true>
__host__ __device__ __forceinline__ SwapMove swap_move(const SwapView& t, int64_t m, int64_t row, int ci, int co, double amt, double out)
{
    SwapMove mv;
    mv.valid = true;
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        const double2 R = t.R[row];
        mv.g = t.gamma[row];
        mv.rn = swap_reserves(ci == 0 ? R.x : R.y, co == 0 ? R.x : R.y, mv.g, amt, out);
        mv.qi = mv.qo = 0.0;
        if constexpr (TEST) mv.valid = swap_reserves_valid(mv.rn, KIND == CFMM_KIND_SOLIDLY);
    } else {
        static_assert(KIND == CFMM_KIND_WEIGHTED || KIND == CFMM_KIND_CURVE, "UniV3 has no state the kernel writes");
        const int64_t ji = (int64_t)ci * m + row, jo = (int64_t)co * m + row;
        mv.g = t.nglg[row].x;
        mv.rn = swap_reserves(t.nR[ji], t.nR[jo], mv.g, amt, out);
        if constexpr (TEST) mv.valid = swap_reserves_valid(mv.rn, false);
        if constexpr (KIND == CFMM_KIND_WEIGHTED) {
            mv.qi = swap_weighted_q(mv.rn.x, t.npar[ji]);
            mv.qo = swap_weighted_q(mv.rn.y, t.npar[jo]);
        } else {
            mv.qi = swap_curve_q(mv.rn.x);
            mv.qo = swap_curve_q(mv.rn.y);
            if constexpr (TEST) {
                const double2 ab = reinterpret_cast<const double2*>(t.npar)[row];   // {α, log β}
                if (mv.valid && ab.x > 0.0) mv.valid = swap_curve_in_range(ab.y, t.nq + row, m, t.n_coins, ci, mv.qi, co, mv.qo);
            }
        }
    }
    return mv;
}
template <int KIND>
__host__ __device__ __forceinline__ void swap_store(const SwapView& t, int64_t m, int64_t row, int ci, int co, const SwapMove& mv)
{
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        const double2 Rn = ci == 0 ? mv.rn : make_double2(mv.rn.y, mv.rn.x);
        t.R_new[row] = Rn;
        if (t.left_window && !(swap_in_window(Rn.x) && swap_in_window(Rn.y))) *t.left_window = 1;
        if constexpr (KIND == CFMM_KIND_GEOMEAN) t.Q_new[row] = swap_geomean_q(mv.g, t.eta[row], Rn.x, Rn.y);
    } else {
        const int64_t ji = (int64_t)ci * m + row, jo = (int64_t)co * m + row;
        t.nR_new[ji] = mv.rn.x;
        t.nR_new[jo] = mv.rn.y;
        t.nq_new[ji] = mv.qi;
        t.nq_new[jo] = mv.qo;
    }
}

} // namespace cfmm
