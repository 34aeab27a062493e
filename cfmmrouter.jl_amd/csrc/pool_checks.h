// pool_checks.h -- internal, host only: the checks of a pool's STATE (reserves, Curve's parameters, a UniV3 price) and the
// constants prepared from it, each in one place.  The upload (abi_upload.cpp, cfmm_pools_add_*) applies them to every pool of a
// batch, the sparse update (abi_update.cpp, cfmm_pools_set_*) to the rows it is given: same checks, same order, same error
// texts, same expressions -- an updated pool carries the bits of an uploaded one.  `i` is the pool number an error names.
#pragma once

#include "ctx.h"
#include "curve_pool.h"
#include "univ3_pool.h"

namespace cfmm {

inline int check_reserves(const cfmm_ctx* c, int64_t i, const double* R, int n)
{
    for (int k = 0; k < n; ++k)
        if (!finite_pos(R[k])) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: reserves must be finite and > 0", (long long)i);
    return CFMM_OK;
}

// the closed form cubes R2/R1 (SolidlyOps): 2^±300 cubed is finite, anything wider need not be
inline int check_solidly_range(const cfmm_ctx* c, int64_t i, const double* R)
{
    if (!in_fast_window(R[0]) || !in_fast_window(R[1]))
        return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: reserves of a Solidly stable pair must lie within [2^-%d, 2^%d]",
                    (long long)i, kFastExp, kFastExp);
    return CFMM_OK;
}

// Curve: α >= 0, β > 0, and with α > 0 the pool inside the solve's range; R: the pool's n_coins reserves
inline int check_curve_params(const cfmm_ctx* c, int64_t i, double alpha, double beta, const double* R, int n_coins)
{
    if (!std::isfinite(alpha) || alpha < 0.0)
        return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: alpha must be finite and >= 0", (long long)i);
    if (!finite_pos(beta)) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: beta must be finite and > 0", (long long)i);
    if (alpha > 0.0) {
        double rho[kMaxCoins];
        for (int k = 0; k < n_coins; ++k) rho[k] = std::log(R[k]);
        if (!curve_in_range(std::log(beta), rho, n_coins))
            return fail(c, CFMM_ERR_INVALID_ARG,
                        "pool %lld: log(P0/R_k) = log(beta) - sum log R - log R_k must lie within +-%g when alpha > 0",
                        (long long)i, kCurveLogRange);
    }
    return CFMM_OK;
}

inline int check_univ3_price(const cfmm_ctx* c, int64_t i, double cp)
{
    if (!finite_pos(cp)) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: current_price must be finite and > 0", (long long)i);
    return CFMM_OK;
}
// a pool's ladder of nt >= 1 ticks, tick by tick: the price bound, the ordering, the liquidity
inline int check_univ3_ladder(const cfmm_ctx* c, int64_t i, const double* lt, const double* lq, int64_t nt)
{
    for (int64_t j = 0; j < nt; ++j) {
        if (!finite_pos(lt[j])) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld tick %lld: price must be finite and > 0", (long long)i, (long long)j);
        if (j > 0 && !(lt[j] < lt[j - 1]))
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: lower_ticks must be strictly descending", (long long)i);
        if (!(lq[j] >= 0.0) || !std::isfinite(lq[j]))
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld tick %lld: liquidity must be finite and >= 0", (long long)i, (long long)j);
    }
    return CFMM_OK;
}
// every non-empty tick's liquidity inside the window of the fast arithmetic (Segment::fast_ok)
inline bool univ3_liquidity_in_window(const double* lq, int64_t nt)
{
    bool fast = true;
    for (int64_t j = 0; j < nt; ++j) fast = fast && (lq[j] == 0.0 || in_fast_window(lq[j]));
    return fast;
}
// the pool's current tick (univ3_current_tick) into ct, or the refusal of a price above the first tick
inline int check_univ3_tick(const cfmm_ctx* c, int64_t i, const double* lt, int64_t nt, double cp, int64_t& ct)
{
    ct = univ3_current_tick(lt, nt, cp);
    if (ct < 1)
        return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: current_price above the first tick (the reference would index tick 0)",
                    (long long)i);
    return CFMM_OK;
}

// GeometricMeanTwoCoin: {Q1, Q2}, the v-independent pieces of the log-space closed forms (ops_two_coin.h, GeoMeanLogOps);
// e = η = w1/w2 (src/cfmms.jl:188)
inline double2 geomean_q(double gamma, double e, double r1, double r2)
{
    const double lg = std::log(gamma), le = std::log(e), l1 = std::log(r1), l2 = std::log(r2);
    return make_double2(((lg + le) + l2) + e * l1, e * ((lg + l1) - le) + l2);
}
// weighted: q = log(R / w), w normalised to sum to 1
inline double weighted_q(double r, double wn) { return std::log(r / wn); }
// Curve: q = log R per coin and {α, log β} (curve_solve_lbeta: at α = 0, one that keeps P₀/R_k inside the solve's range)
inline void curve_fill(const double* R, double alpha, double beta, int nc, double* q, double* ab)
{
    for (int k = 0; k < nc; ++k) q[k] = std::log(R[k]);
    ab[0] = alpha;
    ab[1] = curve_solve_lbeta(alpha, std::log(beta), q, nc);
}

} // namespace cfmm
