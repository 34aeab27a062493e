"""CPU reference for Curve (StableSwap) pools: φ(R) = α·Σ R_k − β·Π R_k⁻¹, α >= 0, β > 0 (src/cfmms.jl:66-70 declares
Curve{T} with α, β and no find_arb!).  StableSwap with its invariant D held fixed is this φ with α = A·nⁿ, β = D^{n+1}/nⁿ.

The problem of the reference's find_arb! docstring (src/cfmms.jl:21-33): maximise Σ v_k(λ_k − δ_k) subject to
φ(R + γδ − λ) >= φ(R), δ, λ >= 0.  With r = R + γδ − λ, multiplier ν = 1/x and P = β/Π r (so ∂φ_k = α + P/r_k) the KKT
conditions give, coin by coin,

    r_k = P/(v_k·x − α)     if that is < R_k     (coin leaves the pool)
    r_k = P/(v_k·x/γ − α)   if that is > R_k     (coin enters the pool)
    r_k = R_k               otherwise,

and two scalar equations remain: (E1) P·Π r_k = β and (E2) α·Σ(r_k − R_k) = P − P₀, P₀ = β/Π R_k.

Two solvers, neither the device's algorithm (which interpolates E1 exactly between its breakpoints and runs a
safeguarded Newton iteration on E2):

  solve_decimal  one pool at a time in `decimal` at 40 digits, NAIVE (ν, P) form: the terms v_k·x − α are formed as
                 they read (40 digits absorb the cancellation of stiff pools).  Outer bisection on x, inner bisection
                 on log P.  Slow; for small sets.
  solve          vectorised float64 for bulk checks.  Outer bisection on u = log(v_min·x/γ − α) (the terms are then
                 sums of non-negative parts plus one difference of exact inputs, no cancellation against α); inner:
                 E1 is piecewise linear in log P, solved exactly by sorting its breakpoints and walking the slopes.

optimality_ok is the KKT predicate both are checked with.
"""
from decimal import Decimal, localcontext

import numpy as np


def _terms(u, cd, ed, el, alpha, gamma):
    """log of the δ- and λ-terms v_k·x/γ − α and v_k·x − α at e^u = v_min·x/γ − α (λ: −inf where the term is <= 0)."""
    eu = np.exp(u)[:, None]
    td = cd * eu + alpha[:, None] * ed
    tl = gamma[:, None] * cd * eu + alpha[:, None] * el
    with np.errstate(divide="ignore", invalid="ignore"):
        ad = np.log(td)
        al = np.where(tl > 0, np.log(np.where(tl > 0, tl, 1.0)), -np.inf)
    return ad, al


def _inner(ad, al, rho, lbeta):
    """log P solving L + Σ max(min(L − al, ρ), L − ad) = log β, exactly: the breakpoints sorted, the left side walked
    from the first one along its slopes (a λ-branch ends at ρ + al: slope −1; a δ-branch starts at ρ + ad: slope +1)."""
    m, n = rho.shape
    bl = rho + al                                    # −inf: the λ-branch is never live
    live_l = np.isfinite(bl)
    bps = np.concatenate([np.where(live_l, bl, np.inf), rho + ad], axis=1)
    dsl = np.concatenate([np.where(live_l, -1.0, 0.0), np.ones((m, n))], axis=1)
    order = np.argsort(bps, axis=1)
    b = np.take_along_axis(bps, order, axis=1)
    slope = 1.0 + live_l.sum(axis=1, keepdims=True) + np.cumsum(np.take_along_axis(dsl, order, axis=1), axis=1)
    b0 = b[:, 0]
    F0 = b0 + np.sum(np.maximum(np.minimum(b0[:, None] - al, rho), b0[:, None] - ad), axis=1) - lbeta
    with np.errstate(invalid="ignore"):
        steps = np.where(np.isfinite(b[:, 1:]), slope[:, :-1] * np.diff(b, axis=1), np.inf)
    F = np.concatenate([F0[:, None], F0[:, None] + np.cumsum(steps, axis=1)], axis=1)   # F at every breakpoint
    j = np.argmax(F >= 0, axis=1)                    # first breakpoint at or past the root (F at +inf is +inf)
    rows = np.arange(m)
    with np.errstate(invalid="ignore"):
        L = np.where(j == 0, b0 - F0 / (1.0 + live_l.sum(axis=1)),                # below every breakpoint
                     b[rows, j - 1] - F[rows, j - 1] / slope[rows, j - 1])        # linear on [b_{j−1}, b_j]
    return L


def _state(u, cd, ed, el, alpha, gamma, rho, lbeta):
    ad, al = _terms(u, cd, ed, el, alpha, gamma)
    L = _inner(ad, al, rho, lbeta)
    lr = np.maximum(np.minimum(L[:, None] - al, rho), L[:, None] - ad)
    return L, lr


def _resid(L, lr, rho, alpha, L0):
    """E2 / scale: α·Σ(r − R) − (P − P₀), every difference through expm1 of a log difference."""
    R = np.exp(rho)
    dr = R * np.expm1(lr - rho)
    dP = np.exp(L0) * np.expm1(L - L0)
    scale = alpha * np.sum(R + np.abs(dr), axis=1) + np.exp(L0) + np.abs(dP)
    return (alpha * np.sum(dr, axis=1) - dP) / scale


def solve(R, alpha, beta, gamma, v):
    """R, v: [m, n]; alpha, beta, gamma: [m].  -> (Δ, Λ) [m, n]."""
    R = np.asarray(R, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    m, n = R.shape
    alpha = np.asarray(alpha, dtype=np.float64).reshape(m)
    gamma = np.asarray(gamma, dtype=np.float64).reshape(m)
    lbeta = np.log(np.asarray(beta, dtype=np.float64).reshape(m))
    rho = np.log(R)
    L0 = lbeta - rho.sum(axis=1)
    vmin = v.min(axis=1, keepdims=True)
    cd = v / vmin
    ed = (v - vmin) / vmin
    el = ed - (1.0 - gamma[:, None]) * cd          # γ·v_k/v_min − 1 (1 − γ is exact for γ in [1/2, 1])
    # no trade iff max γ∇φ_k/v_k <= min ∇φ_k/v_k at R (the fee band)
    grad = alpha[:, None] + np.exp(L0[:, None] - rho)
    band = np.max(gamma[:, None] * grad / v, axis=1) <= np.min(grad / v, axis=1)
    # bracket of u: E2 / scale is decreasing in u; expand from u0 = log(P₀/R_ref)
    u0 = L0 - rho[np.arange(m), np.argmin(v, axis=1)]
    lo, hi = u0 - 1.0, u0 + 1.0
    for k in range(12):
        flo = _resid(*_state(lo, cd, ed, el, alpha, gamma, rho, lbeta), rho, alpha, L0)
        fhi = _resid(*_state(hi, cd, ed, el, alpha, gamma, rho, lbeta), rho, alpha, L0)
        bad_lo, bad_hi = ~(flo > 0), ~(fhi < 0)
        if not (np.any(bad_lo & ~band) or np.any(bad_hi & ~band)):
            break
        lo = np.where(bad_lo, lo - 2.0 ** (k + 1), lo)
        hi = np.where(bad_hi, hi + 2.0 ** (k + 1), hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        pos = _resid(*_state(mid, cd, ed, el, alpha, gamma, rho, lbeta), rho, alpha, L0) > 0
        lo = np.where(pos, mid, lo)
        hi = np.where(pos, hi, mid)
        if np.all(hi - lo <= 2 * np.finfo(float).eps * np.maximum(np.abs(lo), 1.0)):
            break
    L, lr = _state(0.5 * (lo + hi), cd, ed, el, alpha, gamma, rho, lbeta)
    lam = np.where(lr < rho, -R * np.expm1(lr - rho), 0.0)
    dlt = np.where(lr > rho, R * np.expm1(lr - rho) / gamma[:, None], 0.0)
    lam[band] = 0.0
    dlt[band] = 0.0
    return dlt, lam


def sweep(batch, v):
    """One Curve PoolBatch (1-based Ai [m, n]) at global prices v -> (Δ, Λ) [m, n]."""
    return solve(batch.R, batch.α, batch.β, batch.γ, np.asarray(v, dtype=np.float64)[batch.Ai - 1])


def solve_decimal(R, alpha, beta, gamma, v, digits=40):
    """One pool, 40-digit decimal, naive (ν, P) form.  -> (Δ, Λ) as float64 arrays."""
    with localcontext() as ctx:
        ctx.prec = digits
        D = Decimal
        R = [D(float(r)) for r in R]
        v = [D(float(x)) for x in v]
        a, b, g = D(float(alpha)), D(float(beta)) if not isinstance(beta, Decimal) else beta, D(float(gamma))
        n = len(R)
        prodR = D(1)
        for r in R:
            prodR *= r
        P0 = b / prodR
        grad = [a + P0 / r for r in R]
        if max(g * grad[k] / v[k] for k in range(n)) <= min(grad[k] / v[k] for k in range(n)):
            return np.zeros(n), np.zeros(n)
        lb = b.ln()
        rho = [r.ln() for r in R]

        def state(x):
            # inner: bisection on L = log P of L + Σ max(min(L − log(v x − α), ρ), L − log(v x/γ − α)) = log β
            al = [(v[k] * x - a).ln() if v[k] * x - a > 0 else None for k in range(n)]
            ad = [(v[k] * x / g - a).ln() for k in range(n)]

            def lr(L, k):
                t = rho[k] if al[k] is None else min(L - al[k], rho[k])
                return max(t, L - ad[k])

            lo, hi = lb - sum(rho) - 1, lb - sum(rho) + 1
            while lo + sum(lr(lo, k) for k in range(n)) > lb:
                lo -= 2 * (hi - lo)
            while hi + sum(lr(hi, k) for k in range(n)) < lb:
                hi += 2 * (hi - lo)
            for _ in range(4 * digits):
                mid = (lo + hi) / 2
                if mid + sum(lr(mid, k) for k in range(n)) < lb:
                    lo = mid
                else:
                    hi = mid
            L = (lo + hi) / 2
            r = [lr(L, k).exp() for k in range(n)]
            return r, a * sum(r[k] - R[k] for k in range(n)) - (L.exp() - P0)

        xlo = a * g / min(v)           # the δ-term of the cheapest coin vanishes here
        # E2 is decreasing in x; bisect on log(x − xlo), the bracket found by doubling
        ylo, yhi = D(-1), D(1)
        base = max(grad[k] / v[k] for k in range(n))
        while state(xlo + base * ylo.exp())[1] <= 0:
            ylo -= 2 * (yhi - ylo)
        while state(xlo + base * yhi.exp())[1] >= 0:
            yhi += 2 * (yhi - ylo)
        for _ in range(4 * digits):
            mid = (ylo + yhi) / 2
            if state(xlo + base * mid.exp())[1] > 0:
                ylo = mid
            else:
                yhi = mid
        r, _ = state(xlo + base * ((ylo + yhi) / 2).exp())
        lam = [R[k] - r[k] if r[k] < R[k] else D(0) for k in range(n)]
        dlt = [(r[k] - R[k]) / g if r[k] > R[k] else D(0) for k in range(n)]
        return np.array([float(x) for x in dlt]), np.array([float(x) for x in lam])


def netflows(D, L, Ai0, n_tokens):
    return np.bincount(np.asarray(Ai0).ravel(), weights=(L - D).ravel(), minlength=n_tokens)[:n_tokens]


def optimality_ok(v_local, D, L, R, alpha, beta, gamma, rtol=1e-10):
    """KKT at R⁺ = R + γΔ − Λ for one pool: primal feasibility (Δ, Λ >= 0, R⁺ > 0), the constraint tight in its E2 form
    (α·Σ(R⁺ − R) = P⁺ − P₀, which never evaluates φ itself) and the fee band at R⁺: max γ∇φ_k/v_k <= min ∇φ_k/v_k,
    both relative to their own scales."""
    R = np.asarray(R, dtype=np.float64)
    v = np.asarray(v_local, dtype=np.float64)
    Rp = R + gamma * D - L
    if not (np.all(D >= 0) and np.all(L >= 0) and np.all(Rp > 0)):
        return False
    lb = np.log(beta)
    P0, Pp = np.exp(lb - np.sum(np.log(R))), np.exp(lb - np.sum(np.log(Rp)))
    dP = P0 * np.expm1(np.sum(np.log(R)) - np.sum(np.log(Rp)))
    dr = Rp - R
    scale = alpha * np.sum(R + np.abs(dr) + gamma * D + L) + P0 + Pp
    tight = abs(alpha * np.sum(dr) - dP) <= rtol * scale
    g = (alpha + Pp / Rp) / v
    band = np.max(gamma * g) <= np.min(g) + rtol * np.max(g)
    return bool(tight and band)


def optimality_ok_mp(v_local, D, L, R, alpha, beta, gamma, rtol, Rp=None):
    """optimality_ok's conditions in mpmath at the caller's precision, on trades given as mpf (the 60-digit truth before
    it is rounded): primal feasibility, E2 tight and the fee band at R⁺, both relative to their own scales.  Rp: R⁺ itself
    where R + γΔ − Λ would cancel (a coin drained to far below the working precision of its old reserve)."""
    import mpmath as mp
    M = lambda x: x if isinstance(x, mp.mpf) else mp.mpf(float(x))
    R, v, D, L = [M(x) for x in R], [M(x) for x in v_local], [M(x) for x in D], [M(x) for x in L]
    a, b, g = M(alpha), M(beta), M(gamma)
    n = len(R)
    Rp = [R[k] + g * D[k] - L[k] for k in range(n)] if Rp is None else [M(x) for x in Rp]
    if not (all(x >= 0 for x in D + L) and all(x > 0 for x in Rp)):
        return False
    P0, Pp = b / mp.fprod(R), b / mp.fprod(Rp)
    scale = a * mp.fsum(R[k] + abs(Rp[k] - R[k]) + g * D[k] + L[k] for k in range(n)) + P0 + Pp
    tight = abs(a * mp.fsum(Rp[k] - R[k] for k in range(n)) - (Pp - P0)) <= rtol * scale
    gr = [(a + Pp / Rp[k]) / v[k] for k in range(n)]
    band = max(g * x for x in gr) <= min(gr) + rtol * max(gr)
    return bool(tight and band)
