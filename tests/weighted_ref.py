"""CPU reference for N-coin weighted geometric-mean pools (GeometricMean / Product, src/cfmms.jl:57-64).

An independent solver of the problem of the reference's find_arb! docstring (src/cfmms.jl:21-33):
maximise Σ v_k(λ_k − δ_k) subject to Π (R_k + γδ_k − λ_k)^{w_k} >= Π R_k^{w_k}.  The KKT conditions with
multiplier e^t give R_k'(t) = R_k exp(min(0, t − s_k^λ) + max(0, t − s_k^δ)), s_k^λ = log(R_k v_k / w_k),
s_k^δ = s_k^λ − log γ; t* is the root of G(t) = Σ w_k [min(0, t − s_k^λ) + max(0, t − s_k^δ)].  The device scans G's
breakpoints; this module BISECTS on t instead (vectorised over pools, to machine precision), so the two share
only the optimality conditions, not the algorithm.
"""
import numpy as np


def solve(R, w, gamma, v):
    """R, w, v: [m, n] (v = the prices of each pool's coins); gamma: [m].  -> (Δ, Λ) [m, n]."""
    R = np.asarray(R, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    w = w / w.sum(axis=1, keepdims=True)
    v = np.asarray(v, dtype=np.float64)
    g = np.asarray(gamma, dtype=np.float64).reshape(-1, 1)
    sl = np.log(R) + np.log(v) - np.log(w)
    sd = sl - np.log(g)
    lo = sl.min(axis=1) - 1.0          # G(lo) < 0: every λ term is negative there
    hi = sd.max(axis=1) + 1.0          # G(hi) > 0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        t = mid[:, None]
        G = (w * (np.minimum(t - sl, 0.0) + np.maximum(t - sd, 0.0))).sum(axis=1)
        neg = G < 0
        lo = np.where(neg, mid, lo)
        hi = np.where(neg, hi, mid)
        if np.all(hi - lo <= 4 * np.finfo(float).eps * np.maximum(np.abs(lo), 1.0)):
            break
    t = (0.5 * (lo + hi))[:, None]
    lam = np.where(t < sl, -R * np.expm1(t - sl), 0.0)
    dlt = np.where(t > sd, R * np.expm1(t - sd) / g, 0.0)
    band = sl.max(axis=1) <= sd.min(axis=1)   # inside the fee band: no trade at all
    lam[band] = 0.0
    dlt[band] = 0.0
    return dlt, lam


def sweep(batch, v):
    """One weighted PoolBatch (1-based Ai [m, n]) at global prices v -> (Δ, Λ) [m, n]."""
    Ai0 = batch.Ai - 1
    return solve(batch.R, batch.w, batch.γ, np.asarray(v, dtype=np.float64)[Ai0])


def netflows(D, L, Ai0, n_tokens):
    return np.bincount(np.asarray(Ai0).ravel(), weights=(L - D).ravel(), minlength=n_tokens)[:n_tokens]


def dual_acc(D, L, Ai0, v):
    vl = np.asarray(v, dtype=np.float64)[Ai0]
    return float(np.sum((L * vl).sum(axis=1) - (D * vl).sum(axis=1)))


def optimality_ok(v_local, D, L, R, w, gamma):
    """The reference's optimality predicate (test/cfmms.jl:3-22) for one N-coin pool: primal feasibility, the trading
    function kept (ϕ(R⁺) ≈ ϕ(R), ϕ(R⁺) >= ϕ(R) − √eps) and max γ∇ϕ_i/c_i <= min ∇ϕ_i/c_i + √eps at R⁺ = R + γΔ − Λ."""
    w = np.asarray(w, dtype=np.float64) / np.sum(w)
    Rp = R + gamma * D - L
    se = np.sqrt(np.finfo(float).eps)
    pfeas = bool(np.all(D >= 0) and np.all(L >= 0))
    phi = lambda x: float(np.prod(x ** w))
    pR, pRp = phi(R), phi(Rp)
    sat = bool(np.isclose(pR, pRp, rtol=se, atol=0.0) and pRp >= pR - se)
    grad = w * pRp / Rp
    opt = bool(np.max(gamma * grad / v_local) <= np.min(grad / v_local) + se)
    return pfeas and sat and opt
