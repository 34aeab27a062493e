"""The 60-digit fixture tests/golden/precise.npz (made by tests/golden/make_precise_golden.py) and the scale-aware error
bounds its tests assert.  numpy only.

Every bound is K·u·scale with u = 2⁻⁵³; the functions below return the scale (the bound at K = 1), computed from the
inputs and the truth alone, never from the output under test.

Two-coin pool, one direction with exponent e (η = w₁/w₂ for direction 1, 1/η for direction 2), tendered side r_b
(R₁ / R₂), received side r_a, true new reserves X* = r_b + γΔ*, Y* = r_a − Λ*.  The log-space kernel evaluates
X = exp(A/(e+1)) with A = log γ + log e + log r_a + (log v_out − log v_in) + e·log r_b, Y = X·r_a/c.  Each logarithm
carries a rounding error of u·|its value| and the sum adds the same again, so A is off by ≈ u·Σ|terms|; the division
by e + 1 maps that to a relative error of X of
        κ − 1 = (|ln γ| + |ln η| + |ln v₁| + |ln v₂| + |ln r_a| + e·|ln r_b|)/(e + 1)
(|ln η| for both directions: log(1/η) = −log η), plus a few ulp from exp and the roundings of X·r_a·d/n.  Δ = (X − r_b)/γ
then has an absolute error u·(κ·X* + r_b)/γ per unit of K (the subtraction rounds at the ulp of r_b), and Λ = r_a − Y
likewise u·(κ·Y* + r_a).  The reference-order forms (pow) obey the same bound: the rounding of η = w₁/w₂ and of the pow
exponents costs the same u·e·|ln r| in the exponent.

Weighted pool (N coins): s_k = ln(R_k·v_k/w_k) (normalised w) is formed with an absolute error ≈ u·|s_k|; t* is a
weighted mean of the live s's (plus log γ), so it inherits u·max_k |s_k| and a few ulp from G's sums; λ_k = −R_k·expm1
(t* − s_k), δ_k = R_k·expm1(t* − s_k + ln γ)/γ turn an absolute error ε of the exponent into ε·R_k' with R_k' the new
reserve.  Hence, per unit of K, with κ = 1 + |ln γ| + max_k |s_k|:
        |Δ_k − Δ*_k| <= u·κ·(R_k + γΔ*_k)/γ,      |Λ_k − Λ*_k| <= u·κ·R_k.
"""
import os

import numpy as np

U = 2.0 ** -53
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "precise.npz")


def load():
    """-> (two-coin cases, weighted cases, two-coin class names, weighted class names); a case is a dict of arrays."""
    z = np.load(PATH)
    cases = {}
    for kind in ("gcases", "wcases"):
        out = {}
        for name in z[kind]:
            name = str(name)
            out[name] = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
        cases[kind] = out
    return cases["gcases"], cases["wcases"], [str(c) for c in z["gclasses"]], [str(c) for c in z["wclasses"]]


def _abslog(x):
    return np.abs(np.log(np.asarray(x, dtype=np.float64)))


def two_coin_scale(R, w, g, vp, D, L):
    """Bounds at K = 1 for the trades of [m] two-coin pools: vp [m, 2] = each pool's two prices, D / L the truth
    -> (bD [m, 2], bL [m, 2])."""
    R1, R2, g = R[:, 0], R[:, 1], np.asarray(g, dtype=np.float64)
    eta = w[:, 0] / w[:, 1]
    common = _abslog(g) + _abslog(eta) + _abslog(vp[:, 0]) + _abslog(vp[:, 1])
    k1 = 1.0 + (common + _abslog(R2) + eta * _abslog(R1)) / (eta + 1.0)            # direction 1: e = η,   r_b = R₁
    k2 = 1.0 + (common + _abslog(R1) + _abslog(R2) / eta) / (1.0 / eta + 1.0)      # direction 2: e = 1/η, r_b = R₂
    X1, Y1 = R1 + g * D[:, 0], R2 - L[:, 1]
    X2, Y2 = R2 + g * D[:, 1], R1 - L[:, 0]
    bD = U * np.stack([(k1 * X1 + R1) / g, (k2 * X2 + R2) / g], 1)
    bL = U * np.stack([k2 * Y2 + R1, k1 * Y1 + R2], 1)
    return bD, bL


def weighted_scale(R, w, g, vl, D, L):
    """Bounds at K = 1 for [m, N] weighted pools; vl [m, N] = each coin's price -> (bD, bL) [m, N]."""
    g = np.asarray(g, dtype=np.float64)[:, None]
    wn = w / w.sum(axis=1, keepdims=True)
    s = np.log(R) + np.log(vl) - np.log(wn)
    kappa = 1.0 + np.abs(np.log(g)) + np.max(np.abs(s), axis=1, keepdims=True)
    return U * kappa * (R + g * D) / g, U * kappa * R


def ratios(D, L, Dt, Lt, bD, bL):
    """Per-pool normalised error max(|Δ − Δ*|/bD, |Λ − Λ*|/bL): the K this pool needs.  NaN / Inf -> inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.maximum(np.abs(D - Dt) / bD, np.abs(L - Lt) / bL)
    e = np.where(np.isfinite(e), e, np.inf)
    return e.max(axis=1)


def pow_out_of_range(R, w, g, vp):
    """Pools where the reference-order forms (src/cfmms.jl:180-181 in binary64 pow) take a power outside the normal
    float64 range -- r^η, r^(1/η), or the bases built from them -- predicted from the inputs (margin: 2^±1000)."""
    R1, R2 = np.log2(R[:, 0]), np.log2(R[:, 1])
    eta = w[:, 0] / w[:, 1]
    lg, lm = np.log2(np.asarray(g, dtype=np.float64)), np.log2(vp[:, 1]) - np.log2(vp[:, 0])
    bad = np.zeros(len(R1), dtype=bool)
    for e, la, lb, m in ((eta, R2, R1, lm), (1.0 / eta, R1, R2, -lm)):   # (e, log₂ r_a, log₂ r_b, log₂ m)
        pw = e * lb                                    # r_b^e
        bd = lg + m + np.log2(e) + la + pw             # γ·m·e·r_a·r_b^e
        pa = la / e                                    # r_a^(1/e)
        bl = lb + pa - (np.log2(e) + lg + m)           # (r_b·r_a^(1/e)) / (e·γ·m)
        for x in (pw, bd, pa, bl):
            bad |= np.abs(x) > 1000.0
    return bad


def class_max(r, cls, names):
    """{class name: max ratio} over the classes present."""
    return {names[c]: float(np.max(r[cls == c])) for c in np.unique(cls)}
