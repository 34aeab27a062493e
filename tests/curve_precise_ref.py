"""The 60-digit Curve (StableSwap) fixture tests/golden/curve_precise.npz (made by tests/golden/make_curve_golden.py) and
the scale-aware error bounds its tests assert.  numpy only.

Every bound is K·u·scale with u = 2⁻⁵³; `scale` returns the scale (the bound at K = 1), computed from the inputs and the
truth alone, never from the output under test.  Two parts, per trade:

  Conditioning.  cΔ_k, cΛ_k = Σ_j |x_j·∂T_k/∂x_j| over the 2N + 3 inputs (R_k, v_k, α, β, γ), evaluated by the generator
  in mpmath (central differences at a relative step of 1e-20, each solve to 1e-50).  The device stops on E2's own
  residual, 4·(N + 2)·eps of the size of E2's terms: a backward-error criterion, so the trade it returns is the exact
  trade of inputs perturbed by a few u, and differs from the truth by a few u times this sum.  It is what makes the
  drained and stiff pools, where a relative perturbation of one reserve moves a trade by orders of magnitude more than
  itself, carry a bound that is honest about them.

  Log space.  The solve works on log r_k = max(min(L − a_k^λ, ρ_k), L − a_k^δ): ρ_k = log R_k, log β and L carry an
  absolute error of ≈ u·|their value|, and the outer unknown s its own u·|s*|.  r_k = e^{log r_k} then has a relative
  error of κ·u with κ = 1 + |ln γ| + |ln β| + max_k |ρ_k| + |s*|, and a trade, formed as R_k·expm1(log r_k − ρ_k), an
  absolute error of κ·u·(r*_k + R_k) (the ulp of R_k: the subtraction happens in the exponent).  Δ divides by γ.

Hence, per unit of K, with r* = R + γΔ* − Λ*:
        |Δ_k − Δ*_k| <= u·(κ·(r*_k + R_k)/γ + cΔ_k),      |Λ_k − Λ*_k| <= u·(κ·(r*_k + R_k) + cΛ_k).

Range.  The device refuses at upload, with CFMM_ERR_INVALID_ARG, a pool with α > 0 whose log(P₀/R_k) = log β − Σρ − ρ_k
lies outside ±CURVE_LOG_RANGE for some k (P₀/R_k, the β-term of ∇φ_k, is formed in linear space; the solve starts
from it).  A pool with α = 0 is Product: its trades do not depend on β, and the upload replaces a log β outside that range
by Σρ + mean ρ (`solve_lbeta`).  `refused` predicts the first from the inputs; `ref_out_of_range` the pools where
tests/curve_ref.py, which forms the same quantities in float64 and has no such replacement, cannot meet the bound.
"""
import os

import numpy as np

U = 2.0 ** -53
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curve_precise.npz")
CURVE_LOG_RANGE = 600.0    # curve_pool.h kCurveLogRange


def load():
    """-> (cases, class names); a case is a dict of arrays: v [n] (v2 on one case), R, Ai [m, N]; alpha, beta, gamma,
    cls, s [m]; the truth D, L and the conditioning cD, cL [m, N]."""
    z = np.load(PATH)
    cases = {}
    for name in z["cases"]:
        name = str(name)
        cases[name] = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    return cases, [str(c) for c in z["classes"]]


def _x(R, beta):
    """log(P₀/R_k) = log β − Σρ − ρ_k [m, N]"""
    rho = np.log(R)
    return (np.log(beta) - rho.sum(axis=1))[:, None] - rho


def refused(R, alpha, beta):
    """[m] bool: the pools the upload refuses (α > 0 and some |log(P₀/R_k)| > CURVE_LOG_RANGE)."""
    return (np.asarray(alpha) > 0) & np.any(np.abs(_x(R, beta)) > CURVE_LOG_RANGE, axis=1)


def ref_out_of_range(R, alpha, beta):
    """[m] bool: pools whose P₀/R_k leaves the float64 range the reference solver forms it in (margin: e^±600)."""
    return np.any(np.abs(_x(R, beta)) > CURVE_LOG_RANGE, axis=1)


def solve_lbeta(R, alpha, beta):
    """[m] log β as the device's solve takes it (curve_pool.h curve_solve_lbeta)."""
    rho = np.log(R)
    lb = np.log(beta)
    swap = (np.asarray(alpha) == 0) & np.any(np.abs(_x(R, beta)) > CURVE_LOG_RANGE, axis=1)
    return np.where(swap, rho.sum(axis=1) + rho.sum(axis=1) / R.shape[1], lb)


def scale(c, rows=slice(None)):
    """Bounds at K = 1 for the trades of a case (or its rows) -> (bD, bL) [m, N]."""
    R, g, beta = c["R"][rows], c["gamma"][rows][:, None], c["beta"][rows]
    D, L = c["D"][rows], c["L"][rows]
    rho = np.log(R)
    kappa = 1.0 + np.abs(np.log(g)) + np.abs(np.log(beta))[:, None] + np.max(np.abs(rho), axis=1, keepdims=True) \
        + np.abs(c["s"][rows])[:, None]
    rs = (R + g * D - L) + R
    return U * (kappa * rs / g + c["cD"][rows]), U * (kappa * rs + c["cL"][rows])


def ratios(D, L, Dt, Lt, bD, bL):
    """Per-pool normalised error max(|Δ − Δ*|/bD, |Λ − Λ*|/bL): the K this pool needs.  NaN / Inf -> inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.maximum(np.abs(D - Dt) / bD, np.abs(L - Lt) / bL)
    e = np.where(np.isfinite(e), e, np.inf)
    return e.max(axis=1)


def class_max(r, cls, names):
    """{class name: max ratio} over the classes present."""
    return {names[c]: float(np.max(r[cls == c])) for c in np.unique(cls)}
