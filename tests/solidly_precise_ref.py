"""The 60-digit fixture of Solidly-style stable pairs, tests/golden/solidly_precise.npz (made by
tests/golden/make_solidly_golden.py), and the scale-aware error bounds its tests assert.  numpy only.

Every bound is K·u·scale with u = 2⁻⁵³; `scale` returns the scale (the bound at K = 1), computed from the inputs and the
truth alone, never from the output under test.  In the frame of the tendered coin a and the received coin b, with
x′* = r_a + γΔ*, y′* = r_b − Λ* the exact new reserves:

  Conditioning.  cΔ, cΛ = Σ_j |x_j·∂T/∂x_j| over the five inputs R₁, R₂, γ, v₁, v₂, evaluated by the generator in mpmath
  (central differences at a relative step of 1e-20).  The first operations of the closed form -- the direction test,
  c³ = (v_a − γ·v_b)/(v_a + γ·v_b), t₀ = r_b/r_a -- round their results by a relative u each, which is the exact result
  for inputs perturbed by about u: the trade moves by u times this sum.  This is what makes the balanced pools (p′(1) = 0:
  a price 1e-9 from parity moves t by 1e-3), the band edges and the drained pools carry a bound that is honest about them.

  Forward rounding.  The new reserve is formed as x′ = r_a·(N(t₀)/N(t))^¼, N(t) = t(1 + t²), y′ = t·x′, and the trades as
  x′ − r_a and r_b − y′.  Counting the roundings after c³ with their first-order weights: cbrt 1, the two quadratics
  1 ± c + c² about 2 each (they lie in [3/4, 3] and are sums of terms <= 1), three products and a quotient for t: about
  9u on t in the worst case; N(t) carries 3·(that) + 3, the fourth root quarters it, the two square roots and the product
  add 3: about 11u on x′ and 20u on y′ if every rounding were at its maximum and of the same sign, and √(Σ weights²) ≈ 4u
  for roundings of random sign.  κ = 4 is that root-sum-square figure: at K = 1 the bound is what a typical evaluation of
  the closed form shows, K = 4 its first-order worst case.  The subtraction adds the ulp of the larger operand, hence
  (x′* + r_a) and (y′* + r_b).  Δ divides by γ.

Hence, per unit of K:
        |Δ − Δ*| <= u·(κ·(x′* + r_a)/γ + cΔ),      |Λ − Λ*| <= u·(κ·(y′* + r_b) + cΛ).
Both bounds are evaluated for both coins of a pool (the coin that is not tendered has Δ* = +0.0 and cΔ = 0, and likewise
Λ), which covers an evaluation that -- within a few ulps of a band edge -- decides the direction test the other way; a
pool inside the band stores the conditioning of whichever direction a perturbation opens.
"""
import os

import numpy as np

U = 2.0 ** -53
KAPPA = 4.0
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solidly_precise.npz")


def load():
    """-> (case, class names); the case is a dict of arrays: v [n]; R, Ai (1-based) [m, 2]; gamma, cls, dir [m]; the
    truth D, L and the conditioning cD, cL [m, 2] (zero on the coin that does not trade)."""
    z = np.load(PATH)
    c = {k: z[k] for k in ("v", "R", "gamma", "cls", "dir")}
    c["Ai"] = z["Ai"].astype(np.int64)
    d1, d2 = z["dir"] == 1, z["dir"] == 2
    zero = np.zeros(len(d1))
    pair = lambda a, on1, on2: np.stack([np.where(on1, a, zero), np.where(on2, a, zero)], axis=1)
    c["D"], c["cD"] = pair(z["d"], d1, d2), pair(z["cd"], d1, d2)
    c["L"], c["cL"] = pair(z["l"], d2, d1), pair(z["cl"], d2, d1)
    # a pool inside the band (dir 0) stores the conditioning of whichever direction a perturbation opens: on both coins
    idle = z["dir"] == 0
    c["cD"][idle] = z["cd"][idle][:, None]
    c["cL"][idle] = z["cl"][idle][:, None]
    return c, [str(n) for n in z["classes"]]


def scale(c, rows=slice(None)):
    """Bounds at K = 1 for the trades of the case (or its rows) -> (bD, bL) [m, 2]."""
    R, g = c["R"][rows], c["gamma"][rows][:, None]
    D, L = c["D"][rows], c["L"][rows]
    new = R + g * D - L                                  # {x′*, y′*} in the pool's own coin order
    return U * (KAPPA * (new + R) / g + c["cD"][rows]), U * (KAPPA * (new + R) + c["cL"][rows])


def ratios(D, L, Dt, Lt, bD, bL):
    """Per-pool normalised error max(|Δ − Δ*|/bD, |Λ − Λ*|/bL): the K this pool needs.  NaN / Inf -> inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.maximum(np.abs(D - Dt) / bD, np.abs(L - Lt) / bL)
    e = np.where(np.isfinite(e), e, np.inf)
    return e.max(axis=1)


def class_max(r, cls, names):
    """{class name: max ratio} over the classes present."""
    return {names[c]: float(np.max(r[cls == c])) for c in np.unique(cls)}


def k_of(ratio, cap):
    """The rule of the fixture tests: the next power of two >= 2× the worst ratio of the numpy reference, at most `cap`."""
    k = 1.0
    while k < 2.0 * ratio:
        k *= 2.0
    return min(k, float(cap))
