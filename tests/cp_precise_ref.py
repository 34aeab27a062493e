"""The 60-digit fixture tests/golden/cp_precise.npz (made by tests/golden/make_cp_precise_golden.py) and the scale-aware
error bounds its tests assert for ProductTwoCoin and UniV3 / BoundedProduct trades.  numpy only, and only + − × / sqrt.

Every bound is K·u·scale with u = 2⁻⁵³; the functions below return the scale (the bound at K = 1), computed from the
inputs and the truth alone, never from the output under test.

ProductTwoCoin, one direction: tendered reserve R_in, received reserve R_out, true new reserves X* = R_in + γΔ* and
Y* = R_out − Λ*.  The reference forms Δ = max(sqrt(γ·m·k) − R_in, 0)/γ and Λ = max(R_out − sqrt(k/(m·γ)), 0)
(src/cfmms.jl:125-126): the argument of each square root is three correctly rounded operations away from exact, the
square root halves their relative error and adds its own, so the root (X* or Y*) is off by about 2u of itself; the
subtraction rounds at the ulp of the larger operand, and the division by γ adds one more rounding.  Per unit of K:
        |Δ − Δ*| <= u·(X* + R_in)/γ,        |Λ − Λ*| <= u·(Y* + R_out).
A direction that does not trade has X* = R_in (Y* = R_out): the bound is the rounding noise of the max(·, 0) test itself.

UniV3: the trade is a sum over ticks of differences of two square-root terms, tick i moving from a = clamp_i(cp) to
b = clamp_i(P).  The reference forms every term as sqrt(k/p) or sqrt(k·p) (two roundings, relative error about 1.5u of
the term) or as k/β (the same), subtracts, and adds the ticks up in walk order; the error of a tick's contribution is a
few u of the LARGER of its two terms, whatever their difference.  So with
        S₁ = Σ √k_i / √min(a, b)      (coin 1: the tendered side when the price falls, the received side when it rises)
        S₂ = Σ √k_i · √max(a, b)      (coin 2: the other one)
summed over the current tick if it is non-empty (it is always evaluated, also when cp sits on its boundary and its own
contribution is zero: there δmax = k/α − (R₂+β) is pure rounding noise of size u·S and is what the reference returns,
src/cfmms.jl:329-332) and over every non-empty tick that [min(cp, P), max(cp, P)] touches, per unit of K:
        price falling   |Δ₁ − Δ₁*| <= u·S₁/γ,   |Λ₂ − Λ₂*| <= u·S₂
        price rising    |Δ₂ − Δ₂*| <= u·S₂/γ,   |Λ₁ − Λ₁*| <= u·S₁.
The partial sums of the walk are bounded by S as well, so no factor for the number of terms is applied.  A pool inside
its no-arbitrage band is given the scale of its current tick in the direction pr = v₁/v₂ lies from cp: a quote within
rounding of the band's edge may trade where the truth does not, by that much.  The direction that does not trade has
scale 0: its outputs must be exactly 0.
"""
import os

import numpy as np

U = 2.0 ** -53
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cp_precise.npz")
# K is capped: 16 on these classes, 64 on every other one
WELL = {"well", "inside", "walk_head", "walk_deep"}
# K per class: the next power of two >= 2x the largest ratio observed (k_from) over the C oracle, the prepared constants
# (profiles/cp_precise_cpu_tests.log) and every device path on an MI355X (profiles/cp_precise_gpu_tests.log)
K_PRODUCT = {"well": 4, "band_edge": 2, "gamma1": 2, "both_live": 2, "wide": 8, "res_out": 4, "px_out": 4}
K_UNIV3 = {"inside": 8, "walk_head": 4, "walk_deep": 2, "drained_all": 8, "on_boundary": 4, "cp_on_tick": 8, "empty_cur": 4,
           "narrow": 8, "band": 4, "gamma": 4, "wide": 4, "res_out": 8}


def load():
    """-> (product cases, UniV3 cases, product class names, UniV3 class names); a case is a dict of arrays."""
    z = np.load(PATH)
    cases = {}
    for kind in ("pcases", "ucases"):
        out = {}
        for name in z[kind]:
            name = str(name)
            out[name] = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
        cases[kind] = out
    return cases["pcases"], cases["ucases"], [str(c) for c in z["pclasses"]], [str(c) for c in z["uclasses"]]


def product_scale(R, g, D, L):
    """Bounds at K = 1 for [m] ProductTwoCoin pools from the truth D / L -> (bD [m, 2], bL [m, 2])."""
    g = np.asarray(g, dtype=np.float64)[:, None]
    bD = U * (2.0 * R + g * D) / g              # X* + R_in, X* = R_in + γΔ*
    bL = U * (2.0 * R - L)                      # Y* + R_out, Y* = R_out − Λ*
    return bD, bL


def univ3_direction(cp, g, vp):
    """-> (falling [m] bool: pr = v₁/v₂ lies below cp, P [m]: the target marginal price, cp inside the band)"""
    pr = vp[:, 0] / vp[:, 1]
    P = np.where(pr < g * cp, pr / g, np.where(pr > cp / g, g * pr, cp))
    return pr < cp, P


def univ3_scale(c, rows=None, v=None, cp=None):
    """Bounds at K = 1 for the pools `rows` (default: all) of a UniV3 case at prices v (default: the case's)
    -> (bD [m, 2], bL [m, 2]); zero in the direction that does not trade."""
    idx = np.arange(len(c["gamma"])) if rows is None else np.arange(len(c["gamma"]))[rows]
    v = c["v"] if v is None else v
    cp_all = c["cp"] if cp is None else cp
    off, lt_all, lq_all = c["tick_off"], c["lower_ticks"], c["liquidity"]
    bD, bL = np.zeros((len(idx), 2)), np.zeros((len(idx), 2))
    falling, P = univ3_direction(cp_all[idx], c["gamma"][idx], v[c["Ai"][idx] - 1])
    for r, i in enumerate(idx):
        lt, k = lt_all[off[i]:off[i + 1]], lq_all[off[i]:off[i + 1]]
        lo = np.append(lt[1:], 0.0)
        q, p, g = cp_all[i], P[r], c["gamma"][i]
        cur = np.arange(len(lt)) == np.count_nonzero(lt >= q) - 1
        use = (k > 0) & (cur | ((lo <= max(q, p)) & (lt >= min(q, p))))
        a, b = np.clip(q, lo, lt), np.clip(p, lo, lt)
        rk = np.sqrt(k[use])
        s1 = np.sum(rk / np.sqrt(np.minimum(a, b)[use]))
        s2 = np.sum(rk * np.sqrt(np.maximum(a, b)[use]))
        if falling[r]:
            bD[r, 0], bL[r, 1] = U * s1 / g, U * s2
        else:
            bD[r, 1], bL[r, 0] = U * s2 / g, U * s1
    return bD, bL


def ratios(D, L, Dt, Lt, bD, bL):
    """Per-pool normalised error max(|Δ − Δ*|/bD, |Λ − Λ*|/bL): the K this pool needs.  An exact value needs 0 whatever
    the scale; an error where the scale is 0, NaN and Inf -> inf."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        eD, eL = np.abs(D - Dt), np.abs(L - Lt)
        e = np.maximum(np.where(eD == 0, 0.0, eD / bD), np.where(eL == 0, 0.0, eL / bL))
    e = np.where(np.isfinite(e), e, np.inf)
    return e.max(axis=1)


def zero_rows_exact(D, L, zclear):
    """Trades whose truth is zero with the no-trade condition clear by more than 2^-40 must be exactly zero.  zclear [m]
    (UniV3: the whole pool) or [m, 2] (Product: direction 1 = {Δ₁, Λ₂}, direction 2 = {Δ₂, Λ₁})."""
    if zclear.ndim == 1:
        return bool(np.all(D[zclear] == 0) and np.all(L[zclear] == 0))
    return bool(np.all(D[zclear] == 0) and np.all(L[:, ::-1][zclear] == 0))


def class_max(r, cls, names):
    """{class name: max ratio} over the classes present."""
    return {names[c]: float(np.max(r[cls == c])) for c in np.unique(cls)}


def k_from(observed):
    """The project's rule: the next power of two >= 2x the largest ratio observed (at least 1)."""
    k = 1
    while k < 2.0 * observed:
        k *= 2
    return k
