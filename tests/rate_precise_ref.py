"""Marginal rates of the exact-input quotes against an 80-digit truth: the fixture's loader, the bound, the K table and a numpy
restatement of the forms of csrc/rate_pool.h (the instrument K was measured with).  No device, no library: plain numpy.

The truth (tests/golden/make_rate_golden.py -> tests/golden/rate_precise.npz) does not use the project's closed forms: per
row of tests/golden/quote_precise.npz -- and again at a = 0 -- it is γ·(∂φ/∂R_in)/(∂φ/∂R_out) at the state the trade leaves,
the partial derivatives taken numerically of φ itself at the 80-digit root, cross-checked by a central difference of the
80-digit quote (30 digits), stored as the nearest double.

The bound.  rate is a short composition of correctly rounded operations and library functions good to about an ulp, applied
to the state AS THE DEVICE HOLDS IT, so first-order error propagation gives
    |rate − rate*|  <=  K·u·( rate*  +  Σ_j |x_j · ∂rate/∂x_j| ),          u = 2^-53
where rate* covers the rounding of the result and its last operations and the conditioning sum (`cond` in the fixture, from
the truth's side) what a relative perturbation u of every input does.  The inputs are those of tests/quote_precise_ref.py:
    Product, Solidly   R_i, R_o, γ, a
    weighted           R_i, R_o, w_i, w_o, γ, a
    Curve              R_i, R_o, α, γ, a, and the LOGS the device holds: log β and every log R_k enter through
                       P₀ = exp(log β − Σ log R_k): their share is (|log β| + Σ_k |log R_k|)·|∂rate/∂log P₀|
    UniV3              rate = γk/s², s = s_in + γa − Σ_j δmax_j over the drained ticks, δmax_j = k_j/β_j − s_in,j:
                       cond = rate·(1 + |1 − 2γa/s| + 2(γa + s_in + Σ_j (k_j/β_j + s_in,j))/s): k, γ, a, s_in and the
                       prepared constants of every drained tick.  An exhausted ladder has rate* = cond = 0: exactly +0.0.
UniV3 rows flagged `at_boundary` (the exact γa within 2^-40 relative of a Σδmax: the 10 rows of boundary_dn / boundary_up)
carry the rate on either side of the boundary (`rate` behind it, `rate_left` in front, each with its cond); a result is
held to whichever is NEARER.  Nowhere else.

K per (family, class): the numpy restatement below is run over the fixture on the CPU; K is the next power of two >= 2x its
worst ratio in the class, at least 1, capped at 16 on `typical` and 64 elsewhere (the project's convention, as
tests/quote_precise_ref.py).  The host build of rate_pool.h and the device are held to the same K.
Measured worst ratios of the restatement (python tests/rate_precise_ref.py prints them) are in K_MEASURED.
"""
import os

import numpy as np

import quote_precise_ref as P

FIXTURE = os.path.join(P.ROOT, "tests", "golden", "rate_precise.npz")
U = P.U
GROUPS = P.GROUPS

# worst ratio |rate − rate*| / (u·(rate* + cond)) of the numpy restatement per (family, class); see K_of
K_MEASURED = {
    ('curve', 'alpha0'): 0.939,
    ('curve', 'huge'): 0.554,
    ('curve', 'lopsided'): 0.418,
    ('curve', 'low_gamma'): 0.713,
    ('curve', 'small_a'): 0.879,
    ('curve', 'stiff'): 1,
    ('curve', 'tiny'): 0.716,
    ('curve', 'typical'): 0.74,
    ('geomean', 'huge'): 0.514,
    ('geomean', 'lopsided'): 0.475,
    ('geomean', 'low_gamma'): 0.433,
    ('geomean', 'tiny'): 0.318,
    ('geomean', 'typical'): 0.523,
    ('geomean', 'w02_98'): 0.309,
    ('product', 'huge'): 0.445,
    ('product', 'lopsided'): 0.463,
    ('product', 'low_gamma'): 0.452,
    ('product', 'tiny'): 0.463,
    ('product', 'typical'): 0.441,
    ('solidly', 'balanced'): 0.5,
    ('solidly', 'huge'): 0.541,
    ('solidly', 'lopsided'): 0.469,
    ('solidly', 'low_gamma'): 1.26,
    ('solidly', 't0_hi'): 0.598,
    ('solidly', 't0_lo'): 1.66,
    ('solidly', 'tiny'): 0.627,
    ('solidly', 'typical'): 0.884,
    ('univ3', 'boundary_dn'): 0.373,
    ('univ3', 'boundary_up'): 0.767,
    ('univ3', 'depth1'): 0.559,
    ('univ3', 'depth4'): 0.154,
    ('univ3', 'depth5'): 0.0921,
    ('univ3', 'depth64'): 0.0726,
    ('univ3', 'empty_current'): 0.207,
    ('univ3', 'empty_in_path'): 0.227,
    ('univ3', 'exhausted'): 0,
    ('univ3', 'in_tick'): 0.629,
    ('univ3', 'last_tick'): 0.157,
    ('univ3', 'spot'): 0.201,
    ('weighted', 'huge'): 0.302,
    ('weighted', 'lopsided'): 0.37,
    ('weighted', 'low_gamma'): 0.96,
    ('weighted', 'pairs'): 0.324,
    ('weighted', 'tiny'): 0.316,
    ('weighted', 'typical'): 0.613,
    ('weighted', 'w02_98'): 0.359,
}
K_CAP_TYPICAL, K_CAP = 16, 64


def K_of(group, cls):
    """K of a (family, class): next power of two >= 2x the restatement's worst ratio, at least 1, capped."""
    worst = K_MEASURED[(P.family(group), cls)]
    k = max(1, P.next_pow2(2.0 * worst))
    cap = K_CAP_TYPICAL if cls == "typical" else K_CAP
    assert k <= cap, f"{group}/{cls}: K = {k} exceeds the cap {cap}: a finding about the form, not a reason to raise the cap"
    return k


def load():
    """(the quote fixture, the rate fixture)"""
    z = np.load(FIXTURE, allow_pickle=False)
    return P.load(), {k: z[k] for k in z.files}


def group(fxs, g):
    """the rows of one group: the rate fixture's columns (a, out, rate, cond, cls, ...) and, per row, the pool and the query
    of the quote fixture's row it was made from (R, gamma, cin, cout, w, alpha, beta; UniV3: the pools, pool, cin)"""
    qfx, rfx = fxs
    q = P.group(qfx, g)
    r = {k[len(g) + 1:]: v for k, v in rfx.items() if k.startswith(g + "_")}
    names = [str(s) for s in rfx["classes"]]
    r["cls"] = np.array([names[c] for c in r["cls"]])
    if g == "univ3":
        for k in ("current_price", "pool_gamma", "tick_off", "lower_ticks", "liquidity"):
            r[k] = q[k]
        return r
    for k in ("R", "gamma", "cin", "cout", "w", "alpha", "beta"):
        if k in q:
            r[k] = q[k][r["row"]]
    return r


def ratios(rate, g):
    """|rate − rate*| in units of u·(rate* + cond), per row; on the rows flagged at_boundary against whichever of
    (rate, cond) / (rate_left, cond_left) is nearer.  A zero unit (an exhausted ladder) asks for exactly 0: ratio 0 or inf."""
    rate = np.asarray(rate, dtype=np.float64)

    def against(truth, cond):
        err, unit = np.abs(rate - truth), U * (truth + cond)
        with np.errstate(all="ignore"):
            return np.where(unit > 0.0, err / unit, np.where(err == 0.0, 0.0, np.inf))
    r = against(g["rate"], g["cond"])
    if "at_boundary" in g:
        left = against(g["rate_left"], g["cond_left"])
        nearer_left = np.abs(rate - g["rate_left"]) < np.abs(rate - g["rate"])
        r = np.where(g["at_boundary"] & nearer_left, left, r)
    return r


# ---------------------------------------------------------------------------------------------------------------
# numpy restatement of csrc/rate_pool.h (same operation order, numpy's libm)
# ---------------------------------------------------------------------------------------------------------------
def r_product(Ri, Ro, g, a):
    x = g * a
    xp = Ri + x
    return g * ((Ri / xp) * (Ro / xp))


def r_weighted(Ri, Ro, wi, wo, g, a):
    x = g * a
    wr = wi / wo
    yp = Ro * np.exp(-(wr * np.log1p(x / Ri)))
    return g * (wr * (yp / (Ri + x)))


def r_solidly(Ri, Ro, g, a):
    x = g * a
    xp = Ri + x
    t0, r = Ro / Ri, Ri / xp
    r2 = r * r
    c = (t0 * (t0 * t0 + 1.0)) * (r2 * r2)
    hc = 0.5 * c
    s = np.cbrt(hc + np.hypot(hc, 0.19245008972987526))
    u = s - 1.0 / (3.0 * s)
    for _ in range(2):
        uu = u * u
        u = u - (u * (uu + 1.0) - c) / (3.0 * uu + 1.0)
    uu = u * u
    return g * ((u * (3.0 + uu)) / (1.0 + 3.0 * uu))


def r_curve(Ri, Ro, srho, alpha, lbeta, g, a):
    x = g * a
    xp = Ri + x
    P0 = np.exp(lbeta - srho)
    C = alpha * (Ro - x) - P0
    B = (P0 * Ro) * (Ri / xp)
    h = np.hypot(C, 2.0 * (np.sqrt(alpha) * np.sqrt(B)))
    yp = np.where(C < 0.0, (2.0 * B) / (h - C), (C + h) / (2.0 * alpha))
    Pp = (P0 * (Ri / xp)) * (Ro / yp)
    return g * ((alpha + Pp / xp) / (alpha + Pp / yp))


def r_univ3(prep, g, cin, a):
    """prep: quote_precise_ref.univ3_prepare's records"""
    cur, up, lo = prep
    d = g * a
    k = cur[0]
    s_in = cur[1] if cin == 0 else cur[2]
    dmax = cur[3] if cin == 0 else cur[4]

    def tick(k, s_in, d):
        s = s_in + d
        return g * (k / (s * s))
    if k != 0.0 and d < dmax:
        return tick(k, s_in, d)
    lst = up if cin == 0 else lo
    cnt = len(lst) - 1
    lo_i, hi_i = 0, cnt + 1
    while hi_i - lo_i > 1:
        mid = lo_i + ((hi_i - lo_i) >> 1)
        if lst[mid][5] <= d:
            lo_i = mid
        else:
            hi_i = mid
    if lo_i == cnt:
        return 0.0
    e = lst[lo_i]
    return tick(e[0], e[1], d - e[5])


def restatement(fxs, gname):
    """the numpy forms over one group -> (rate [rows], the group)"""
    g = group(fxs, gname)
    if gname == "univ3":
        preps = [P.univ3_prepare(*P.univ3_pool(g, p)[:3]) for p in range(g["current_price"].size)]
        return np.array([r_univ3(preps[p], float(g["pool_gamma"][p]), int(ci), float(a))
                         for p, ci, a in zip(g["pool"], g["cin"], g["a"])]), g
    rows = np.arange(g["a"].size)
    Ri, Ro = g["R"][rows, g["cin"]], g["R"][rows, g["cout"]]
    fam = P.family(gname)
    with np.errstate(all="ignore"):
        if fam == "product":
            rate = r_product(Ri, Ro, g["gamma"], g["a"])
        elif fam == "solidly":
            rate = r_solidly(Ri, Ro, g["gamma"], g["a"])
        elif fam in ("geomean", "weighted"):
            rate = r_weighted(Ri, Ro, g["w"][rows, g["cin"]], g["w"][rows, g["cout"]], g["gamma"], g["a"])
        else:
            rate = r_curve(Ri, Ro, P.sum_logs(g["R"]), g["alpha"], np.log(g["beta"]), g["gamma"], g["a"])
    return rate, g


def worst_by_class(fxs, outputs=None):
    """{(family, class): worst ratio}; outputs: {group: rate} (default: the numpy restatement)"""
    worst = {}
    for gname in GROUPS:
        if outputs is None:
            rate, g = restatement(fxs, gname)
        else:
            rate, g = outputs[gname], group(fxs, gname)
        r = ratios(rate, g)
        for c in np.unique(g["cls"]):
            key = (P.family(gname), str(c))
            worst[key] = max(worst.get(key, 0.0), float(np.max(r[g["cls"] == c])))
    return worst


if __name__ == "__main__":
    w = worst_by_class(load())
    for key in sorted(w):
        print(f"    {key!r}: {w[key]:.3g},")
