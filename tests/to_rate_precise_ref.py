"""The amount to a target rate against an 80-digit truth: the fixture's loader, the two bounds, the two K tables and a numpy
restatement of the forms of csrc/to_rate_pool.h (the instrument K was measured with).  No device, no library: plain numpy.

The truth (tests/golden/make_to_rate_golden.py -> tests/golden/to_rate_precise.npz): per pool and coin pair of
tests/golden/quote_precise.npz and per limit r (a double), the a >= 0 with rate(a) = r, rate = γ·(∂φ/∂R_in)/(∂φ/∂R_out) at the
state the trade leaves, solved at 80 digits from φ itself and certified by a sign change of rate − r around the root (60
digits); 0 where the spot rate is <= r.  Stored as the nearest double.
ONE EXCEPTION to "never the closed forms": UniV3.  Inside a tick the invariant IS x·y = k, so the rate γ·y′/x′ = γk/x′² falls to r
at x′ = √(γk/r) -- a two-line consequence of φ that the truth takes in mpmath and the code takes in doubles (in its ratio-minus-one
form).  What is independent there is the rest: the ticks rebuilt from the reference's parametrisation in mpmath, the walk across
the records, and the handling of boundaries, empty ranges and the capacity.

The bound on the AMOUNT, the project's convention:
    |a − a*|  <=  K·u·( a*  +  Σ_j |x_j · ∂a/∂x_j| ),          u = 2^-53
the conditioning sum (`cond`) over the inputs tests/rate_precise_ref.py lists per family, with the limit r in the place of
the amount.  By the implicit function theorem ∂a/∂x_j = −(∂rate/∂x_j)/(∂rate/∂a) and ∂a/∂r = 1/(∂rate/∂a).

The bound on the ROUND TRIP in rate space: |rate(a) − r| <= K·u·(r + rcond), rcond the conditioning sum of the rate at the
truth (tests/rate_precise_ref.py's bound, evaluated at a*), rate(a) what the same build's rate function answers for the
amount it returned.  This is the well-conditioned direction where a itself is ill-conditioned (a stiff Curve pool, a balanced
Solidly pair: ∂rate/∂a is tiny, cond is huge and the bound on a says little).  Held on the rows flagged `interior`: truth
> 0 and, on UniV3, the limit reached strictly inside a tick (at a boundary, in an empty tick's range and at the capacity the
rate jumps past r).

K per (family, class), both tables: the restatement below is run over the fixture on the CPU; K is the next power of two >=
2x its worst ratio in the class, at least 1, capped at 16 on `typical` and 64 elsewhere.  The host build of to_rate_pool.h
and the device are held to the same K.  python tests/to_rate_precise_ref.py prints both tables.
"""
import os

import numpy as np

import quote_precise_ref as P
import rate_precise_ref as RP

FIXTURE = os.path.join(P.ROOT, "tests", "golden", "to_rate_precise.npz")
U = P.U
GROUPS = P.GROUPS
CURVE_ITERS = 128   # csrc/to_rate_pool.h kToRateCurveIters

# worst ratio |a − a*| / (u·(a* + cond)) of the numpy restatement per (family, class)
K_MEASURED = {
    ('curve', 'alpha0'): 1.17,
    ('curve', 'huge'): 0.563,
    ('curve', 'lopsided'): 0.443,
    ('curve', 'low_gamma'): 0.703,
    ('curve', 'small_a'): 1.29,
    ('curve', 'stiff'): 0.82,
    ('curve', 'tiny'): 0.735,
    ('curve', 'typical'): 0.959,
    ('geomean', 'huge'): 1.26,
    ('geomean', 'lopsided'): 2.09,
    ('geomean', 'low_gamma'): 1.91,
    ('geomean', 'tiny'): 0.855,
    ('geomean', 'typical'): 3.46,
    ('geomean', 'w02_98'): 5.52,
    ('product', 'huge'): 0.592,
    ('product', 'lopsided'): 0.662,
    ('product', 'low_gamma'): 0.96,
    ('product', 'tiny'): 1.09,
    ('product', 'typical'): 0.964,
    ('solidly', 'balanced'): 1.39,
    ('solidly', 'huge'): 1.93,
    ('solidly', 'lopsided'): 1.42,
    ('solidly', 'low_gamma'): 1.27,
    ('solidly', 't0_hi'): 1.1,
    ('solidly', 't0_lo'): 1.16,
    ('solidly', 'tiny'): 1.97,
    ('solidly', 'typical'): 1.7,
    ('univ3', 'boundary_dn'): 0.212,
    ('univ3', 'boundary_up'): 0.343,
    ('univ3', 'depth1'): 0.367,
    ('univ3', 'depth4'): 0.459,
    ('univ3', 'depth5'): 0.119,
    ('univ3', 'depth64'): 0.0618,
    ('univ3', 'empty_current'): 0.0623,
    ('univ3', 'empty_in_path'): 0.235,
    ('univ3', 'exhausted'): 0.699,
    ('univ3', 'in_tick'): 0.395,
    ('univ3', 'last_tick'): 0.499,
    ('univ3', 'spot'): 0,
    ('weighted', 'huge'): 1.71,
    ('weighted', 'lopsided'): 3.04,
    ('weighted', 'low_gamma'): 0.895,
    ('weighted', 'pairs'): 1.67,
    ('weighted', 'tiny'): 2.52,
    ('weighted', 'typical'): 2.44,
    ('weighted', 'w02_98'): 5.62,
}
# worst ratio |rate(a) − r| / (u·(r + rcond)) of the numpy restatement per (family, class), on the `interior` rows
K_MEASURED_RATE = {
    ('curve', 'alpha0'): 0.588,
    ('curve', 'huge'): 0.465,
    ('curve', 'lopsided'): 0.183,
    ('curve', 'low_gamma'): 0.257,
    ('curve', 'small_a'): 1.12,
    ('curve', 'stiff'): 0.645,
    ('curve', 'tiny'): 0.243,
    ('curve', 'typical'): 0.514,
    ('geomean', 'huge'): 0.947,
    ('geomean', 'lopsided'): 1.88,
    ('geomean', 'low_gamma'): 2,
    ('geomean', 'tiny'): 1.19,
    ('geomean', 'typical'): 3.32,
    ('geomean', 'w02_98'): 5.39,
    ('product', 'huge'): 0.903,
    ('product', 'lopsided'): 1.17,
    ('product', 'low_gamma'): 0.801,
    ('product', 'tiny'): 0.622,
    ('product', 'typical'): 1.18,
    ('solidly', 'balanced'): 1.25,
    ('solidly', 'huge'): 1.82,
    ('solidly', 'lopsided'): 1.21,
    ('solidly', 'low_gamma'): 1.38,
    ('solidly', 't0_hi'): 0.922,
    ('solidly', 't0_lo'): 2.01,
    ('solidly', 'tiny'): 2.42,
    ('solidly', 'typical'): 2.03,
    ('univ3', 'boundary_dn'): 0,
    ('univ3', 'boundary_up'): 0,
    ('univ3', 'depth1'): 0.152,
    ('univ3', 'depth4'): 0.0979,
    ('univ3', 'depth5'): 0.0902,
    ('univ3', 'depth64'): 0,
    ('univ3', 'empty_current'): 0.204,
    ('univ3', 'empty_in_path'): 0,
    ('univ3', 'exhausted'): 0,
    ('univ3', 'in_tick'): 0.463,
    ('univ3', 'last_tick'): 0.38,
    ('univ3', 'spot'): 0,
    ('weighted', 'huge'): 2.23,
    ('weighted', 'lopsided'): 3.03,
    ('weighted', 'low_gamma'): 0.93,
    ('weighted', 'pairs'): 1.95,
    ('weighted', 'tiny'): 2.28,
    ('weighted', 'typical'): 2.29,
    ('weighted', 'w02_98'): 5.84,
}
K_CAP_TYPICAL, K_CAP = 16, 64


def _K(table, group, cls):
    worst = table[(P.family(group), cls)]
    k = max(1, P.next_pow2(2.0 * worst))
    cap = K_CAP_TYPICAL if cls == "typical" else K_CAP
    assert k <= cap, f"{group}/{cls}: K = {k} exceeds the cap {cap}: a finding about the form, not a reason to raise the cap"
    return k


def K_of(group, cls):
    return _K(K_MEASURED, group, cls)


def K_rate_of(group, cls):
    return _K(K_MEASURED_RATE, group, cls)


def load():
    """(the quote fixture, the to-rate fixture)"""
    z = np.load(FIXTURE, allow_pickle=False)
    return P.load(), {k: z[k] for k in z.files}


def group(fxs, g):
    """the rows of one group: the fixture's columns (r, a, cond, rcond, interior, cls, ...) and, per row, the pool and the
    coin pair of the quote fixture's row it was made from (UniV3: the pools, pool, cin)"""
    qfx, tfx = fxs
    q = P.group(qfx, g)
    r = {k[len(g) + 1:]: v for k, v in tfx.items() if k.startswith(g + "_")}
    names = [str(s) for s in tfx["classes"]]
    r["cls"] = np.array([names[c] for c in r["cls"]])
    if g == "univ3":
        for k in ("current_price", "pool_gamma", "tick_off", "lower_ticks", "liquidity"):
            r[k] = q[k]
        return r
    for k in ("R", "gamma", "cin", "cout", "w", "alpha", "beta"):
        if k in q:
            r[k] = q[k][r["row"]]
    return r


def ratios(a, g):
    """|a − a*| in units of u·(a* + cond), per row.  A zero unit asks for exactly the truth."""
    a = np.asarray(a, dtype=np.float64)
    err, unit = np.abs(a - g["a"]), U * (g["a"] + g["cond"])
    with np.errstate(all="ignore"):
        exact = (a == g["a"])   # (+inf capacity rows: inf − inf is no number)
        return np.where(exact, 0.0, np.where(unit > 0.0, err / unit, np.inf))


def rate_ratios(rate_back, g):
    """|rate(a) − r| in units of u·(r + rcond) on the interior rows, 0 elsewhere"""
    rate_back = np.asarray(rate_back, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(g["interior"], np.abs(rate_back - g["r"]) / (U * (g["r"] + g["rcond"])), 0.0)


# ---------------------------------------------------------------------------------------------------------------
# numpy restatement of csrc/to_rate_pool.h (same operation order, numpy's libm), one row at a time
# ---------------------------------------------------------------------------------------------------------------
F = np.float64


def _sqrt1pm1(d):
    return d / (np.sqrt(F(1.0) + d) + F(1.0))


def t_product(Ri, Ro, g, r):
    s = RP.r_product(Ri, Ro, g, F(0.0))
    if s <= r:
        return F(0.0)
    return (Ri * _sqrt1pm1((s - r) / r)) / g


def t_weighted(Ri, Ro, wi, wo, g, r):
    s = RP.r_weighted(Ri, Ro, wi, wo, g, F(0.0))
    if s <= r:
        return F(0.0)
    d = (s - r) / r
    return (Ri * np.expm1(np.log1p(d) / (F(1.0) + wi / wo))) / g


def t_solidly(Ri, Ro, g, r):
    s = RP.r_solidly(Ri, Ro, g, F(0.0))
    if s <= r:
        return F(0.0)
    rho = r / g
    if rho < 1.0:
        u = np.tanh(np.arctanh(rho) / F(3.0))
    elif rho > 1.0:
        u = F(1.0) / np.tanh(np.arctanh(F(1.0) / rho) / F(3.0))
    else:
        u = rho
    t0 = Ro / Ri
    q = ((t0 - u) * ((F(1.0) + t0 * t0) + (t0 * u + u * u))) / (u * (F(1.0) + u * u))
    a = (Ri * np.expm1(F(0.25) * np.log1p(q))) / g
    return F(0.0) if a < 0.0 else a


def t_curve(Ri, Ro, srho, alpha, lbeta, g, r):
    """-> (a, evaluations of the rate)"""
    rate = lambda a: F(RP.r_curve(Ri, Ro, srho, alpha, lbeta, g, a))   # noqa: E731
    s = rate(F(0.0))
    if s <= r:
        return F(0.0), 1
    hi = (Ri * _sqrt1pm1((s - r) / r)) / g
    lo, flo = F(0.0), s - r
    n = 1
    fhi = rate(hi) - r
    n += 1
    noise = F(2.0 ** -52) * r
    if -noise <= fhi <= noise:
        return hi, n
    if fhi > 0.0:
        f = F(4.0)
        while fhi > 0.0 and n < CURVE_ITERS:
            lo, flo = hi, fhi
            hi = f * hi
            f = f * f if f < 2.0 ** 32 else F(2.0 ** 64)
            if not hi < np.inf:
                return F(np.inf), n
            fhi = rate(hi) - r
            n += 1
        if not fhi <= 0.0:
            return lo, n
    else:
        f = F(0.25)
        while n < CURVE_ITERS:
            c = f * hi
            f = f * f if f > 2.0 ** -32 else F(2.0 ** -64)
            if not c > 0.0:
                break
            fc = rate(c) - r
            n += 1
            if fc != fc:
                break
            if fc > 0.0:
                lo, flo = c, fc
                break
            hi, fhi = c, fc
    while lo > 0.0 and hi > 4.0 * lo and n < CURVE_ITERS:
        c = np.sqrt(lo) * np.sqrt(hi)
        fc = rate(c) - r
        n += 1
        if fc != fc:
            break
        if fc > 0.0:
            lo, flo = c, fc
        else:
            hi, fhi = c, fc
    side = 0
    flo_w, fhi_w = flo, fhi
    while n < CURVE_ITERS:
        c = hi - (fhi_w * (hi - lo)) / (fhi_w - flo_w)
        if not (lo < c < hi):
            c = lo + F(0.5) * (hi - lo)
        if not (lo < c < hi):
            break
        fc = rate(c) - r
        n += 1
        if fc != fc:
            break
        if -noise <= fc <= noise:
            lo = c
            break
        if fc > 0.0:
            lo, flo_w = c, fc
            if side == -1:
                fhi_w = F(0.5) * fhi_w
            side = -1
        else:
            hi, fhi_w = c, fc
            if side == 1:
                flo_w = F(0.5) * flo_w
            side = 1
    return lo, n


def t_univ3(prep, g, cin, r):
    """prep: quote_precise_ref.univ3_prepare's records (k, s_in, δmax, s_out, rout, Σδmax, ΣR_out)"""
    cur, up, lo = prep
    s = F(RP.r_univ3(prep, g, cin, F(0.0)))
    if s <= r:
        return F(0.0)
    k = cur[0]
    s_in = cur[1] if cin == 0 else cur[2]
    dmax = cur[3] if cin == 0 else cur[4]

    def start(k, s_in):
        return g * (k / (s_in * s_in))
    if k != 0.0 and 0.0 < dmax:
        d = s_in * _sqrt1pm1((start(k, s_in) - r) / r)
        if d < dmax:
            return (F(0.0) if d < 0.0 else d) / g
    lst = up if cin == 0 else lo
    cnt = len(lst) - 1
    lo_i, hi_i = -1, cnt
    while hi_i - lo_i > 1:
        mid = lo_i + ((hi_i - lo_i) >> 1)
        if start(lst[mid][0], lst[mid][1]) > r:
            lo_i = mid
        else:
            hi_i = mid
    if lo_i < 0:
        return lst[0][5] / g
    e = lst[lo_i]
    d = e[1] * _sqrt1pm1((start(e[0], e[1]) - r) / r)
    d = F(0.0) if d < 0.0 else (e[2] if d > e[2] else d)
    return (e[5] + d) / g


def restatement(fxs, gname):
    """the numpy forms over one group -> (a [rows], rate(a) [rows], Curve evaluations [rows] or None, the group)"""
    g = group(fxs, gname)
    n = g["r"].size
    a, back = np.empty(n), np.empty(n)
    iters = None
    with np.errstate(all="ignore"):
        if gname == "univ3":
            preps = [P.univ3_prepare(*P.univ3_pool(g, p)[:3]) for p in range(g["current_price"].size)]
            for j in range(n):
                p, ci, gam = int(g["pool"][j]), int(g["cin"][j]), F(g["pool_gamma"][g["pool"][j]])
                a[j] = t_univ3(preps[p], gam, ci, F(g["r"][j]))
                back[j] = RP.r_univ3(preps[p], gam, ci, F(a[j])) if np.isfinite(a[j]) else 0.0
            return a, back, iters, g
        fam = P.family(gname)
        rows = np.arange(n)
        Ri, Ro = g["R"][rows, g["cin"]], g["R"][rows, g["cout"]]
        if fam == "curve":
            iters = np.zeros(n, dtype=np.int64)
            srho, lbeta = P.sum_logs(g["R"]), np.log(g["beta"])
        for j in range(n):
            gam, r = F(g["gamma"][j]), F(g["r"][j])
            if fam == "product":
                a[j] = t_product(Ri[j], Ro[j], gam, r)
                back[j] = RP.r_product(Ri[j], Ro[j], gam, a[j])
            elif fam == "solidly":
                a[j] = t_solidly(Ri[j], Ro[j], gam, r)
                back[j] = RP.r_solidly(Ri[j], Ro[j], gam, a[j])
            elif fam in ("geomean", "weighted"):
                wi, wo = g["w"][j, g["cin"][j]], g["w"][j, g["cout"][j]]
                a[j] = t_weighted(Ri[j], Ro[j], wi, wo, gam, r)
                back[j] = RP.r_weighted(Ri[j], Ro[j], wi, wo, gam, a[j])
            else:
                a[j], iters[j] = t_curve(Ri[j], Ro[j], srho[j], g["alpha"][j], lbeta[j], gam, r)
                back[j] = RP.r_curve(Ri[j], Ro[j], srho[j], g["alpha"][j], lbeta[j], gam, a[j])
    return a, back, iters, g


def worst_by_class(fxs, outputs=None):
    """({(family, class): worst ratio in a}, {...: worst ratio in rate space}, the largest Curve evaluation count);
    outputs: {group: (a, rate(a))} (default: the numpy restatement)"""
    worst, worst_rate, most = {}, {}, 0
    for gname in GROUPS:
        if outputs is None:
            a, back, iters, g = restatement(fxs, gname)
            if iters is not None:
                most = max(most, int(iters.max()))
        else:
            (a, back), g = outputs[gname], group(fxs, gname)
        r, rr = ratios(a, g), rate_ratios(back, g)
        for c in np.unique(g["cls"]):
            key = (P.family(gname), str(c))
            worst[key] = max(worst.get(key, 0.0), float(np.max(r[g["cls"] == c])))
            worst_rate[key] = max(worst_rate.get(key, 0.0), float(np.max(rr[g["cls"] == c])))
    return worst, worst_rate, most


if __name__ == "__main__":
    w, wr, most = worst_by_class(load())
    print("K_MEASURED = {")
    for key in sorted(w):
        print(f"    {key!r}: {w[key]:.3g},")
    print("}\nK_MEASURED_RATE = {")
    for key in sorted(wr):
        print(f"    {key!r}: {wr[key]:.3g},")
    print("}\n# largest Curve evaluation count:", most)
