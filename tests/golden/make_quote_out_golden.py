"""Writes tests/golden/quote_out_precise.npz: exact-output swap quotes of every pool kind with an 80-digit truth (stored as
the nearest double) and the conditioning sum of tests/quote_out_precise_ref.py per row.

Rows: every row of tests/golden/quote_precise.npz -- same state, coins and class -- with o = that fixture's stored `out`,
plus the classes only the inverse has (near_drain, o_gt_Ri, on_boundary, closing_exact, beyond, asymptotic).
The truth is independent of the project's arithmetic: the root `a` of φ(R + γa·e_in − o·e_out) = φ(R), found by bracketing
bisection on φ ITSELF (weighted pools: on log φ = Σ w_k log R_k), and for UniV3 the reference's tick-by-tick walk
(src/cfmms.jl:401-434) inverted tick by tick in mpmath from the ladder.  The closed forms appear here only for three
things: the bracket's upper end, a cross-check of every root (they must agree to 1e-40), and the conditioning sum (mp.diff).
usage: python tests/golden/make_quote_out_golden.py        (needs mpmath; deterministic: seeded)"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quote_out_precise_ref as P  # noqa: E402
import quote_precise_ref as F  # noqa: E402

mp.mp.dps = 80
M = mp.mpf
rng = np.random.default_rng(20240717)
NEW = ["near_drain", "o_gt_Ri", "on_boundary", "closing_exact", "beyond", "asymptotic"]


def root(f, hi):
    """the root of f in (0, hi), f(0) < 0 < f(hi): bisection until the bracket is 1e-72 of the root"""
    lo, hi = M(0), M(hi)
    assert f(lo) < 0 < f(hi)
    for _ in range(400):
        mid = (lo + hi) / 2
        if f(mid) < 0:
            lo = mid
        else:
            hi = mid
        if hi - lo <= hi * M(10) ** -72:
            break
    return (lo + hi) / 2


def phi_weighted(R, w):
    return sum(wk * mp.log(Rk) for Rk, wk in zip(R, w))


def phi_solidly(R):
    x, y = R
    return x ** 3 * y + x * y ** 3


def phi_curve(R, alpha, beta):
    pr = M(1)
    for Rk in R:
        pr *= Rk
    return alpha * sum(R) - beta / pr


def truth(phi, R, g, cin, cout, o, guess):
    R = [M(float(x)) for x in R]
    k0 = phi(R)

    def f(a):
        Rn = list(R)
        Rn[cin] = R[cin] + M(g) * a
        Rn[cout] = R[cout] - M(o)
        return phi(Rn) - k0            # φ is increasing in every reserve: negative below the root
    return root(f, 2 * guess)


# ---- closed forms in mpmath: bracket, cross-check, conditioning ----------------------------------------------------
def cf_product(Ri, Ro, g, o):
    return Ri * o / ((Ro - o) * g)


def cf_weighted(Ri, Ro, wi, wo, g, o):
    return Ri * ((1 - o / Ro) ** (-wo / wi) - 1) / g


def cf_solidly(Ri, Ro, g, o):
    y = Ro - o
    s0 = Ri / Ro
    c = s0 * (1 + s0 * s0) * (Ro / y) ** 4
    s = mp.cbrt(c / 2 + mp.sqrt(c * c / 4 + M(1) / 27))
    return ((s - 1 / (3 * s)) * y - Ri) / g


def cf_curve(Ri, Ro, alpha, lP0, g, o):
    y = Ro - o
    P0 = mp.e ** lP0
    E = alpha * (Ri - o) + P0
    G = Ri * o * (alpha + P0 / y)
    h = mp.sqrt(E * E + 4 * alpha * G)
    return (2 * G / (E + h) if E >= 0 else (h - E) / (2 * alpha)) / g


def cond_sum(f, xs, skip=()):
    """Σ_j |x_j ∂f/∂x_j| over the arguments xs (mp.diff)"""
    s = M(0)
    for j, xj in enumerate(xs):
        if xj == 0 or j in skip:
            continue
        s += abs(xj * mp.diff(lambda t, j=j: f(*[t if k == j else xs[k] for k in range(len(xs))]), xj))
    return s


def check(a, cf, what):
    assert abs(a - cf) <= M(10) ** -40 * max(abs(a), M(10) ** -300), (what, a, cf)


def lognormal(n, sigma=2.0):
    return np.exp(rng.normal(0.0, sigma, n)) * 1e3


# ---- the reserve kinds ----------------------------------------------------------------------------------------------
def solve_row(fam, r):
    """r: dict with R, gamma, cin, cout, o (+ w | alpha, beta) -> (a, cond) in mpmath, a = +inf where o >= R_o"""
    R, g, ci, co, o = r["R"], float(r["gamma"]), int(r["cin"]), int(r["cout"]), float(r["o"])
    Rm = [M(float(x)) for x in R]
    if o >= float(R[co]):
        return mp.inf, M(0)
    if fam == "product":
        phi, cf, xs, skip = (lambda RR: RR[0] * RR[1]), cf_product, [Rm[ci], Rm[co], M(g), M(o)], ()
        if len(Rm) != 2:
            raise ValueError
    elif fam == "solidly":
        phi, cf, xs, skip = phi_solidly, cf_solidly, [Rm[ci], Rm[co], M(g), M(o)], ()
    elif fam in ("geomean", "weighted"):
        wm = [M(float(x)) for x in r["w"]]
        phi, cf, xs, skip = (lambda RR: phi_weighted(RR, wm)), cf_weighted, [Rm[ci], Rm[co], wm[ci], wm[co], M(g), M(o)], ()
    else:
        al, be = M(float(r["alpha"])), M(float(r["beta"]))
        pr = M(1)
        for x in Rm:
            pr *= x
        lP0 = mp.log(be / pr)
        phi, cf, xs, skip = (lambda RR: phi_curve(RR, al, be)), cf_curve, [Rm[ci], Rm[co], al, lP0, M(g), M(o)], (3,)
    guess = cf(*xs)
    if o == 0.0:
        return M(0), M(0)
    a = truth(phi, R, g, ci, co, o, guess)
    check(a, guess, fam)
    cond = cond_sum(cf, xs, skip)
    if fam == "curve":   # the logs the device holds: log β and every log R_k enter through log P₀ (argument 3)
        logs = abs(mp.log(be)) + sum(abs(mp.log(x)) for x in Rm)
        cond += logs * abs(mp.diff(lambda t: cf_curve(xs[0], xs[1], xs[2], t, xs[4], xs[5]), lP0))
    return a, cond


def extra_rows(gname, N):
    """the inverse's own classes for one group: dicts with cls, R, gamma, cin, cout, o (+ w | alpha, beta)"""
    fam = P.family(gname)
    rows = []
    if gname in ("product", "solidly", "geomean", "weighted3", "curve3"):
        for k in (1, 8, 20, 30, 40):   # o = R_o·(1 − 2^-k): the pool all but drained
            R = lognormal(N, 1.0)
            ci = int(rng.integers(N)); co = int((ci + 1 + rng.integers(N - 1)) % N)
            r = dict(cls="near_drain", R=R, gamma=0.997, cin=ci, cout=co, o=float(R[co] * (1.0 - 2.0 ** -k)))
            if fam in ("geomean", "weighted"):
                w = rng.dirichlet(np.ones(N) * 2.0)
                r["w"] = w / w.sum()
            if fam == "curve":
                r["alpha"] = float(np.exp(rng.uniform(np.log(0.1), np.log(10.0))))
                r["beta"] = float(r["alpha"] * np.exp(np.mean(np.log(R))) * np.prod(R))
            rows.append(r)
    if fam == "curve":
        for k in range(5):   # E′ < 0: o > R_i + P₀/α needs a deep out side and a stiff pool (P₀/α = 1e-6 of the reserves)
            x = float(lognormal(1)[0])
            R = x * np.exp(rng.normal(0.0, 0.05, N))
            ci = int(rng.integers(N)); co = int((ci + 1 + rng.integers(N - 1)) % N)
            R[co] = 100.0 * R[ci]
            alpha = float(np.exp(rng.uniform(np.log(0.1), np.log(10.0))))
            beta = float(1e-6 * alpha * R[ci] * np.prod(R))
            rows.append(dict(cls="o_gt_Ri", R=R, gamma=0.9996, cin=ci, cout=co, o=float((1.5, 3.0, 10.0, 50.0, 99.0)[k] * R[ci]),
                             alpha=alpha, beta=beta))
    return rows


def make_reserve_group(out, src, gname, classes):
    g = F.group(src, gname)
    fam, N = P.family(gname), g["R"].shape[1]
    rows = []
    for j in range(g["a"].size):
        r = dict(cls=str(g["cls"][j]), R=g["R"][j], gamma=g["gamma"][j], cin=g["cin"][j], cout=g["cout"][j], o=g["out"][j])
        for c in ("w", "alpha", "beta"):
            if c in g:
                r[c] = g[c][j]
        rows.append(r)
    rows += extra_rows(gname, N)
    for r in rows:
        r["a"], r["cond"] = solve_row(fam, r)
        if fam == "curve" and r["cls"] == "o_gt_Ri":   # the class is what its name says
            P0 = float(r["beta"]) / float(np.prod(r["R"]))
            assert float(r["alpha"]) * (float(r["R"][r["cin"]]) - r["o"]) + P0 < 0
    m = len(rows)
    f = lambda key: np.array([float(r[key]) for r in rows])
    out[f"{gname}_R"] = np.array([r["R"] for r in rows], dtype=np.float64).reshape(m, N)
    out[f"{gname}_gamma"], out[f"{gname}_o"], out[f"{gname}_a"], out[f"{gname}_cond"] = f("gamma"), f("o"), f("a"), f("cond")
    out[f"{gname}_cin"] = np.array([r["cin"] for r in rows], dtype=np.int32)
    out[f"{gname}_cout"] = np.array([r["cout"] for r in rows], dtype=np.int32)
    out[f"{gname}_scale"] = np.array([float(r["R"][r["cin"]]) / float(r["gamma"]) for r in rows])
    out[f"{gname}_cls"] = np.array([classes.index(r["cls"]) for r in rows], dtype=np.int32)
    if "w" in g:
        out[f"{gname}_w"] = np.array([r["w"] for r in rows]).reshape(m, N)
    for c in ("alpha", "beta"):
        if c in g:
            out[f"{gname}_{c}"] = f(c)


# ---- UniV3 ----------------------------------------------------------------------------------------------------------
def mp_direction(cp, lt, lq, cin):
    """the non-empty ticks of the direction in walk order, the current one first: (k, s_in, s_out, β_out, R_out, δmax)"""
    from make_quote_golden import mp_ticks
    t, ct = mp_ticks(cp, lt, lq)
    nt = len(lt)
    recs = []
    for idx in (range(ct, nt + 1) if cin == 0 else range(ct, 0, -1)):
        k, al, be, R1, R2 = t[idx]
        if cin == 1:
            al, be, R1, R2 = be, al, R2, R1      # flip_sides
        if k == 0:
            continue
        s_in = R1 + al
        recs.append((k, s_in, R2 + be, be, R2, k / be - s_in if be > 0 else mp.inf))
    return recs


def mp_inverse_walk(cp, lt, lq, g, cin, o, closing=False):
    """trade_through_pools (src/cfmms.jl:416-434) inverted -> (a, scale, cond).  closing: o IS the direction's total as the
    device holds it -- the answer is Σδmax/γ by definition, whatever side of the exact total the double o fell on."""
    recs = mp_direction(cp, lt, lq, cin)
    g, o = M(g), M(float(o))
    sd, sr, roots, routs = M(0), M(0), M(0), M(0)   # Σδmax, ΣR_out, Σ(k/β + s_in), Σ(s_out + β) over the drained ticks
    for j, (k, s_in, s_out, be, rout, dmax) in enumerate(recs):
        last = j == len(recs) - 1
        if not closing and (o - sr < rout):
            ot = o - sr
            d = k / (s_out - ot) - s_in
            slope = k / (s_out - ot) ** 2 / g                # ∂a/∂o
            cond = (sd + d) / g + roots / g + routs * slope + d / g + s_out * slope + o * slope
            return (sd + d) / g, (roots + s_in) / g, cond
        if dmax == mp.inf:
            return mp.inf, M(0), M(0)
        sd, sr = sd + dmax, sr + rout
        roots, routs = roots + k / be + s_in, routs + s_out + be
        if last:
            if closing:
                slope = (s_in + dmax) ** 2 / k / g           # the last tick's slope at its end
                return sd / g, roots / g, sd / g + roots / g + (routs + o) * slope
            return mp.inf, M(0), M(0)
    return (M(0), M(0), M(0)) if closing else (mp.inf, M(0), M(0))


def make_univ3(out, src, classes):
    g = F.group(src, "univ3")
    npool = g["current_price"].size
    pools = [F.univ3_pool(g, p) for p in range(npool)]
    preps = [F.univ3_prepare(*pl[:3]) for pl in pools]
    rows = []   # (cls, pool, cin, o, closing)
    for j in range(g["a"].size):
        c, p, ci = str(g["cls"][j]), int(g["pool"][j]), int(g["cin"][j])
        if c == "exhausted":   # at the discontinuity: the device's own total, bit for bit (module docstring of the ref)
            rows.append((c, p, ci, P.univ3_totals(preps[p], ci)[1], True))
        else:
            rows.append((c, p, ci, float(g["out"][j]), False))
    for p in range(npool):
        for ci in (0, 1):
            lst = preps[p][1] if ci == 0 else preps[p][2]
            sd, sr = P.univ3_totals(preps[p], ci)
            finite = np.isfinite(sd)
            for e in sorted({0, 1, len(lst) // 2, len(lst) - 2} & set(range(len(lst) - 1))):
                if lst[e][6] > 0 and np.isfinite(lst[e][5]):
                    rows.append(("on_boundary", p, ci, lst[e][6], False))
            if sr > 0:
                rows.append(("closing_exact" if finite else "asymptotic", p, ci, sr, finite))
    for p, ci, mult in ((0, 0, 1.0000001), (0, 1, 3.0), (1, 1, 1.0000001), (4, 0, 1.5)):
        rows.append(("beyond", p, ci, float(np.nextafter(P.univ3_totals(preps[p], ci)[1], np.inf) * mult), False))
    res = []
    for c, p, ci, o, closing in rows:
        cp, lt, lq, gm = pools[p]
        a, scale, cond = mp_inverse_walk(cp, lt, lq, gm, ci, o, closing)
        if c == "asymptotic":
            a = mp.inf
        if c in ("beyond", "asymptotic"):
            assert a == mp.inf, (c, p, ci)
        res.append((c, p, ci, o, float(a), float(scale), float(cond)))
    for k in ("current_price", "pool_gamma", "tick_off", "lower_ticks", "liquidity"):
        out[f"univ3_{k}"] = g[k]
    out["univ3_pool"] = np.array([r[1] for r in res], dtype=np.int64)
    out["univ3_cin"] = np.array([r[2] for r in res], dtype=np.int32)
    for k, col in (("o", 3), ("a", 4), ("scale", 5), ("cond", 6)):
        out[f"univ3_{k}"] = np.array([r[col] for r in res])
    out["univ3_cls"] = np.array([classes.index(r[0]) for r in res], dtype=np.int32)


def main():
    src = F.load()
    classes = [str(s) for s in src["classes"]] + NEW
    out = {"classes": np.array(classes)}
    for gname in P.GROUPS:
        if gname == "univ3":
            make_univ3(out, src, classes)
        else:
            make_reserve_group(out, src, gname, classes)
        a = out[f"{gname}_a"]
        print(gname, a.size, "rows,", int(np.sum(np.isinf(a))), "+inf", flush=True)
    np.savez_compressed(P.FIXTURE, **out)
    n = sum(out[f"{g}_a"].size for g in P.GROUPS)
    ninf = sum(int(np.sum(np.isinf(out[f"{g}_a"]))) for g in P.GROUPS)
    print(P.FIXTURE, os.path.getsize(P.FIXTURE), "bytes;", n, "rows,", ninf, "of them +inf")
    assert ninf <= P.MAX_INF_SHARE * n


if __name__ == "__main__":
    main()
