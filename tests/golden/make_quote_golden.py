"""Writes tests/golden/quote_precise.npz: exact-input swap quotes of every pool kind with an 80-digit truth (stored as the
nearest double) and the conditioning sum of tests/quote_precise_ref.py per row.

The truth is independent of the project's arithmetic: the root `out` in (0, R_o) of φ(R + γa·e_in − out·e_out) = φ(R),
found by mpmath's bracketing root finder on φ ITSELF (weighted pools: on log φ = Σ w_k log R_k), and for UniV3 the
reference's tick-by-tick walk (src/cfmms.jl:401-434) evaluated in mpmath from the ladder.  The closed forms appear here
only for two things: a cross-check of every root (they must agree to 1e-40), and the conditioning sum (mp.diff).
usage: python tests/golden/make_quote_golden.py        (needs mpmath; deterministic: seeded)"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quote_precise_ref as P  # noqa: E402

mp.mp.dps = 80
M = mp.mpf
CLASSES = ["tiny", "typical", "huge", "lopsided", "low_gamma", "balanced", "t0_hi", "t0_lo", "stiff", "small_a", "alpha0",
           "pairs", "w02_98", "in_tick", "boundary_dn", "boundary_up", "depth1", "depth4", "depth5", "depth64", "empty_in_path",
           "empty_current", "last_tick", "exhausted"]
rng = np.random.default_rng(20240611)


def root(f, hi):
    """the root of f in (0, hi), f(0) > 0 > f(hi⁻): bisection until the bracket is 1e-72 of the root"""
    lo, hi = M(0), M(hi)
    for _ in range(400):
        mid = (lo + hi) / 2
        if f(mid) > 0:
            lo = mid
        else:
            hi = mid
        if hi - lo <= hi * M(10) ** -72:
            break
    return (lo + hi) / 2


# ---- φ per family (exact inputs: the doubles of the row) ------------------------------------------------------------
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


def truth(phi, R, g, cin, cout, a):
    R = [M(float(x)) for x in R]
    k0 = phi(R)

    def f(o):
        Rn = list(R)
        Rn[cin] = R[cin] + M(g) * M(a)
        Rn[cout] = R[cout] - o
        return phi(Rn) - k0            # φ is increasing in every reserve: positive below the root
    return root(f, R[cout])


# ---- closed forms in mpmath: cross-check + conditioning -------------------------------------------------------------
def cf_weighted(Ri, Ro, wi, wo, g, a):
    return Ro * (1 - (Ri / (Ri + g * a)) ** (wi / wo))


def cf_solidly(Ri, Ro, g, a):
    xp = Ri + g * a
    c = (Ro / Ri) * (1 + (Ro / Ri) ** 2) * (Ri / xp) ** 4
    s = mp.cbrt(c / 2 + mp.sqrt(c * c / 4 + M(1) / 27))
    return Ro - (s - 1 / (3 * s)) * xp


def cf_curve(Ri, Ro, alpha, lP0, g, a):
    x = g * a
    xp = Ri + x
    P0 = mp.e ** lP0
    C = alpha * (Ro - x) - P0
    B = P0 * Ro * Ri / xp
    E = alpha * (Ro + x) + P0
    G = Ro * x * (alpha + P0 / xp)
    return 2 * G / (E + mp.sqrt(C * C + 4 * alpha * B))


def cond_sum(f, xs):
    """Σ_j |x_j ∂f/∂x_j| over the arguments xs (mp.diff)"""
    s = M(0)
    for j, xj in enumerate(xs):
        if xj == 0:
            continue
        d = mp.diff(lambda t: f(*[t if k == j else xs[k] for k in range(len(xs))]), xj)
        s += abs(xj * d)
    return s


def check(o, cf, what):
    assert abs(o - cf) <= M(10) ** -40 * max(abs(o), M(10) ** -300), (what, o, cf)


# ---- rows -----------------------------------------------------------------------------------------------------------
def lognormal(n, sigma=2.0):
    return np.exp(rng.normal(0.0, sigma, n)) * 1e3


def generic_rows(n_coins, per=4):
    """(cls, R, gamma, cin, cout, a) over the five classes every family shares"""
    rows = []

    def pair():
        ci = int(rng.integers(n_coins))
        co = int((ci + 1 + rng.integers(n_coins - 1)) % n_coins)
        return ci, co
    for _ in range(per):
        R = lognormal(n_coins); ci, co = pair()
        rows.append(("tiny", R, 0.997, ci, co, 1e-12 * R[ci]))
    for _ in range(3 * per):
        R = lognormal(n_coins); ci, co = pair()
        rows.append(("typical", R, float(rng.choice([0.997, 0.9995, 1.0])), ci, co, float(np.exp(rng.uniform(np.log(1e-3), np.log(0.5)))) * R[ci]))
    for _ in range(per):
        R = lognormal(n_coins); ci, co = pair()
        rows.append(("huge", R, 0.997, ci, co, 1e6 * R[ci]))
    for k in range(per):
        R = lognormal(n_coins, 0.5); ci, co = pair()
        R[ci], R[co] = (1e12, 1e-6) if k % 2 == 0 else (1e-6, 1e12)
        rows.append(("lopsided", R, 0.997, ci, co, float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0)))) * R[ci]))
    for k in range(per):
        R = lognormal(n_coins); ci, co = pair()
        rows.append(("low_gamma", R, 0.5 if k % 2 else 0.9, ci, co, float(rng.uniform(0.01, 0.5)) * R[ci]))
    return rows


def pack(out, name, rows, N, extra_cols):
    """rows: dicts with cls, R, gamma, cin, cout, a, out, cond (+ extra columns)"""
    m = len(rows)
    out[f"{name}_R"] = np.array([r["R"] for r in rows], dtype=np.float64).reshape(m, N)
    out[f"{name}_gamma"] = np.array([r["gamma"] for r in rows])
    out[f"{name}_cin"] = np.array([r["cin"] for r in rows], dtype=np.int32)
    out[f"{name}_cout"] = np.array([r["cout"] for r in rows], dtype=np.int32)
    out[f"{name}_a"] = np.array([r["a"] for r in rows])
    out[f"{name}_out"] = np.array([float(r["out"]) for r in rows])
    out[f"{name}_cond"] = np.array([float(r["cond"]) for r in rows])
    out[f"{name}_scale"] = np.array([float(r["R"][r["cout"]]) for r in rows])
    out[f"{name}_cls"] = np.array([CLASSES.index(r["cls"]) for r in rows], dtype=np.int32)
    for c in extra_cols:
        out[f"{name}_{c}"] = np.array([r[c] for r in rows], dtype=np.float64)


def make_weighted(out, name, N, weights_of):
    rows = []
    specs = generic_rows(N)
    if N == 3:   # every (in, out) pair
        for ci in range(3):
            for co in range(3):
                if ci != co:
                    R = lognormal(3)
                    specs.append(("pairs", R, 0.997, ci, co, 0.1 * R[ci]))
    for k in range(4):   # weights 0.02 / 0.98, both ways
        R = lognormal(N)
        specs.append(("w02_98", R, 0.997, k % 2, 1 - k % 2, (0.05 if k < 2 else 5.0) * R[k % 2]))
    for cls, R, g, ci, co, a in specs:
        w = weights_of(N)
        if cls == "w02_98":   # coins 0 and 1 at 0.02 : 0.98 (of the half the other coins leave them when N > 2)
            share = 1.0 if N == 2 else 0.5
            w = np.full(N, (1.0 - share) / max(N - 2, 1))
            w[0], w[1] = 0.02 * share, 0.98 * share
        Rm, wm = [M(float(x)) for x in R], [M(float(x)) for x in w]
        o = truth(lambda RR: phi_weighted(RR, wm), R, g, ci, co, a)
        xs = [Rm[ci], Rm[co], wm[ci], wm[co], M(g), M(float(a))]
        check(o, cf_weighted(*xs), name)
        rows.append(dict(cls=cls, R=R, w=w, gamma=g, cin=ci, cout=co, a=float(a), out=o, cond=cond_sum(cf_weighted, xs)))
    pack(out, name, rows, N, ())
    out[f"{name}_w"] = np.array([r["w"] for r in rows]).reshape(len(rows), N)


def dirichlet(N):
    w = rng.dirichlet(np.ones(N) * 2.0)
    return w / w.sum()


def make_two_coin(out):
    rows = []
    for cls, R, g, ci, co, a in generic_rows(2):
        Rm = [M(float(x)) for x in R]
        o = truth(lambda RR: RR[0] * RR[1], R, g, ci, co, a)
        xs = [Rm[ci], Rm[co], M(g), M(float(a))]
        cf = lambda Ri, Ro, gg, aa: Ro * gg * aa / (Ri + gg * aa)
        check(o, cf(*xs), "product")
        rows.append(dict(cls=cls, R=R, gamma=g, cin=ci, cout=co, a=float(a), out=o, cond=cond_sum(cf, xs)))
    pack(out, "product", rows, 2, ())

    rows = []
    specs = generic_rows(2)
    for k in range(6):
        x = float(lognormal(1)[0])
        specs.append(("balanced", np.array([x, x]), 0.9995, k % 2, 1 - k % 2, float(np.exp(rng.uniform(np.log(1e-6), np.log(10.0)))) * x))
    for cls, t0 in (("t0_hi", np.exp(3.0)), ("t0_lo", np.exp(-3.0))):
        for k in range(6):
            x = float(lognormal(1)[0])
            R = np.array([x, x * t0])          # coin 0 in: t₀ = R_o/R_i
            specs.append((cls, R, 0.9995, 0, 1, float(np.exp(rng.uniform(np.log(1e-6), np.log(100.0)))) * x))
    for cls, R, g, ci, co, a in specs:
        Rm = [M(float(x)) for x in R]
        o = truth(phi_solidly, R, g, ci, co, a)
        xs = [Rm[ci], Rm[co], M(g), M(float(a))]
        check(o, cf_solidly(*xs), "solidly")
        rows.append(dict(cls=cls, R=R, gamma=g, cin=ci, cout=co, a=float(a), out=o, cond=cond_sum(cf_solidly, xs)))
    pack(out, "solidly", rows, 2, ())

    make_weighted(out, "geomean", 2, dirichlet)


def make_curve(out, name, N):
    rows = []
    specs = [(cls, R, g, ci, co, a, 1.0) for cls, R, g, ci, co, a in generic_rows(N, per=3)]

    def near(n):       # a pegged pool: reserves within a few percent of each other
        return float(lognormal(1)[0]) * np.exp(rng.normal(0.0, 0.05, n))
    for cls, ratio in (("stiff", 1e-6), ("small_a", 1e6), ("alpha0", None)):
        for k in range(5):
            R = near(N)
            ci = int(rng.integers(N)); co = int((ci + 1 + rng.integers(N - 1)) % N)
            specs.append((cls, R, 0.9996, ci, co, float(np.exp(rng.uniform(np.log(1e-6), np.log(2.0)))) * R[ci], ratio))
    for cls, R, g, ci, co, a, ratio in specs:
        # P₀/R_ref = ratio·α  (ratio None: α = 0), R_ref the geometric mean reserve
        Rref = float(np.exp(np.mean(np.log(R))))
        alpha = 0.0 if ratio is None else float(np.exp(rng.uniform(np.log(0.1), np.log(10.0))))
        P0 = (1.0 if ratio is None else ratio * alpha) * Rref
        beta = float(P0 * np.prod(R))
        Rm = [M(float(x)) for x in R]
        al, be = M(alpha), M(beta)
        o = truth(lambda RR: phi_curve(RR, al, be), R, g, ci, co, a)
        pr = M(1)
        for x in Rm:
            pr *= x
        lP0 = mp.log(be / pr)
        xs = [Rm[ci], Rm[co], al, lP0, M(g), M(float(a))]
        check(o, cf_curve(*xs), name)
        # the logs the device holds: log β and every log R_k enter through log P₀ (argument 3)
        logs = abs(mp.log(be)) + sum(abs(mp.log(x)) for x in Rm)
        cond = M(0)
        for j in (0, 1, 2, 4, 5):
            if xs[j] != 0:
                cond += abs(xs[j] * mp.diff(lambda t, j=j: cf_curve(*[t if k == j else xs[k] for k in range(6)]), xs[j]))
        cond += logs * abs(mp.diff(lambda t: cf_curve(xs[0], xs[1], xs[2], t, xs[4], xs[5]), lP0))
        rows.append(dict(cls=cls, R=R, gamma=g, cin=ci, cout=co, a=float(a), out=o, cond=cond, alpha=alpha, beta=beta))
    pack(out, name, rows, N, ("alpha", "beta"))


# ---- UniV3 ----------------------------------------------------------------------------------------------------------
def mp_ticks(cp, lt, lq):
    """compute_at_tick (src/cfmms.jl:294-313) for every tick in mpmath: (k, α, β, R1, R2) 1-based, and the current tick"""
    nt = len(lt)
    ct = max(j + 1 for j in range(nt) if lt[j] >= cp)
    t = [None]
    for idx in range(1, nt + 1):
        k, pp = M(float(lq[idx - 1])), M(float(lt[idx - 1]))
        pm = M(float(lt[idx])) if idx < nt else M(0)
        al, be = mp.sqrt(k / pp), mp.sqrt(k * pm)
        p = pp if idx > ct else (pm if idx < ct else M(float(cp)))
        t.append((k, al, be, mp.sqrt(k / p) - al, mp.sqrt(k * p) - be) if k != 0 else (k, M(0), M(0), M(0), M(0)))
    return t, ct


def mp_walk(cp, lt, lq, g, cin, a):
    """trade_through_pools (src/cfmms.jl:416-434) in mpmath -> (out, scale, cond)"""
    t, ct = mp_ticks(cp, lt, lq)
    nt = len(lt)
    order = range(ct, nt + 1) if cin == 0 else range(ct, 0, -1)
    d = M(g) * M(float(a))
    lam, scale, cond, drained = M(0), M(0), M(0), M(0)
    for idx in order:
        k, al, be, R1, R2 = t[idx]
        if cin == 1:
            al, be, R1, R2 = be, al, R2, R1      # flip_sides
        if k == 0:
            continue                             # max_amount 0, R_2 0: nothing happens
        s_in, s_out = R1 + al, R2 + be
        mx = k / be - s_in if be > 0 else mp.inf
        if mx > d:
            l = s_out - k / (s_in + d)
            l = min(R2, l)
            lam += l
            scale += R2
            cond += s_out + k / (s_in + d) + (s_in + 2 * M(g) * M(float(a)) + drained) * k / (s_in + d) ** 2
            return lam, scale, cond
        lam += R2
        scale += R2
        cond += s_out + be
        drained += k / be + s_in
        d -= mx
    return lam, scale, cond


def mp_dmaxes(cp, lt, lq, cin):
    """δmax of the non-empty ticks of the direction in walk order, the current one first (inf: the zero-lower-price tick)"""
    t, ct = mp_ticks(cp, lt, lq)
    nt = len(lt)
    order = range(ct, nt + 1) if cin == 0 else range(ct, 0, -1)
    mxs = []
    for idx in order:
        k, al, be, R1, R2 = t[idx]
        if cin == 1:
            al, be, R1, R2 = be, al, R2, R1
        if k == 0:
            continue
        mxs.append(k / be - (R1 + al) if be > 0 else mp.inf)
    return mxs


def mp_sum_dmax(cp, lt, lq, cin, depth):
    """Σδmax of the first `depth` non-empty ticks of the direction, and the next one's δmax (None: there is none)"""
    mxs = mp_dmaxes(cp, lt, lq, cin)
    return sum(mxs[:depth], M(0)), (mxs[depth] if depth < len(mxs) else None)


def make_univ3(out):
    pools, queries = [], []

    def ladder(nt, cur, empty=()):
        """nt ticks with upper prices descending geometrically around 1; the price sits inside tick `cur` (1-based)"""
        step = float(np.exp(rng.uniform(0.01, 0.08)))
        top = step ** (cur - 0.5)
        lt = np.array([top / step ** j for j in range(nt)])
        lq = np.exp(rng.normal(np.log(1e6), 1.0, nt))
        for e in empty:
            lq[e - 1] = 0.0
        pm = lt[cur] if cur < nt else lt[cur - 1] / step
        cp = float(np.exp(rng.uniform(np.log(pm) + 0.1 * np.log(step), np.log(lt[cur - 1]) - 0.1 * np.log(step))))
        return cp, lt, lq

    def add(cls, pool, cin, a):
        queries.append((cls, pool, cin, float(a)))

    def at_depth(pool, cin, depth, frac=0.4):
        cp, lt, lq, g = pools[pool]
        s, nxt = mp_sum_dmax(cp, lt, lq, cin, depth)
        return float((s + frac * (nxt if nxt is not None and nxt != mp.inf else s)) / M(g))

    # a 70-tick pool with the price in tick 3 (coin 0 in walks up to 67 ticks, coin 1 in two)
    pools.append((*ladder(70, 3), 0.997))
    # an 8-tick pool, price in tick 5
    pools.append((*ladder(8, 5), 0.9995))
    # an empty tick in the path both ways (ticks 3 and 6 of 8, price in tick 4)
    pools.append((*ladder(8, 4, empty=(3, 6)), 0.997))
    # an empty CURRENT tick (tick 4 of 8)
    pools.append((*ladder(8, 4, empty=(4,)), 0.997))
    # a single tick (BoundedProduct): its lower price is 0
    pools.append((*ladder(1, 1), 0.997))
    for p in (0, 1, 2):
        for cin in (0, 1):
            s, _ = mp_sum_dmax(*pools[p][:3], cin, 1)
            for f in (1e-9, 1e-3, 0.5, 0.999):
                add("in_tick", p, cin, float(f * s / M(pools[p][3])))
    for p, cin, depth in ((0, 0, 1), (0, 0, 7), (1, 0, 2), (1, 1, 3), (2, 1, 1)):
        s, _ = mp_sum_dmax(*pools[p][:3], cin, depth)
        exact = s / M(pools[p][3])
        dn = float(exact)
        if M(dn) > exact:
            dn = float(np.nextafter(dn, 0.0))
        add("boundary_dn", p, cin, dn)
        add("boundary_up", p, cin, float(np.nextafter(dn, np.inf)))
    for cls, depth in (("depth1", 1), ("depth4", 4), ("depth5", 5), ("depth64", 64)):
        for frac in (0.1, 0.7):
            add(cls, 0, 0, at_depth(0, 0, depth, frac))
    add("depth1", 1, 1, at_depth(1, 1, 1))
    add("depth4", 1, 1, at_depth(1, 1, 4))
    for cin in (0, 1):
        add("empty_in_path", 2, cin, at_depth(2, cin, 1, 0.5))
        add("empty_in_path", 2, cin, at_depth(2, cin, 2, 0.5))
        add("empty_current", 3, cin, at_depth(3, cin, 0, 0.3))
        add("empty_current", 3, cin, at_depth(3, cin, 1, 0.3))
    # the zero-lower-price last tick absorbs any amount (coin 0 in)
    for p, mult in ((1, 10.0), (1, 1e6), (4, 0.5), (4, 1e9)):
        finite = [x for x in mp_dmaxes(*pools[p][:3], 0) if x != mp.inf]
        base = sum(finite, M(0)) if finite else mp.sqrt(M(float(pools[p][2][-1])))
        add("last_tick", p, 0, float(mult * base / M(pools[p][3])))
    # beyond all liquidity, price rising (coin 1 in)
    for p in (0, 1, 2, 4):
        s = sum(mp_dmaxes(*pools[p][:3], 1), M(0))
        for mult in (1.0000001, 3.0):
            add("exhausted", p, 1, float(mult * s / M(pools[p][3])))

    rows = []
    for cls, p, cin, a in queries:
        cp, lt, lq, g = pools[p]
        o, scale, cond = mp_walk(cp, lt, lq, g, cin, a)
        rows.append((cls, p, cin, a, float(o), float(scale), float(cond)))
    out["univ3_current_price"] = np.array([p[0] for p in pools])
    out["univ3_pool_gamma"] = np.array([p[3] for p in pools])
    out["univ3_tick_off"] = np.cumsum([0] + [len(p[1]) for p in pools]).astype(np.int64)
    out["univ3_lower_ticks"] = np.concatenate([p[1] for p in pools])
    out["univ3_liquidity"] = np.concatenate([p[2] for p in pools])
    out["univ3_pool"] = np.array([r[1] for r in rows], dtype=np.int64)
    out["univ3_cin"] = np.array([r[2] for r in rows], dtype=np.int32)
    out["univ3_a"] = np.array([r[3] for r in rows])
    out["univ3_out"] = np.array([r[4] for r in rows])
    out["univ3_scale"] = np.array([r[5] for r in rows])
    out["univ3_cond"] = np.array([r[6] for r in rows])
    out["univ3_cls"] = np.array([CLASSES.index(r[0]) for r in rows], dtype=np.int32)


def main():
    out = {"classes": np.array(CLASSES)}
    make_two_coin(out)
    for N in (2, 3, 8):
        make_weighted(out, f"weighted{N}", N, dirichlet)
    for N in (2, 3, 4):
        make_curve(out, f"curve{N}", N)
    make_univ3(out)
    np.savez_compressed(P.FIXTURE, **out)
    print(P.FIXTURE, os.path.getsize(P.FIXTURE), "bytes;", {g: int(out[f"{g}_a"].size) for g in P.GROUPS})


if __name__ == "__main__":
    main()
