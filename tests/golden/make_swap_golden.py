"""Writes tests/golden/swap_precise.npz: SEQUENCES of 1-4 exact-input swaps on one pool, carried with EXACT state between the
steps, with an 80-digit truth per step (stored as the nearest double): the amount out, the state the step leaves (the two
reserves that moved, or the UniV3 price) and the pieces of the bound of tests/swap_precise_ref.py.

The truth does not use the project's arithmetic.  Reserve kinds: the root `out` of φ(R + γa·e_in − out·e_out) = φ(R) by
bisection on φ itself, as tests/golden/make_quote_golden.py finds it (its φ's, root finder and closed forms are imported
from there; the closed forms serve the cross-check and the derivatives only), then R_in + γa and R_out − out in mpmath, never
rounded between steps.  UniV3: the reference's tick-by-tick walk (src/cfmms.jl:401-434) in mpmath from the ladder, the pool
resting where the walk ends -- P = k/s'² or s'²/k in the landing tick, the far edge of the last non-empty tick when the
direction is exhausted, capped at the first tick's upper price -- and that price carried as an mpmath number.
usage: python tests/golden/make_swap_golden.py        (needs mpmath; deterministic: seeded)"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_quote_golden as G  # noqa: E402

mp.mp.dps = 80
M = mp.mpf
MAX_STEPS = 4
rng = np.random.default_rng(20241019)


# ---- reserve kinds ------------------------------------------------------------------------------------------------------
def closed_form(fam, R, w, alpha, beta, g, ci, co, a):
    """the family's closed form as a function of the whole reserve vector (mpmath)"""
    def f(Rv):
        if fam in ("product", "geomean", "weighted"):
            return G.cf_weighted(Rv[ci], Rv[co], w[ci], w[co], g, a)
        if fam == "solidly":
            return G.cf_solidly(Rv[ci], Rv[co], g, a)
        lP0 = mp.log(beta) - sum(mp.log(x) for x in Rv)
        return G.cf_curve(Rv[ci], Rv[co], alpha, lP0, g, a)
    return f


def phi_of(fam, w, alpha, beta):
    if fam in ("product", "geomean", "weighted"):
        return lambda R: G.phi_weighted(R, w)
    if fam == "solidly":
        return G.phi_solidly
    return lambda R: G.phi_curve(R, alpha, beta)


def cond_of(fam, R, w, alpha, beta, g, ci, co, a):
    """quote_precise_ref's conditioning sum at this (exact) state"""
    if fam in ("product", "solidly"):
        cf = (lambda ri, ro, gg, aa: G.cf_weighted(ri, ro, M(1), M(1), gg, aa)) if fam == "product" else G.cf_solidly
        return G.cond_sum(cf, [R[ci], R[co], g, a])
    if fam in ("geomean", "weighted"):
        return G.cond_sum(G.cf_weighted, [R[ci], R[co], w[ci], w[co], g, a])
    lb = mp.log(beta)
    lP0 = lb - sum(mp.log(x) for x in R)
    c = G.cond_sum(lambda ri, ro, al, gg, aa: G.cf_curve(ri, ro, al, lP0, gg, aa), [R[ci], R[co], alpha, g, a])
    dl = mp.diff(lambda t: G.cf_curve(R[ci], R[co], alpha, t, g, a), lP0)
    return c + (abs(lb) + sum(abs(mp.log(x)) for x in R)) * abs(dl)


def reserve_sequence(fam, R0, w, alpha, beta, g, steps):
    """steps: [(cin, cout, a)] -> per step dict(out, Rin, Rout, scale, cond, dq [N]) with exact state carried"""
    R = [M(float(x)) for x in R0]
    w = None if w is None else [M(float(x)) for x in w]
    if fam == "weighted":
        ws = sum(w)
        w = [x / ws for x in w]
    if fam == "product":
        w = [M(1)] * len(R)
    alpha, beta, g = M(float(alpha)), M(float(beta)), M(float(g))
    phi = phi_of(fam, w, alpha, beta)
    rows = []
    for ci, co, a in steps:
        a = M(float(a))
        k0 = phi(R)

        def f(o):
            Rn = list(R)
            Rn[ci] = R[ci] + g * a
            Rn[co] = R[co] - o
            return phi(Rn) - k0
        o = G.root(f, R[co])
        cf = closed_form(fam, R, w, alpha, beta, g, ci, co, a)
        G.check(o, cf(R), (fam, ci, co))
        dq = [abs(mp.diff(lambda t, k=k: cf([t if j == k else R[j] for j in range(len(R))]), R[k])) if (k in (ci, co) or fam == "curve") else M(0)
              for k in range(len(R))]
        row = dict(out=o, scale=R[co], cond=cond_of(fam, R, w, alpha, beta, g, ci, co, a), dq=dq)
        R[ci] = R[ci] + g * a
        R[co] = R[co] - o
        row.update(Rin=R[ci], Rout=R[co])
        rows.append(row)
    return rows


def lognormal(n, sigma=2.0):
    return np.exp(rng.normal(0.0, sigma, n)) * 1e3


def reserve_cases(N):
    """(cls, R0, gamma, steps): `balanced` reserves within a few percent of each other, `typical` lognormal ones, `lopsided`
    twelve and more orders of magnitude apart, `low_gamma` a fee of 10-50%; 1-4 steps each, directions mixed, a pool coin
    revisited, amounts from 1e-3 to 0.5 of the tendered reserve"""
    out = []

    def steps_for(R, n):
        s = []
        Rc = np.array(R, dtype=float)
        for j in range(n):
            ci = int(rng.integers(N))
            co = int((ci + 1 + rng.integers(N - 1)) % N)
            a = float(np.exp(rng.uniform(np.log(1e-3), np.log(0.5)))) * Rc[ci]
            s.append((ci, co, a))
            Rc[ci] += a                         # (only to keep the later amounts in proportion)
        return s
    for n in (1, 2, 3, 4, 4):
        R = 1e4 * (1.0 + 0.05 * rng.uniform(-1, 1, N))
        out.append(("balanced", R, float(rng.choice([0.997, 0.9995, 1.0])), steps_for(R, n)))
    for n in (1, 2, 3, 4, 4):
        R = lognormal(N)
        out.append(("typical", R, float(rng.choice([0.997, 0.9995, 1.0])), steps_for(R, n)))
    for k, n in enumerate((2, 3, 4)):
        R = lognormal(N, 0.5)
        R[0], R[1] = (1e12, 1e-6) if k % 2 == 0 else (1e-6, 1e12)
        out.append(("lopsided", R, 0.997, steps_for(R, n)))
    for k, n in enumerate((2, 4)):
        R = lognormal(N)
        out.append(("low_gamma", R, 0.5 if k else 0.9, steps_for(R, n)))
    return out


def pack_reserve(out, name, fam, N):
    cases = reserve_cases(N)
    S = len(cases)
    z = lambda *shape: np.zeros(shape)
    cols = dict(R0=z(S, N), gamma=z(S), w=z(S, N), alpha=z(S), beta=z(S), nsteps=np.zeros(S, dtype=np.int64),
                cin=np.zeros((S, MAX_STEPS), dtype=np.int32), cout=np.zeros((S, MAX_STEPS), dtype=np.int32), a=z(S, MAX_STEPS),
                out=z(S, MAX_STEPS), Rin=z(S, MAX_STEPS), Rout=z(S, MAX_STEPS), scale=z(S, MAX_STEPS), cond=z(S, MAX_STEPS),
                dq=z(S, MAX_STEPS, N))
    cls = []
    for s, (c, R0, g, steps) in enumerate(cases):
        w = rng.dirichlet(np.ones(N)) if fam in ("geomean", "weighted") else np.ones(N)
        if fam == "curve":          # pegged pools: reserves near each other, α from stiff to soft, β from the invariant's scale
            if c in ("balanced", "typical", "low_gamma"):
                R0 = float(np.mean(R0)) * (1.0 + 0.3 * rng.uniform(-1, 1, N))
            else:
                R0 = 1e4 * np.exp(rng.uniform(-3, 3, N))
            steps = [(ci, co, min(a, 0.5 * R0[ci])) for ci, co, a in steps]
            alpha = float(np.exp(rng.uniform(np.log(0.1), np.log(100.0))))
            beta = float(np.prod(R0) * np.mean(R0) * np.exp(rng.uniform(-1, 1)))
        else:
            alpha, beta = 0.0, 1.0
        rows = reserve_sequence(fam, R0, w, alpha, beta, g, steps)
        cls.append(c)
        cols["R0"][s], cols["gamma"][s], cols["w"][s], cols["alpha"][s], cols["beta"][s] = R0, g, w, alpha, beta
        cols["nsteps"][s] = len(steps)
        for j, ((ci, co, a), r) in enumerate(zip(steps, rows)):
            cols["cin"][s, j], cols["cout"][s, j], cols["a"][s, j] = ci, co, a
            for f in ("out", "Rin", "Rout", "scale", "cond"):
                cols[f][s, j] = float(r[f])
            cols["dq"][s, j] = [float(x) for x in r["dq"]]
    for f, v in cols.items():
        out[f"{name}_{f}"] = v
    out[f"{name}_cls"] = np.array(cls)


# ---- UniV3 ----------------------------------------------------------------------------------------------------------------
def mp_ticks(cp, lt, lq):
    """compute_at_tick (src/cfmms.jl:294-313) for every tick in mpmath at the (mpmath) price cp"""
    nt = len(lt)
    ct = max(j + 1 for j in range(nt) if M(float(lt[j])) >= cp)
    t = [None]
    for idx in range(1, nt + 1):
        k, pp = M(float(lq[idx - 1])), M(float(lt[idx - 1]))
        pm = M(float(lt[idx])) if idx < nt else M(0)
        al, be = mp.sqrt(k / pp), mp.sqrt(k * pm)
        p = pp if idx > ct else (pm if idx < ct else cp)
        t.append((k, al, be, mp.sqrt(k / p) - al, mp.sqrt(k * p) - be) if k != 0 else (k, M(0), M(0), M(0), M(0)))
    return t, ct


def mp_swap(cp, lt, lq, g, cin, a):
    """trade_through_pools (src/cfmms.jl:416-434) in mpmath, and where the pool rests -> (out, scale, cond, new price)"""
    t, ct = mp_ticks(cp, lt, lq)
    nt = len(lt)
    order = range(ct, nt + 1) if cin == 0 else range(ct, 0, -1)
    d = M(float(g)) * M(float(a))
    lam, scale, cond, drained = M(0), M(0), M(0), M(0)
    price = lambda k, s: k / (s * s) if cin == 0 else (s * s) / k
    rest = cp
    if a == 0:
        return lam, scale, cond, cp
    for idx in order:
        k, al, be, R1, R2 = t[idx]
        if cin == 1:
            al, be, R1, R2 = be, al, R2, R1      # flip_sides
        if k == 0:
            continue
        s_in, s_out = R1 + al, R2 + be
        mx = k / be - s_in if be > 0 else mp.inf
        if mx > d:
            l = min(R2, s_out - k / (s_in + d))
            lam += l
            scale += R2
            cond += s_out + k / (s_in + d) + (s_in + 2 * M(float(g)) * M(float(a)) + drained) * k / (s_in + d) ** 2
            return lam, scale, cond, price(k, s_in + d)
        lam += R2
        scale += R2
        cond += s_out + be
        drained += k / be + s_in
        d -= mx
        rest = price(k, s_in + mx)               # the far edge of the last tick drained so far
    return lam, scale, cond, min(rest, M(float(lt[0])))


def univ3_cases():
    """(cls, cp, lt, lq, gamma, steps [(cin, a)]).  Ladders of 1, 2 and 5 ticks.  The `exact` ladders have upper prices 4, 1,
    1/4 (, 1/16, 1/64) and liquidity 144: every root of a tick edge is exact, and from the price 2.25 = 1.5² the roots of the
    current price are too (√(144/2.25) = 8, √(144·2.25) = 18), so with γ = 1 a swap of 4 of coin 0 ends EXACTLY on the edge
    between the first two ticks."""
    L5 = np.array([4.0, 1.0, 0.25, 0.0625, 0.015625])
    k5 = np.full(5, 144.0)
    hole = np.array([144.0, 0.0, 144.0, 100.0, 81.0])
    r5 = np.array([3.1, 1.7, 0.9, 0.41, 0.13])
    q5 = np.array([52.0, 870.0, 13.0, 240.0, 95.0])
    return [
        ("one_tick", 1.3, np.array([2.0]), np.array([50.0]), 0.997, [(0, 2.0), (1, 1.0), (0, 30.0)]),
        ("one_tick", 0.7, np.array([5.0]), np.array([1e6]), 1.0, [(1, 10.0), (1, 10.0)]),
        ("two_ticks", 1.5, np.array([3.0, 1.0]), np.array([40.0, 90.0]), 0.997, [(0, 1.0), (0, 4.0), (1, 2.0), (1, 3.0)]),
        ("tick_edge", 2.25, L5[:2], k5[:2], 1.0, [(0, 4.0), (0, 1.0), (1, 0.5)]),
        ("tick_edge", 2.25, L5, k5, 1.0, [(0, 4.0), (1, 6.0), (0, 16.0)]),
        ("crosses", 2.25, L5, k5, 0.997, [(0, 40.0), (1, 100.0), (0, 3.0), (0, 90.0)]),
        ("crosses", 2.9, r5, q5, 0.9995, [(0, 35.0), (0, 20.0), (1, 40.0)]),
        ("empty_tick", 2.25, L5, hole, 0.997, [(0, 20.0), (1, 30.0), (0, 60.0)]),
        ("empty_tick", 0.5, L5, hole, 1.0, [(1, 5.0), (0, 1.0)]),
        ("exhausted", 0.1, L5, k5, 0.997, [(1, 1e6), (1, 1.0), (0, 2.0)]),
        ("exhausted", 0.3, r5, q5, 1.0, [(1, 1e9), (0, 5.0), (1, 1e9)]),
        ("reversal", 1.1, r5, q5, 0.997, [(0, 8.0), (1, 8.0), (0, 8.0), (1, 8.0)]),
    ]


def pack_univ3(out):
    cases = univ3_cases()
    S = len(cases)
    cols = dict(cp=np.zeros(S), gamma=np.zeros(S), nsteps=np.zeros(S, dtype=np.int64), cin=np.zeros((S, MAX_STEPS), dtype=np.int32),
                a=np.zeros((S, MAX_STEPS)), out=np.zeros((S, MAX_STEPS)), price=np.zeros((S, MAX_STEPS)),
                scale=np.zeros((S, MAX_STEPS)), cond=np.zeros((S, MAX_STEPS)))
    off, lts, lqs, cls = [0], [], [], []
    for s, (c, cp, lt, lq, g, steps) in enumerate(cases):
        cls.append(c)
        cols["cp"][s], cols["gamma"][s], cols["nsteps"][s] = cp, g, len(steps)
        lts.append(lt)
        lqs.append(lq)
        off.append(off[-1] + len(lt))
        P = M(float(cp))
        for j, (ci, a) in enumerate(steps):
            o, sc, cd, P = mp_swap(P, lt, lq, g, ci, a)
            cols["cin"][s, j], cols["a"][s, j] = ci, a
            cols["out"][s, j], cols["price"][s, j], cols["scale"][s, j], cols["cond"][s, j] = float(o), float(P), float(sc), float(cd)
    for f, v in cols.items():
        out[f"univ3_{f}"] = v
    out["univ3_cls"] = np.array(cls)
    out["univ3_tick_off"] = np.array(off, dtype=np.int64)
    out["univ3_lower_ticks"] = np.concatenate(lts)
    out["univ3_liquidity"] = np.concatenate(lqs)


def main():
    out = {}
    for name, fam, N in (("product", "product", 2), ("geomean", "geomean", 2), ("solidly", "solidly", 2), ("weighted3", "weighted", 3),
                         ("weighted8", "weighted", 8), ("curve3", "curve", 3), ("curve8", "curve", 8)):
        pack_reserve(out, name, fam, N)
        print(name, "done")
    pack_univ3(out)
    path = os.path.join(HERE, "swap_precise.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
