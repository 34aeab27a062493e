"""Writes tests/golden/swap_out_precise.npz: SEQUENCES of 1-4 exact-OUTPUT swaps on one pool, carried with EXACT state between
the steps, with an 80-digit truth per step (stored as the nearest double): the amount to tender, the state the step leaves
(the two reserves that moved, or the UniV3 price) and the pieces of the bound of tests/swap_out_precise_ref.py.

The truth does not use the project's arithmetic.  Reserve kinds: the smallest `a` with φ(R + γa·e_in − want·e_out) = φ(R) by
bisection on φ itself -- tests/golden/make_quote_out_golden.py's φ's, root finder, cross-check and closed forms are imported
from there; the closed forms serve the bracket, the cross-check and the derivatives only -- then R_in + γa* and R_out − want in
mpmath, never rounded between steps.  UniV3: the reference's tick-by-tick walk (src/cfmms.jl:401-434) inverted in mpmath from
the ladder at the (mpmath) price, the pool resting where that walk ends -- P = k/s'² or s'²/k in the landing tick, the far
edge of the last non-empty tick when the direction is exhausted, capped at the first tick's upper price.
usage: python tests/golden/make_swap_out_golden.py        (needs mpmath; deterministic: seeded)"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_quote_out_golden as G  # noqa: E402
import make_swap_golden as GS  # noqa: E402  (mp_ticks at an mpmath price)
import quote_precise_ref as F  # noqa: E402

mp.mp.dps = 80
M = mp.mpf
MAX_STEPS = 4
rng = np.random.default_rng(20250301)


# ---- reserve kinds ------------------------------------------------------------------------------------------------------
def forms(fam, R, w, alpha, beta, g, ci, co, o):
    """(φ, the closed form as a function of the whole reserve vector, quote_out_precise_ref's conditioning sum) at state R"""
    if fam in ("product", "geomean", "weighted"):
        phi = lambda Rv: G.phi_weighted(Rv, w)
        cf = lambda Rv: G.cf_weighted(Rv[ci], Rv[co], w[ci], w[co], g, o)
        if fam == "product":
            cond = G.cond_sum(G.cf_product, [R[ci], R[co], g, o])
        else:
            cond = G.cond_sum(G.cf_weighted, [R[ci], R[co], w[ci], w[co], g, o])
        return phi, cf, cond
    if fam == "solidly":
        return G.phi_solidly, (lambda Rv: G.cf_solidly(Rv[ci], Rv[co], g, o)), G.cond_sum(G.cf_solidly, [R[ci], R[co], g, o])
    lb = mp.log(beta)
    lP0 = lambda Rv: lb - sum(mp.log(x) for x in Rv)
    cf = lambda Rv: G.cf_curve(Rv[ci], Rv[co], alpha, lP0(Rv), g, o)
    xs = [R[ci], R[co], alpha, lP0(R), g, o]
    cond = G.cond_sum(G.cf_curve, xs, (3,))
    cond += (abs(lb) + sum(abs(mp.log(x)) for x in R)) * abs(mp.diff(lambda t: G.cf_curve(xs[0], xs[1], xs[2], t, xs[4], xs[5]), xs[3]))
    return (lambda Rv: G.phi_curve(Rv, alpha, beta)), cf, cond


def reserve_sequence(fam, R0, w, alpha, beta, g, steps):
    """steps: [(cin, cout, want)] -> per step dict(a, Rin, Rout, scale, cond, da [N]) with exact state carried"""
    R = [M(float(x)) for x in R0]
    w = None if w is None else [M(float(x)) for x in w]
    if fam == "weighted":
        ws = sum(w)
        w = [x / ws for x in w]
    if fam == "product":
        w = [M(1)] * len(R)
    alpha, beta, g = M(float(alpha)), M(float(beta)), M(float(g))
    rows = []
    for ci, co, o in steps:
        o = M(float(o))
        assert 0 < o < R[co]
        phi, cf, cond = forms(fam, R, w, alpha, beta, g, ci, co, o)
        k0 = phi(R)

        def f(a):
            Rn = list(R)
            Rn[ci] = R[ci] + g * a
            Rn[co] = R[co] - o
            return phi(Rn) - k0                 # φ is increasing in every reserve: negative below the root
        guess = cf(R)
        a = G.root(f, 2 * guess)
        G.check(a, guess, (fam, ci, co))
        da = [abs(mp.diff(lambda t, k=k: cf([t if j == k else R[j] for j in range(len(R))]), R[k])) if (k in (ci, co) or fam == "curve") else M(0)
              for k in range(len(R))]
        row = dict(a=a, scale=R[ci] / g, cond=cond, da=da)
        R[ci] = R[ci] + g * a
        R[co] = R[co] - o
        row.update(Rin=R[ci], Rout=R[co])
        rows.append(row)
    return rows


def lognormal(n, sigma=2.0):
    return np.exp(rng.normal(0.0, sigma, n)) * 1e3


def reserve_cases(N):
    """(cls, R0, gamma, steps): make_swap_golden's four classes -- `balanced` reserves within a few percent of each other,
    `typical` lognormal ones, `lopsided` twelve and more orders of magnitude apart, `low_gamma` a fee of 10-50% -- with 1-4
    steps each, directions mixed, a pool coin revisited, the wanted amounts from 1e-3 to 0.5 of the reserve asked"""
    out = []

    def steps_for(R, n):
        s = []
        Rc = np.array(R, dtype=float)
        for j in range(n):
            ci = int(rng.integers(N))
            co = int((ci + 1 + rng.integers(N - 1)) % N)
            o = float(np.exp(rng.uniform(np.log(1e-3), np.log(0.5)))) * Rc[co]
            s.append((ci, co, o))
            Rc[co] -= o                         # (only to keep the later amounts within the reserve)
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
                cin=np.zeros((S, MAX_STEPS), dtype=np.int32), cout=np.zeros((S, MAX_STEPS), dtype=np.int32), want=z(S, MAX_STEPS),
                a=z(S, MAX_STEPS), Rin=z(S, MAX_STEPS), Rout=z(S, MAX_STEPS), scale=z(S, MAX_STEPS), cond=z(S, MAX_STEPS),
                da=z(S, MAX_STEPS, N))
    cls = []
    for s, (c, R0, g, steps) in enumerate(cases):
        w = rng.dirichlet(np.ones(N)) if fam in ("geomean", "weighted") else np.ones(N)
        if fam == "curve":          # pegged pools, as make_swap_golden: reserves near each other, α from stiff to soft
            if c in ("balanced", "typical", "low_gamma"):
                R0 = float(np.mean(R0)) * (1.0 + 0.3 * rng.uniform(-1, 1, N))
            else:
                R0 = 1e4 * np.exp(rng.uniform(-3, 3, N))
            Rc, st2 = np.array(R0, dtype=float), []
            for ci, co, o in steps:             # the same fractions of the reserves this pool holds
                o = min(o, 0.5 * Rc[co])
                st2.append((ci, co, o))
                Rc[co] -= o
            steps = st2
            alpha = float(np.exp(rng.uniform(np.log(0.1), np.log(100.0))))
            beta = float(np.prod(R0) * np.mean(R0) * np.exp(rng.uniform(-1, 1)))
        else:
            alpha, beta = 0.0, 1.0
        rows = reserve_sequence(fam, R0, w, alpha, beta, g, steps)
        cls.append(c)
        cols["R0"][s], cols["gamma"][s], cols["w"][s], cols["alpha"][s], cols["beta"][s] = R0, g, w, alpha, beta
        cols["nsteps"][s] = len(steps)
        for j, ((ci, co, o), r) in enumerate(zip(steps, rows)):
            cols["cin"][s, j], cols["cout"][s, j], cols["want"][s, j] = ci, co, o
            for f in ("a", "Rin", "Rout", "scale", "cond"):
                cols[f][s, j] = float(r[f])
            cols["da"][s, j] = [float(x) for x in r["da"]]
    for f, v in cols.items():
        out[f"{name}_{f}"] = v
    out[f"{name}_cls"] = np.array(cls)


# ---- UniV3 ----------------------------------------------------------------------------------------------------------------
def mp_direction(cp, lt, lq, cin):
    """the non-empty ticks of the direction in walk order at the mpmath price cp, the current one first:
    (k, s_in, s_out, β_out, R_out, δmax)"""
    t, ct = GS.mp_ticks(cp, lt, lq)
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


def mp_swap_out(cp, lt, lq, g, cin, o, closing=False):
    """make_quote_out_golden.mp_inverse_walk's sums at an mpmath price, and where the pool rests
    -> (a, scale, cond, new price, s' of the landing tick).  closing: o IS the direction's total as the device holds it."""
    recs = mp_direction(cp, lt, lq, cin)
    g, o = M(float(g)), M(float(o))
    price = lambda k, s: k / (s * s) if cin == 0 else (s * s) / k
    top = M(float(lt[0]))
    if o == 0:
        return M(0), M(0), M(0), cp, M(1)
    sd, sr, roots, routs = M(0), M(0), M(0), M(0)   # Σδmax, ΣR_out, Σ(k/β + s_in), Σ(s_out + β) over the drained ticks
    for j, (k, s_in, s_out, be, rout, dmax) in enumerate(recs):
        last = j == len(recs) - 1
        if not closing and (o - sr < rout):
            ot = o - sr
            d = k / (s_out - ot) - s_in
            slope = k / (s_out - ot) ** 2 / g                # ∂a/∂o
            cond = (sd + d) / g + roots / g + routs * slope + d / g + s_out * slope + o * slope
            return (sd + d) / g, (roots + s_in) / g, cond, min(price(k, s_in + d), top), s_in + d
        if dmax == mp.inf:
            return mp.inf, M(0), M(0), cp, M(1)
        sd, sr = sd + dmax, sr + rout
        roots, routs = roots + k / be + s_in, routs + s_out + be
        if last:
            if closing:
                slope = (s_in + dmax) ** 2 / k / g           # the last tick's slope at its end
                return sd / g, roots / g, sd / g + roots / g + (routs + o) * slope, min(price(k, s_in + dmax), top), s_in + dmax
            return mp.inf, M(0), M(0), cp, M(1)
    return mp.inf, M(0), M(0), cp, M(1)


L5 = np.array([4.0, 1.0, 0.25, 0.0625, 0.015625])
K5 = np.full(5, 144.0)
HOLE = np.array([144.0, 0.0, 144.0, 100.0, 81.0])
R5 = np.array([3.1, 1.7, 0.9, 0.41, 0.13])
Q5 = np.array([52.0, 870.0, 13.0, 240.0, 95.0])


def device_sum(cp, lt, lq, cin, e):
    """ΣR_out of record e of the direction (e = -1: the closing record) as the upload prepares it at the double price cp: the
    wanted amount of a boundary step is that sum BIT FOR BIT (quote_out_precise_ref's convention)"""
    prep = F.univ3_prepare(float(cp), lt, lq)
    return float((prep[1] if cin == 0 else prep[2])[e][6])


def univ3_cases():
    """(cls, cp, lt, lq, gamma, steps [(cin, want, closing)]).  Ladders of 1, 2 and 5 ticks.  The `exact` ladders have upper
    prices 4, 1, 1/4 (, 1/16, 1/64) and liquidity 144: every root of a tick edge is exact, and from the price 2.25 = 1.5² the
    roots of the current price are too (√(144/2.25) = 8, √(144·2.25) = 18), so with γ = 1 the first tick holds exactly 6 of
    coin 1 and asking for 6 costs 4 and ends EXACTLY on the edge between the first two ticks; the second tick holds 6 again.
    `boundary`: the wanted amount is a running ΣR_out of the prepared records, bit for bit; `exhausted`: it is the closing
    record's, in the direction a finite input exhausts (coin 1 in: the ladder ends at the first tick's upper price)."""
    F_ = False
    return [
        ("one_tick", 1.3, np.array([2.0]), np.array([50.0]), 0.997, [(0, 0.5, F_), (1, 0.3, F_), (0, 1.0, F_)]),
        ("one_tick", 0.7, np.array([5.0]), np.array([1e6]), 1.0, [(1, 4.0, F_), (1, 4.0, F_)]),
        ("two_ticks", 1.5, np.array([3.0, 1.0]), np.array([40.0, 90.0]), 0.997, [(0, 0.4, F_), (0, 1.5, F_), (1, 0.7, F_), (1, 0.9, F_)]),
        ("tick_edge", 2.25, L5[:2], K5[:2], 1.0, [(0, 6.0, F_), (0, 1.0, F_), (1, 0.25, F_)]),
        ("tick_edge", 2.25, L5, K5, 1.0, [(0, 6.0, F_), (0, 6.0, F_), (1, 3.0, F_)]),
        ("boundary", 2.9, R5, Q5, 0.9995, [(0, device_sum(2.9, R5, Q5, 0, 1), F_), (1, 2.0, F_)]),
        ("boundary", 1.1, R5, Q5, 0.997, [(1, device_sum(1.1, R5, Q5, 1, 0), F_), (0, 3.0, F_), (0, 2.0, F_)]),
        ("boundary", 2.25, L5, HOLE, 0.997, [(0, device_sum(2.25, L5, HOLE, 0, 1), F_), (1, 5.0, F_)]),
        ("crosses", 2.25, L5, K5, 0.997, [(0, 14.0, F_), (1, 20.0, F_), (0, 1.0, F_), (0, 0.3, F_)]),
        ("crosses", 2.9, R5, Q5, 0.9995, [(0, 8.0, F_), (0, 3.0, F_), (1, 4.0, F_)]),
        ("empty_tick", 2.25, L5, HOLE, 0.997, [(0, 5.0, F_), (1, 2.0, F_), (0, 1.0, F_)]),
        ("empty_tick", 0.5, L5, HOLE, 1.0, [(1, 1.0, F_), (0, 2.0, F_)]),
        ("exhausted", 0.1, L5, K5, 0.997, [(1, device_sum(0.1, L5, K5, 1, -1), True), (0, 2.0, F_), (0, 5.0, F_)]),
        ("exhausted", 0.3, R5, Q5, 1.0, [(1, device_sum(0.3, R5, Q5, 1, -1), True), (0, 1.0, F_)]),
        ("reversal", 1.1, R5, Q5, 0.997, [(0, 3.0, F_), (1, 3.0, F_), (0, 3.0, F_), (1, 3.0, F_)]),
    ]


def pack_univ3(out):
    cases = univ3_cases()
    S = len(cases)
    cols = dict(cp=np.zeros(S), gamma=np.zeros(S), nsteps=np.zeros(S, dtype=np.int64), cin=np.zeros((S, MAX_STEPS), dtype=np.int32),
                want=np.zeros((S, MAX_STEPS)), a=np.zeros((S, MAX_STEPS)), price=np.zeros((S, MAX_STEPS)),
                scale=np.zeros((S, MAX_STEPS)), cond=np.zeros((S, MAX_STEPS)), sland=np.ones((S, MAX_STEPS)))
    off, lts, lqs, cls = [0], [], [], []
    for s, (c, cp, lt, lq, g, steps) in enumerate(cases):
        cls.append(c)
        cols["cp"][s], cols["gamma"][s], cols["nsteps"][s] = cp, g, len(steps)
        lts.append(lt)
        lqs.append(lq)
        off.append(off[-1] + len(lt))
        P = M(float(cp))
        for j, (ci, o, closing) in enumerate(steps):
            a, sc, cd, P, sl = mp_swap_out(P, lt, lq, g, ci, o, closing)
            assert a != mp.inf, (c, s, j)
            cols["cin"][s, j], cols["want"][s, j] = ci, o
            cols["a"][s, j], cols["price"][s, j], cols["scale"][s, j], cols["cond"][s, j] = float(a), float(P), float(sc), float(cd)
            cols["sland"][s, j] = float(sl)
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
        print(name, "done", flush=True)
    pack_univ3(out)
    path = os.path.join(HERE, "swap_out_precise.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
