"""Writes tests/golden/optimum_precise.npz: a small market of every pool family, sizing cases (cfmm_size_path) and orders
(cfmm_split_paths) over it, and per case the OPTIMUM at 80 digits (stored as the nearest doubles), a noise bound of the pinned
quotes and what the contract's own search reaches when it is given exact quotes.

The truth is independent of the project's arithmetic, as make_quote_golden.py's is, and reuses that file's `truth`, `root`, φ's,
closed forms and `mp_ticks` by import: a hop's exact quote is the root of φ itself by bisection (UniV3: the reference's
tick-by-tick walk over `mp_ticks`, restated here for an 80-digit amount and cross-checked against `mp_walk` at the rounded
amount); a path's quote chains them without rounding.  The closed forms appear only as a cross-check of every hop at the
optimum (1e-40) and in the conditioning sums.

The market: seven segments in the order of SEGMENTS (tests/optimum_ref.py).  The smooth families are drawn like the `typical`
rows of quote_precise.npz (γ, weights, α) on pegged reserves of one common scale L·exp(N(0, 0.1)), L = 1e3·exp(N(0, 1)) -- an
amount stays a trade of comparable size at every hop; row 0 of the product and geomean segments is 64 times deeper.  The UniV3
segment IS pools 0, 1, 2 and 4 of quote_precise.npz: 70 ticks (depths 1, 5, 64 with coin 0 in; exhausted after two with coin 1
in), 8 ticks, 8 ticks with empty ones, a single tick.

Sizing cases: gain(x) = v_out·q(x) − v_in·x with v_out = 1 and v_in the path's exact marginal rate at a chosen x_t (rounded), so
the optimum x* is interior; max_in = x_t·10^U(0.1, 2).  Classes: `interior` (every family alone and mixed, 1-3 hops), `kink`
(first hop UniV3, x_t on a tick boundary, v_in the geometric mean of the two one-sided rates there: neighbouring ticks share their
boundary price, so there the rate is continuous and only the curvature jumps -- the quote changes records; across an EMPTY tick,
pool 2 at depth 2 with coin 0 in and depth 1 with coin 1 in, the rate itself jumps), `plateau` (first hop
UniV3 with coin 1 in, x_t where the list is exhausted, v_in half the rate from below: beyond it the quote is flat), `solidly_small`
(a two-pool Solidly cycle sized at 1e-6 .. 1e-4.1 of the reserve), `hops8`.  x* = sup{x : gain(x + h) > gain(x)}, h = 1e-30·max_in,
by bisection on values only (90 halvings of [0, max_in]); g* = gain(x*).  A case of another class than `solidly_small` whose gain
comes out so thin that 128·16·e > g*/2000 (the tests' condition on the inputs, with a factor two to spare) is sized again at
twice the x_t.  Also stored: −gain″(x*) and the smaller one-sided slope of the gain at x* (how sharp the optimum is).

Orders: K in {1, 2, 3, 4, 8} pool-disjoint paths of one or two hops.  The multiplier λ is CHOSEN (below the marginal rates at 0
of the paths that are to be used), x_k(λ) = sup{x : q_k(x + h) − q_k(x) >= λh} by bisection on exact quotes, A = the double next
to Σ x_k, and the shares are renormalised to Σ x_k = A over the paths that are neither empty nor pinned on a kink (equal
marginals: the total changes by O(δ²) whichever way δ = A − Σ x_k is spread).  Kinds: `general`, `stall` (8 paths, path 0 through
the deep product pool carries most of A), `empty` (λ between the two lowest rates at 0: one path gets +0), `kink` (path 0 is
one UniV3 hop held on a tick boundary, λ the geometric mean of its one-sided rates there), `plateau` (a UniV3 path that can
be exhausted, λ below its last rate), `one` (K = 1: the share is A).

The noise bound e of a path at x: Σ over its hops of K·u·(R_o + out + cond) (quote_precise_ref.bound; K the family's largest K
of quote_precise_ref.K_of, cond make_quote_golden's conditioning sums) carried through the later hops' exact rates.  A sizing
case stores v_out·e + u·(v_out·q + v_in·x + g) (the three roundings of the gain); an order Σ_k e_k + K·u·T* (its sum).

Resolution: tests/size_path_ref.py and tests/split_paths_ref.py run for 16 rounds over the exact quotes rounded once to
double; the answer after each round r = 1 .. 16 is stored (`*_ref` arrays: a round does not know how many follow).

usage: python tests/golden/make_optimum_golden.py        (needs mpmath; deterministic: seeded; a quarter of an hour on 8 cores;
       `... N FILE` writes every N-th case to FILE instead: a quick look, not the fixture)"""
import functools
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_quote_golden as Q  # noqa: E402   (sets mp.mp.dps = 80)
import optimum_ref as O  # noqa: E402
import quote_precise_ref as P  # noqa: E402
from make_rate_golden import save  # noqa: E402
from size_path_ref import size_path_ref  # noqa: E402
from split_paths_ref import split_paths_ref  # noqa: E402

M = mp.mpf
U = M(2) ** -53
H = 8
ROUNDS = 16
SIZE_CLASSES = ["interior", "kink", "plateau", "solidly_small", "hops8"]
ORDER_KINDS = ["general", "stall", "empty", "kink", "plateau", "one"]
UNIV3_POOLS = (0, 1, 2, 4)
N_POOLS = 8                  # per smooth segment
rng = np.random.default_rng(20240923)
MK = {}                      # segment name -> arrays (filled by make_market before the workers fork)


# ---- the market -----------------------------------------------------------------------------------------------------------------
def make_market():
    fx = P.load()
    for name in O.SEGMENTS:
        if name == "univ3":
            g = P.group(fx, "univ3")
            pools = [P.univ3_pool(g, p) for p in UNIV3_POOLS]
            MK[name] = dict(current_price=np.array([p[0] for p in pools]), pool_gamma=np.array([p[3] for p in pools]),
                            tick_off=np.cumsum([0] + [len(p[1]) for p in pools]).astype(np.int64),
                            lower_ticks=np.concatenate([p[1] for p in pools]), liquidity=np.concatenate([p[2] for p in pools]))
            continue
        n = O.N_COINS[name]
        L = 1e3 * np.exp(rng.normal(0.0, 1.0, N_POOLS))
        if name in ("product", "geomean"):
            L[0] = 64e3
        R = L[:, None] * np.exp(rng.normal(0.0, 0.1, (N_POOLS, n)))
        d = dict(R=R, gamma=rng.choice([0.997, 0.9995, 1.0], N_POOLS))
        if name in ("geomean", "weighted3"):
            d["w"] = rng.dirichlet(np.ones(n) * 2.0, N_POOLS)
        if name.startswith("curve"):
            d["alpha"] = np.exp(rng.uniform(np.log(0.1), np.log(10.0), N_POOLS))
            d["beta"] = d["alpha"] * np.exp(np.mean(np.log(R), axis=1)) * np.prod(R, axis=1)       # P₀ = α·R_ref
        MK[name] = d


def univ3(p):
    g = MK["univ3"]
    a, b = int(g["tick_off"][p]), int(g["tick_off"][p + 1])
    return float(g["current_price"][p]), g["lower_ticks"][a:b], g["liquidity"][a:b], float(g["pool_gamma"][p])


@functools.lru_cache(maxsize=None)
def ticks(p):
    cp, lt, lq, _ = univ3(p)
    return Q.mp_ticks(cp, lt, lq)


def walk(p, cin, a):
    """trade_through_pools for an 80-digit amount over mp_ticks' records (mp_walk rounds the amount to a double first)"""
    t, ct = ticks(p)
    nt = len(t) - 1
    d, lam = M(univ3(p)[3]) * a, M(0)
    for idx in (range(ct, nt + 1) if cin == 0 else range(ct, 0, -1)):
        k, al, be, R1, R2 = t[idx]
        if cin == 1:
            al, be, R1, R2 = be, al, R2, R1
        if k == 0:
            continue
        mx = k / be - (R1 + al) if be > 0 else mp.inf
        if mx > d:
            return lam + min(R2, (R2 + be) - k / (R1 + al + d))
        lam += R2
        d -= mx
    return lam


def boundary(p, cin, depth):
    """the amount that drains exactly the first `depth` non-empty ticks"""
    return Q.mp_sum_dmax(*univ3(p)[:3], cin, depth)[0] / M(univ3(p)[3])


def phi_of(name, r):
    g = MK[name]
    if name == "product":
        return lambda RR: RR[0] * RR[1]
    if name == "solidly":
        return Q.phi_solidly
    if name in ("geomean", "weighted3"):
        wm = [M(float(x)) for x in g["w"][r]]
        return lambda RR: Q.phi_weighted(RR, wm)
    al, be = M(float(g["alpha"][r])), M(float(g["beta"][r]))
    return lambda RR: Q.phi_curve(RR, al, be)


def exact_hop(hop, a):
    s, r, ci, co = hop
    if a == 0:
        return M(0)
    name = O.SEGMENTS[s]
    if name == "univ3":
        return walk(r, ci, a)
    g = MK[name]
    return Q.truth(phi_of(name, r), g["R"][r], float(g["gamma"][r]), ci, co, a)


def exact_path(hops, x):
    for hop in hops:
        x = exact_hop(hop, x)
    return x


def rate(f, x, h, side=+1):
    """one-sided difference quotient of f at x"""
    return (f(x + h) - f(x)) / h if side > 0 else (f(x) - f(x - h)) / h


def first_scale(hop):
    s, r, ci, co = hop
    if O.SEGMENTS[s] == "univ3":                                # the current tick's capacity (the single tick with coin 0 in has none: √k)
        d = Q.mp_dmaxes(*univ3(r)[:3], ci)[0]
        return float(d / M(univ3(r)[3])) if d != mp.inf else float(np.sqrt(univ3(r)[2][0]))
    return float(MK[O.SEGMENTS[s]]["R"][r, ci])


# ---- the noise bound ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def K_family(name):
    fam = P.family(name)
    return max(P.K_of(name, c) for (f, c) in P.K_MEASURED if f == fam)


def hop_bound(hop, a, out):
    """K·u·(R_o + out + cond) of one hop at the amount a, and the cross-check of `out` against the closed form"""
    s, r, ci, co = hop
    name = O.SEGMENTS[s]
    if name == "univ3":
        cp, lt, lq, gm = univ3(r)
        o, scale, cond = Q.mp_walk(cp, lt, lq, gm, ci, float(a))
        Q.check(o, walk(r, ci, M(float(a))), "univ3")
        return K_family(name) * U * (scale + out + cond)
    g = MK[name]
    Rm = [M(float(x)) for x in g["R"][r]]
    gm = M(float(g["gamma"][r]))
    if name == "product":
        cf = lambda Ri, Ro, gg, aa: Ro * gg * aa / (Ri + gg * aa)
        xs = [Rm[ci], Rm[co], gm, a]
    elif name == "solidly":
        cf, xs = Q.cf_solidly, [Rm[ci], Rm[co], gm, a]
    elif name in ("geomean", "weighted3"):
        cf, xs = Q.cf_weighted, [Rm[ci], Rm[co], M(float(g["w"][r, ci])), M(float(g["w"][r, co])), gm, a]
    else:
        be = M(float(g["beta"][r]))
        pr = M(1)
        for x in Rm:
            pr *= x
        lP0 = mp.log(be / pr)
        cf, xs = Q.cf_curve, [Rm[ci], Rm[co], M(float(g["alpha"][r])), lP0, gm, a]
        Q.check(out, cf(*xs), name)
        # as make_quote_golden.make_curve: log β and every log R_k enter through log P₀ (argument 3)
        logs = abs(mp.log(be)) + sum(abs(mp.log(x)) for x in Rm)
        cond = M(0)
        for j in (0, 1, 2, 4, 5):
            if xs[j] != 0:
                cond += abs(xs[j] * mp.diff(lambda t, j=j: cf(*[t if k == j else xs[k] for k in range(6)]), xs[j]))
        cond += logs * abs(mp.diff(lambda t: cf(xs[0], xs[1], xs[2], t, xs[4], xs[5]), lP0))
        return K_family(name) * U * (Rm[co] + out + cond)
    Q.check(out, cf(*xs), name)
    return K_family(name) * U * (Rm[co] + out + Q.cond_sum(cf, xs))


def path_bound(hops, x):
    """(q(x), the propagated bound): e <- e·(the hop's exact rate) + the hop's own bound, hop by hop"""
    e = M(0)
    for hop in hops:
        if x == 0:
            return M(0), e
        y = exact_hop(hop, x)
        h = x * M(10) ** -30
        r = max(rate(lambda t: exact_hop(hop, t), x, h, +1), rate(lambda t: exact_hop(hop, t), x, h, -1))
        e = e * r + hop_bound(hop, x, y)
        x = y
    return x, e


def rounded_quoter(paths):
    """size_path_ref's / split_paths_ref's market: exact quotes rounded once to double"""
    def quote_path(idx, x):
        return np.array([float(exact_path(paths[int(p)], M(float(v)))) for p, v in zip(idx, x)])
    return quote_path


def sup(pred, hi, halvings=90):
    """sup{x in [0, hi] : pred(x)} for a pred that is true below it and false above"""
    lo, hi = M(0), M(hi)
    for _ in range(halvings):
        mid = (lo + hi) / 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


# ---- sizing ---------------------------------------------------------------------------------------------------------------------
def size_case(spec):
    cls, hops, u_t, u_max, at = spec
    q = lambda x: exact_path(hops, x)
    if cls in ("kink", "plateau"):
        p, cin, depth = at
        x_t = boundary(p, cin, depth)
        h = x_t * M(10) ** -30
        rL, rR = rate(q, x_t, h, -1), rate(q, x_t, h, +1)
        assert rL > rR >= 0 and (rR < rL * M(10) ** -30) == (cls == "plateau"), (cls, hops, rL, rR)
        vi = float(rL / 2 if cls == "plateau" else mp.sqrt(rL * rR))
    else:
        x_t = M(first_scale(hops[0]) * 10.0 ** u_t)
        h0 = x_t * M(10) ** -30
        while rate(q, x_t, x_t * M(10) ** -30) < q(h0) / h0 / 1000:     # beyond a UniV3 list's end further down the path: come back
            x_t /= 4
    vo = 1.0
    while True:
        if cls not in ("kink", "plateau"):
            vi = float(rate(q, x_t, x_t * M(10) ** -30))
        max_in = float(x_t) * 10.0 ** u_max
        gain = lambda x: M(vo) * q(x) - M(vi) * x
        h = M(max_in) * M(10) ** -30
        xs = sup(lambda x: gain(x + h) > gain(x), max_in)
        y, e = path_bound(hops, xs)
        gs = M(vo) * y - M(vi) * xs
        assert 0 < xs < M(max_in) and gs > 0, (cls, hops, xs, gs)
        e = M(vo) * e + U * (M(vo) * y + M(vi) * xs + gs)
        # the condition the tests put on the inputs (128·16·e <= 1e-3·g*) with a factor two to spare: a gain so thin that the
        # quotes' noise could hide a thousandth of it is sized further up the curve (`solidly_small` is that case on purpose)
        if cls in ("kink", "plateau", "solidly_small") or 128 * 16 * e <= gs / 2000:
            break
        x_t *= 2
    # how sharp the optimum is: −gain″(x*) by a second difference (meaningful on the smooth classes) and the two one-sided
    # slopes by which the gain falls away from x* (meaningful on a kink)
    hh = xs * M(10) ** -20
    curv = -(gain(xs + hh) - 2 * gs + gain(xs - hh)) / hh ** 2
    hs = M(max_in) * M(10) ** -20                                    # (well above the bisection's resolution of x*)
    slope = min((gs - gain(xs - hs)) / hs, (gs - gain(xs + hs)) / hs)
    trace = []
    size_path_ref(rounded_quoter([hops]), [max_in], [vi], [vo], rounds=ROUNDS, trace=trace)
    x_ref = [float(x[0, j[0]]) for x, g, j in trace]
    g_ref = [float(g[0, j[0]]) for x, g, j in trace]
    return dict(cls=cls, hops=hops, max_in=max_in, vi=vi, vo=vo, x=float(xs), q=float(y), g=float(gs), e=float(e), curv=float(curv),
                slope=float(slope), x_ref=x_ref, g_ref=g_ref)


def random_hop(s, used):
    name = O.SEGMENTS[s]
    n_rows = len(UNIV3_POOLS) if name == "univ3" else N_POOLS
    free = [r for r in range(n_rows) if (s, r) not in used]
    r = int(free[rng.integers(len(free))])
    n = O.N_COINS[name]
    ci = int(rng.integers(n))
    co = int((ci + 1 + rng.integers(n - 1)) % n)
    used.add((s, r))
    return (s, r, ci, co)


def random_path(segs, used=None):
    used = set() if used is None else used
    return tuple(random_hop(s, used) for s in segs)


def mixed(n):
    """n segments, not all the same"""
    while True:
        segs = [int(s) for s in rng.integers(len(O.SEGMENTS), size=n)]
        if len(set(segs)) > 1 and segs.count(3) <= len(UNIV3_POOLS):
            return segs


def size_specs():
    specs = []
    S = len(O.SEGMENTS)
    draw = lambda lo=-3.0, hi=-0.5: (float(rng.uniform(lo, hi)), float(rng.uniform(0.1, 2.0)))
    for s in range(S):                                   # every family alone: 1, 2, 3 hops, twice
        for n in (1, 2, 3) * 2:
            specs.append(("interior", random_path([s] * n), *draw(), None))
    for k in range(34):                                  # mixed: 2 and 3 hops
        specs.append(("interior", random_path(mixed(2 + k % 2)), *draw(), None))
    u3 = O.SEGMENTS.index("univ3")
    for k, (p, cin, depth) in enumerate([(0, 0, 1), (0, 0, 5), (0, 0, 64), (0, 1, 1), (1, 0, 2), (1, 1, 3), (2, 0, 2), (2, 1, 1)]):
        used = {(u3, p)}
        tail = tuple(random_hop(s if s != u3 else 0, used) for s in mixed(3)[:k % 3])        # (one UniV3 hop: one kink)
        specs.append(("kink", ((u3, p, cin, 1 - cin),) + tail, 0.0, draw()[1], (p, cin, depth)))
    for k, p in enumerate((0, 1, 2, 3, 0, 1)):           # coin 1 in: the list ends (row 3 is the single tick)
        used = {(u3, p)}
        tail = tuple(random_hop(s if s != u3 else 0, used) for s in mixed(3)[:(k // 4) * (1 + k % 2)])
        depth = len(Q.mp_dmaxes(*univ3(p)[:3], 1))
        specs.append(("plateau", ((u3, p, 1, 0),) + tail, 0.0, draw()[1], (p, 1, depth)))
    so = O.SEGMENTS.index("solidly")
    for k in range(8):
        a, b = (int(r) for r in rng.choice(N_POOLS, 2, replace=False))
        c = int(rng.integers(2))
        specs.append(("solidly_small", ((so, a, c, 1 - c), (so, b, 1 - c, c)), *draw(-6.0, -4.1), None))
    for s in (0, 1, 2, 4, 5, 6):                         # eight hops: every family that has eight pools, and mixed
        specs.append(("hops8", random_path([s] * H), *draw(), None))
    for k in range(6):
        specs.append(("hops8", random_path(mixed(H)), *draw(), None))
    return specs


# ---- splitting ------------------------------------------------------------------------------------------------------------------
def order_case(spec):
    kind, paths, u_l, at = spec
    K = len(paths)
    qs = [functools.partial(exact_path, p) for p in paths]
    scale = [first_scale(p[0]) for p in paths]
    h0 = [M(s) * M(10) ** -30 for s in scale]
    pinned = [False] * K
    if kind == "one":
        A = scale[0] * 10.0 ** u_l
        x = [M(A)]
    else:
        r0 = [qk(h) / h for qk, h in zip(qs, h0)]
        asc = sorted(r0)
        if kind == "empty":
            lam = mp.sqrt(asc[0] * asc[1])
        elif kind == "kink":
            b = boundary(*at)
            rL, rR = rate(qs[0], b, h0[0], -1), rate(qs[0], b, h0[0], +1)
            assert rL > rR > 0
            lam = mp.sqrt(rL * rR)
        elif kind == "plateau":                              # path 0 ends: λ below the last rate it has
            b = boundary(*at)
            lam = min(rate(qs[0], b, h0[0], -1), asc[0]) * M(10.0 ** -u_l)
        else:
            lam = asc[0] * M(10.0 ** -u_l)
        x = []
        for k in range(K):
            above = lambda t, k=k: qs[k](t + h0[k]) - qs[k](t) >= lam * h0[k]
            hi = M(1e3 * scale[k])
            while above(hi):                                    # (a first tick much smaller than the pool)
                hi *= 8
            x.append(sup(above, hi) if r0[k] > lam else M(0))
        if kind in ("kink", "plateau"):
            assert abs(x[0] - b) <= b * M(10) ** -20, (kind, x[0], b)
            x[0], pinned[0] = b, True
        A = float(sum(x))
        free = [k for k in range(K) if x[k] > 0 and not pinned[k]]
        tot = sum(x[k] for k in free)
        delta = M(A) - sum(x)
        for k in free:
            x[k] += delta * x[k] / tot
        assert sum(x) == M(A) or abs(sum(x) - M(A)) <= M(A) * M(10) ** -70
    T, e, curv = M(0), M(0), []
    for k in range(K):
        y, ek = path_bound(paths[k], x[k])
        T, e = T + y, e + ek
        # −q_k″ at the share by a second difference; 0 where the share is +0 or pinned on a kink (no curvature to speak of)
        hh = x[k] * M(10) ** -20
        curv.append(float(-(qs[k](x[k] + hh) - 2 * y + qs[k](x[k] - hh)) / hh ** 2) if x[k] > 0 and not pinned[k] else 0.0)
    e += K * U * T
    first = np.array([0, K])
    trace = []
    split_paths_ref(rounded_quoter(paths), first, [A], rounds=ROUNDS, trace=trace)
    share_ref, T_ref = [], []
    for xg, yg, n, rem in trace:
        share_ref.append([float(xg[0, k, n[0, k]]) for k in range(K)])
        t = yg[0, 0, n[0, 0]]
        for k in range(1, K):
            t = t + yg[0, k, n[0, k]]
        T_ref.append(float(t))
    return dict(kind=kind, paths=paths, A=A, share=[float(v) for v in x], T=float(T), e=float(e), curv=curv, share_ref=share_ref,
                T_ref=T_ref)


def order_specs():
    specs = []
    S = len(O.SEGMENTS)
    u3, pr = O.SEGMENTS.index("univ3"), O.SEGMENTS.index("product")

    def paths_of(K, segs=None, used=None):
        used = set() if used is None else used
        out = []
        for k in range(K):
            n = 1 + int(rng.integers(2))
            sg = [segs] * n if segs is not None else [int(s) for s in rng.integers(S, size=n)]
            path = []
            for s in sg:                                    # (UniV3 has four pools: a fifth hop through it becomes a product hop)
                full = s == u3 and sum(1 for t in used if t[0] == u3) == len(UNIV3_POOLS)
                path.append(random_hop(pr if full else s, used))
            out.append(tuple(path))
        return tuple(out)
    ul = lambda: float(rng.uniform(0.005, 0.15))
    for K in (1, 2, 3, 4, 8):
        for s in (0, 1, 2, 4, 5, 6):                       # single-family orders (UniV3 has four pools: in the mixed ones)
            hops1 = tuple(random_path([s], u) for u in [set()] for _ in range(K)) if K == 8 else paths_of(K, s)
            specs.append(("one" if K == 1 else "general", hops1, float(rng.uniform(-2.0, -0.5)) if K == 1 else ul(), None))
        for _ in range(4 if K > 1 else 3):                  # mixed
            specs.append(("one" if K == 1 else "general", paths_of(K), float(rng.uniform(-2.0, -0.5)) if K == 1 else ul(), None))
    used = {(pr, 0)}                                        # the documented stall shape: the deep pool beside seven shallow paths
    deep = ((pr, 0, 0, 1),)
    specs.append(("stall", (deep,) + tuple(random_path([int(rng.integers(S))], used) for _ in range(7)), 0.009, None))
    specs.append(("empty", paths_of(3), 0.0, None))
    specs.append(("empty", paths_of(8), 0.0, None))
    for (p, cin, depth), K in (((0, 0, 5), 2), ((2, 1, 1), 4)):
        used = {(u3, p)}
        specs.append(("kink", (((u3, p, cin, 1 - cin),),) + paths_of(K - 1, used=used), 0.0, (p, cin, depth)))
    for p, K in ((0, 2), (1, 3)):
        used = {(u3, p)}
        depth = len(Q.mp_dmaxes(*univ3(p)[:3], 1))
        specs.append(("plateau", (((u3, p, 1, 0),),) + paths_of(K - 1, used=used), ul(), (p, 1, depth)))
    return specs


# ---- the file -------------------------------------------------------------------------------------------------------------------
def hop_arrays(paths):
    n = len(paths)
    n_hops = np.array([len(p) for p in paths], dtype=np.int32)
    seg, ci, co = (np.zeros((n, H), dtype=np.int32) for _ in range(3))
    row = np.zeros((n, H), dtype=np.int64)
    for q, p in enumerate(paths):
        for k, (s, r, a, b) in enumerate(p):
            seg[q, k], row[q, k], ci[q, k], co[q, k] = s, r, a, b
    return dict(n_hops=n_hops, seg=seg, row=row, ci=ci, co=co)


def main():
    make_market()
    s_specs, o_specs = size_specs(), order_specs()
    if len(sys.argv) > 1:                                   # a debugging subset: every n-th case, written elsewhere
        s_specs, o_specs = s_specs[::int(sys.argv[1])], o_specs[::int(sys.argv[1])]
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count())) as pool:
        orders = list(pool.imap(order_case, o_specs, chunksize=1))
        sized = list(pool.imap(size_case, s_specs, chunksize=1))
    out = {"segments": np.array(O.SEGMENTS), "size_classes": np.array(SIZE_CLASSES), "order_kinds": np.array(ORDER_KINDS)}
    for name, d in MK.items():
        for k, v in d.items():
            out[f"{name}_{k}"] = v
    for k, v in hop_arrays([c["hops"] for c in sized]).items():
        out[f"size_{k}"] = v
    out["size_cls"] = np.array([SIZE_CLASSES.index(c["cls"]) for c in sized], dtype=np.int32)
    for k in ("max_in", "vi", "vo", "x", "q", "g", "e", "curv", "slope", "x_ref", "g_ref"):
        out[f"size_{k}"] = np.array([c[k] for c in sized], dtype=np.float64)
    for k, v in hop_arrays([p for c in orders for p in c["paths"]]).items():
        out[f"split_{k}"] = v
    out["split_first"] = np.cumsum([0] + [len(c["paths"]) for c in orders]).astype(np.int64)
    out["split_kind"] = np.array([ORDER_KINDS.index(c["kind"]) for c in orders], dtype=np.int32)
    for k in ("A", "T", "e", "T_ref"):
        out[f"split_{k}"] = np.array([c[k] for c in orders], dtype=np.float64)
    out["split_share"] = np.array([v for c in orders for v in c["share"]], dtype=np.float64)
    out["split_curv"] = np.array([v for c in orders for v in c["curv"]], dtype=np.float64)
    out["split_share_ref"] = np.array([[c["share_ref"][r][k] for r in range(ROUNDS)] for c in orders for k in range(len(c["paths"]))], dtype=np.float64)
    path = O.FIXTURE if len(sys.argv) == 1 else sys.argv[2]
    save(path, out)
    print(path, os.path.getsize(path), "bytes;", len(sized), "sizing cases,", len(orders), "orders,", out["split_share"].size, "paths")


if __name__ == "__main__":
    main()
