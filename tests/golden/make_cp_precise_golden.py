"""Regenerates tests/golden/cp_precise.npz: ProductTwoCoin and UniV3 / BoundedProduct trades to 60 significant digits.

    python tests/golden/make_cp_precise_golden.py

Conventions of make_precise_golden.py: inputs are float64 exactly as the device receives them and are taken as exact; every
truth is computed from them in mpmath at 60 digits and rounded ONCE to float64 (`_f`).  Nothing here calls libm: powers
and exponentials of the inputs are mpmath's, and an input placed near a threshold is constructed in mpmath and then
rounded, so the file is the same on every host.  Nothing is read from, or derived by running, the reference.

Product truth: the closed forms of find_arb! (src/cfmms.jl:125-140) in exact arithmetic, all four outputs.  A few hundred
pools are checked against the KKT conditions solved by bisection on the tendered reserve ratio.

UniV3 truth: NO tick walk.  The pool is a sum of independent bounded-product ticks, tick i with k_i = liquidity[i] on
(p⁻_i, p⁺_i] = (lower_ticks[i+1] or 0, lower_ticks[i]].  With pr = v₁/v₂ the pool does not trade iff γ·cp <= pr <= cp/γ;
otherwise its marginal price moves from cp to P = pr/γ (price falling) or γ·pr (price rising), and every tick moves from
a = clamp_i(cp) to b = clamp_i(P):
    falling   γ·Δ₁ = Σ √k_i (1/√b − 1/√a),   Λ₂ = Σ √k_i (√a − √b)
    rising    γ·Δ₂ = Σ √k_i (√b − √a),       Λ₁ = Σ √k_i (1/√a − 1/√b).
A few hundred pools are checked against an exact tick-by-tick forward trade (amount out for an amount in) with bisection
on the tendered amount until the marginal price is P.  Both checks must agree with the truth to 40 digits or the script
fails.

Cases (`pcases` / `ucases`; arrays are `<case>_<field>`; `cls` indexes `pclasses` / `uclasses`; `zclear` marks the trades
whose truth is zero with the no-trade condition clear by more than a relative 2^-40):
  product  p_main    n = 64: well / band_edge (v₁R₁ = γv₂R₂(1 ± 2^-k) in either direction, k = 10..52, and the no-fee
                     parity point) / gamma1 (γ = 1 within 2^-40 of equilibrium) / both_live (γ > 1) / wide (reserves over
                     1e-9..1e12, prices over 1e±6); also v2, the prices of the update test
           p_resout  n = 16: reserves beyond 2^±150 (the upload clears the fast flag)
           p_pxout   n = 16: one price beyond 2^150
  univ3    u_main    n = 64: inside / walk_head / walk_deep / drained_all / on_boundary / cp_on_tick / empty_cur / narrow /
                     band / gamma / wide (see the builders below); also v2
                     (on_boundary also holds P exactly on a boundary and 1..3 ulps on either side of it)
           u_resout  n = 16: liquidity scaled by 2^±200 (the upload clears the fast flag)
           bounded   n = 16: two-tick pools with an empty second tick (no walk list anywhere: the lean kernel):
                     inside / drained_all / band / cp_on_tick / narrow
"""
import os
import zipfile

import mpmath as mp
import numpy as np

DPS = 60
mp.mp.dps = DPS
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cp_precise.npz")

PCLASSES = ["well", "band_edge", "gamma1", "both_live", "wide", "res_out", "px_out"]
UCLASSES = ["inside", "walk_head", "walk_deep", "drained_all", "on_boundary", "cp_on_tick", "empty_cur", "narrow", "band",
            "gamma", "wide", "res_out"]
MARGIN = mp.mpf(2) ** -40


def _f(x):
    """mpf -> the nearest float64 (ties to even): the one rounding of every stored value."""
    return mp.libmp.to_float(mp.mpf(x)._mpf_, rnd=mp.libmp.round_nearest)


def _M(x):
    return mp.mpf(float(x))


def _p10(u):
    return _f(mp.power(10, mp.mpf(float(u))))


def _p2(u):
    return _f(mp.power(2, mp.mpf(float(u))))


# ---- Product truth ------------------------------------------------------------------------------------------------

def prod_truth(R, g, v):
    """find_arb! of one ProductTwoCoin pool (src/cfmms.jl:125-140) in exact arithmetic -> (Δ₁, Δ₂, Λ₁, Λ₂) as mpf."""
    R1, R2, g, v1, v2 = (_M(x) for x in (R[0], R[1], g, v[0], v[1]))
    k = R1 * R2
    z = mp.mpf(0)
    d1 = max(mp.sqrt(g * (v2 / v1) * k) - R1, z) / g
    d2 = max(mp.sqrt(g * (v1 / v2) * k) - R2, z) / g
    l1 = max(R1 - mp.sqrt(k / ((v1 / v2) * g)), z)
    l2 = max(R2 - mp.sqrt(k / ((v2 / v1) * g)), z)
    return d1, d2, l1, l2


def prod_clear(R, g, v):
    """per direction: the direction is dead (γ·v_out·R_out < v_in·R_in) by more than a relative 2^-40"""
    R1, R2, g, v1, v2 = (_M(x) for x in (R[0], R[1], g, v[0], v[1]))
    return [g * v2 * R2 < v1 * R1 * (1 - MARGIN), g * v1 * R1 < v2 * R2 * (1 - MARGIN)]


def prod_kkt(R, g, v):
    """Independent check: direction 1 tenders coin 1 to X = ρ·R₁ (ρ >= 1), the invariant gives Y = R₂/ρ, and optimality
    is the pool's marginal price Y/X equal to v₁/(γ·v₂); h(ρ) = log(Y/X) − log(v₁/(γ·v₂)) decreases in ρ."""
    R1, R2, g, v1, v2 = (_M(x) for x in (R[0], R[1], g, v[0], v[1]))
    out = []
    for rb, ra, vb, va in ((R1, R2, v1, v2), (R2, R1, v2, v1)):
        target = mp.log(vb / (g * va))
        h = lambda lr: mp.log(ra) - mp.log(rb) - 2 * lr - target
        if h(mp.mpf(0)) <= 0:
            out.append((mp.mpf(0), mp.mpf(0)))
            continue
        lo, hi = mp.mpf(0), mp.mpf(1)
        while h(hi) > 0:
            hi *= 2
        for _ in range(260):
            mid = (lo + hi) / 2
            if h(mid) > 0:
                lo = mid
            else:
                hi = mid
        rho = mp.exp((lo + hi) / 2)
        out.append(((rb * rho - rb) / g, ra - ra / rho))
    (d1, l2), (d2, l1) = out
    return d1, d2, l1, l2


# ---- UniV3 truth --------------------------------------------------------------------------------------------------

def _clamp(x, lo, hi):
    return min(max(x, lo), hi)


def v3_truth(cp, lt, lq, g, v):
    """One UniV3 pool as a sum of independent bounded-product ticks -> (Δ₁, Δ₂, Λ₁, Λ₂) as mpf."""
    cp, g, v1, v2 = _M(cp), _M(g), _M(v[0]), _M(v[1])
    z = mp.mpf(0)
    pr = v1 / v2
    if g * cp <= pr <= cp / g:
        return z, z, z, z
    falling = pr < g * cp
    P = pr / g if falling else g * pr
    tin, tout = [], []
    nt = len(lt)
    for i in range(nt):
        if lq[i] == 0:
            continue
        rk = mp.sqrt(_M(lq[i]))
        hi = _M(lt[i])
        lo = _M(lt[i + 1]) if i + 1 < nt else z
        a, b = _clamp(cp, lo, hi), _clamp(P, lo, hi)
        if a == b:
            continue
        if falling:
            tin.append(rk * (1 / mp.sqrt(b) - 1 / mp.sqrt(a)))
            tout.append(rk * (mp.sqrt(a) - mp.sqrt(b)))
        else:
            tin.append(rk * (mp.sqrt(b) - mp.sqrt(a)))
            tout.append(rk * (1 / mp.sqrt(a) - 1 / mp.sqrt(b)))
    d, lam = mp.fsum(tin) / g, mp.fsum(tout)
    return (d, z, z, lam) if falling else (z, d, lam, z)


def v3_clear(cp, g, v):
    """the pool sits inside its no-arbitrage band by more than a relative 2^-40 on both sides"""
    cp, g, pr = _M(cp), _M(g), _M(v[0]) / _M(v[1])
    return bool(g * cp * (1 + MARGIN) <= pr <= cp / g * (1 - MARGIN))


def v3_forward(cp, lt, lq, g, v):
    """Independent check: the exact tick-by-tick forward trade (amount out for a net amount in), bisected on the amount
    until the pool's marginal price is P.  In the coordinate u = 1/√p (price falling) or √p (price rising) a tick of
    invariant k takes √k·(u_b − u_a) and gives √k·(1/u_a − 1/u_b); u grows along the walk in both directions."""
    cp, g, v1, v2 = _M(cp), _M(g), _M(v[0]), _M(v[1])
    z = mp.mpf(0)
    pr = v1 / v2
    if g * cp <= pr <= cp / g:
        return z, z, z, z
    falling = pr < g * cp
    P = pr / g if falling else g * pr
    nt = len(lt)
    ct = sum(1 for x in lt if _M(x) >= cp) - 1                     # 0-based current tick
    U = 1 / mp.sqrt(P) if falling else mp.sqrt(P)
    order = range(ct, nt) if falling else range(ct, -1, -1)
    walk = []                                                      # (√k, u at entry, u at the far boundary)
    for i in order:
        hi = _M(lt[i])
        lo = _M(lt[i + 1]) if i + 1 < nt else z
        near = cp if i == ct else (hi if falling else lo)
        if falling:
            ua, ub = 1 / mp.sqrt(near), (1 / mp.sqrt(lo) if lo > 0 else mp.inf)
        else:
            ua, ub = mp.sqrt(near), mp.sqrt(hi)
        walk.append((mp.sqrt(_M(lq[i])), ua, ub))
    caps = [rk * (ub - ua) for rk, ua, ub in walk]
    outs = [rk * (1 / ua - 1 / ub) if rk > 0 else z for rk, ua, ub in walk]

    def trade(x):
        """-> (u after tendering x, amount out); u = inf when every tick is drained"""
        out = z
        for (rk, ua, ub), c, o in zip(walk, caps, outs):
            if rk == 0:
                continue
            if x < c:
                u = ua + x / rk
                return u, out + rk * (1 / ua - 1 / u)
            x -= c
            out += o
        return mp.inf, out

    total = mp.fsum(c for (rk, _, _), c in zip(walk, caps) if rk > 0)
    if total == 0:
        return z, z, z, z
    lo, hi = z, min(total, mp.mpf(1)) if total < mp.inf else mp.mpf(1)
    while hi < total and trade(hi)[0] < U:
        hi = min(hi * 2, total)
    for _ in range(400):
        mid = (lo + hi) / 2
        if trade(mid)[0] < U:
            lo = mid
        else:
            hi = mid
    x = (lo + hi) / 2
    if total < mp.inf and total - x <= mp.mpf(10) ** -50 * total:                     # every tick drains: the price jumps past P at `total`
        x, out = total, mp.fsum(outs)
    else:
        out = trade(x)[1]
    return (x / g, z, z, out) if falling else (z, x / g, out, z)


# ---- inputs -------------------------------------------------------------------------------------------------------

def _pairs(rng, m, lo, hi):
    a = rng.integers(lo, hi, m)
    b = rng.integers(lo, hi - 1, m)
    b = b + (b >= a)
    return np.stack([a, b], 1) + 1


def _prices(rng, n, wide_from=None):
    """v[0..2] = 1, 2, 1/2 (quotes against them are exact), the rest over [0.5, 2]; from `wide_from` on over 1e±6"""
    v = rng.uniform(0.5, 2.0, n)
    v[:3] = [1.0, 2.0, 0.5]
    if wide_from is not None:
        for j in range(wide_from, n):
            v[j] = _p10(rng.uniform(-6, 6))
    return v


def product_cases(rng):
    cases = {}
    n = 64
    v = _prices(rng, n, 32)
    v2 = v * (1.0 + rng.uniform(-0.05, 0.05, n))
    Rs, gs, As, cl = [], [], [], []

    def add(R, g, A, c):
        Rs.append(np.array(R, dtype=np.float64)), gs.append(float(g)), As.append(np.array(A)), cl.append(PCLASSES.index(c))

    for A in _pairs(rng, 500, 0, 32):
        add(rng.uniform(0.5, 2, 2), rng.choice([0.997, 1.0]), A, "well")
    for k in range(10, 53):                                       # the live test of either direction at 1 ± 2^-k
        for dir1 in (True, False):
            for sgn in (1, -1):
                for _ in range(2):
                    A = _pairs(rng, 1, 0, 32)[0]
                    g = float(rng.choice([0.997, 1.0, 0.9]))
                    R = rng.uniform(0.5, 2, 2)
                    v1, v2_ = _M(v[A[0] - 1]), _M(v[A[1] - 1])
                    e = 1 + sgn * mp.mpf(2) ** -k
                    if dir1:                                      # v₁R₁ = γ·v₂R₂·(1 ± 2^-k)
                        R[0] = _f(_M(g) * v2_ * _M(R[1]) * e / v1)
                    else:                                         # v₂R₂ = γ·v₁R₁·(1 ± 2^-k)
                        R[1] = _f(_M(g) * v1 * _M(R[0]) * e / v2_)
                    add(R, g, A, "band_edge")
    for _ in range(24):                                           # the no-fee parity point v₁R₁ = v₂R₂
        A = _pairs(rng, 1, 0, 32)[0]
        R = rng.uniform(0.5, 2, 2)
        R[0] = _f(_M(v[A[1] - 1]) * _M(R[1]) / _M(v[A[0] - 1]))
        add(R, 1.0, A, "band_edge")
    for _ in range(150):                                          # γ = 1 within 2^-40 of equilibrium
        A = _pairs(rng, 1, 0, 32)[0]
        R = rng.uniform(0.5, 2, 2)
        R[0] = _f(_M(v[A[1] - 1]) * _M(R[1]) / _M(v[A[0] - 1]) * (1 + mp.mpf(rng.uniform(-1, 1)) * mp.mpf(2) ** -40))
        add(R, 1.0, A, "gamma1")
    for i in range(200):                                          # γ > 1: both directions live for v₁R₁/(v₂R₂) in (1/γ, γ)
        A = _pairs(rng, 1, 0, 32)[0]
        g = [1.001, 1.02][i % 2]
        R = rng.uniform(0.5, 2, 2)
        if i % 5:
            t = mp.power(_M(g), mp.mpf(rng.uniform(-0.98, 0.98)))
            R[0] = _f(t * _M(v[A[1] - 1]) * _M(R[1]) / _M(v[A[0] - 1]))
        add(R, g, A, "both_live")
    for A in _pairs(rng, 450, 0, 64):
        add([_p10(rng.uniform(-9, 12)), _p10(rng.uniform(-9, 12))], rng.choice([0.5, 0.9, 0.997, 0.9999, 1.0]), A, "wide")
    cases["p_main"] = dict(v=v, v2=v2, R=np.array(Rs), gamma=np.array(gs), Ai=np.array(As), cls=np.array(cl, dtype=np.int8))
    # -- reserves beyond 2^±150 ----------------------------------------------------------------------
    n, m = 16, 150
    v = _prices(rng, n)
    R = np.array([[_p2(s * rng.uniform(151, 200)) for _ in range(2)] for s in rng.choice([-1, 1], m)])
    for i in range(0, m, 4):                                      # ... and pools with one reserve outside only
        R[i, 1] = rng.uniform(0.5, 2)
    Ai = _pairs(rng, m, 0, n)
    for i in range(1, m, 4):                                      # ... and pools near their equilibrium, so both sides matter
        R[i, 1] = _f(_M(v[Ai[i, 0] - 1]) * _M(R[i, 0]) / _M(v[Ai[i, 1] - 1]) * mp.mpf(rng.uniform(0.5, 2)))
    cases["p_resout"] = dict(v=v, R=R, gamma=rng.choice([0.997, 1.0], m), Ai=Ai,
                             cls=np.full(m, PCLASSES.index("res_out"), dtype=np.int8))
    # -- one price beyond 2^150 ------------------------------------------------------------------------
    v = _prices(rng, n)
    v[3] = _f(mp.mpf(2) ** 160 * mp.mpf("1.37"))
    Ai = _pairs(rng, m, 0, n)
    for i in range(0, m, 2):                                      # half the pools touch the out-of-window price
        Ai[i, rng.integers(0, 2)] = 4
        if Ai[i, 0] == Ai[i, 1]:
            Ai[i] = [4, 5]
    R = rng.uniform(0.5, 2.0, (m, 2))
    for i in range(0, m, 4):                                      # ... some of them near their equilibrium v₁R₁ = v₂R₂
        R[i, 0] = _p2(rng.uniform(-60, 60))
        R[i, 1] = _f(_M(v[Ai[i, 0] - 1]) * _M(R[i, 0]) / _M(v[Ai[i, 1] - 1]) * mp.mpf(rng.uniform(0.5, 2)))
    cases["p_pxout"] = dict(v=v, R=R, gamma=rng.choice([0.997, 1.0], m), Ai=Ai,
                            cls=np.full(m, PCLASSES.index("px_out"), dtype=np.int8))
    for c in cases.values():
        c["Ai"] = c["Ai"].astype(np.int32)
    return cases


class Ladders:
    """Collects UniV3 pools of one case.  A ladder is built around the target price: P = pr/γ (falling) or γ·pr (rising)
    is fixed by the pool's token pair, so the boundaries and the current price are placed relative to it."""

    def __init__(self, rng, v):
        self.rng, self.v = rng, v
        self.cp, self.g, self.A, self.cl, self.lt, self.lq = [], [], [], [], [], []

    def target(self, A, g, falling):
        pr = _M(self.v[A[0] - 1]) / _M(self.v[A[1] - 1])
        return pr / _M(g) if falling else _M(g) * pr

    @staticmethod
    def bounds(anchor, j, gaps):
        """nt + 1 boundaries, descending, bd[j] = anchor, bd[i]/bd[i+1] = 1 + gaps[i] (tick i spans (bd[i+1], bd[i]])"""
        nt = len(gaps)
        bd = [None] * (nt + 1)
        bd[j] = mp.mpf(anchor)
        for i in range(j - 1, -1, -1):
            bd[i] = bd[i + 1] * (1 + mp.mpf(gaps[i]))
        for i in range(j + 1, nt + 1):
            bd[i] = bd[i - 1] / (1 + mp.mpf(gaps[i - 1]))
        return bd

    def gaps(self, nt, lo=0.003, hi=0.08):
        return [float(x) for x in self.rng.uniform(lo, hi, nt)]

    def liq(self, nt, scale=1.0):
        return np.array([_p10(self.rng.uniform(2, 6)) * scale for _ in range(nt)])

    def add(self, cp, bd, lq, g, A, c, drop_top=False):
        lt = np.array([_f(x) for x in bd[:-1]])
        lq = np.array(lq, dtype=np.float64)
        if drop_top:                                              # the ladder's first tick was only scaffolding
            lt, lq = lt[1:], lq[1:]
        cp = _f(cp)
        assert np.all(np.diff(lt) < 0) and 0 < cp <= lt[0], (c, cp, lt)
        self.cp.append(cp), self.g.append(float(g)), self.A.append(np.array(A)), self.cl.append(UCLASSES.index(c))
        self.lt.append(lt), self.lq.append(lq)

    def generic(self, c, A, g, falling, depth, behind, beyond, gaps=None, lq=None, phi=None, psi=None, on_tick=False,
                scale=1.0, drop_top=False):
        """cp in tick c0, P in tick e = c0 ± depth; `behind` ticks on the far side of cp, `beyond` past the end tick.
        phi: where P sits in the end tick (0 = its upper boundary), psi: where cp sits in its tick likewise."""
        rng = self.rng
        nt = behind + depth + 1 + beyond
        gaps = self.gaps(nt) if gaps is None else gaps
        lq = self.liq(nt, scale) if lq is None else lq
        P = self.target(A, g, falling)
        e = behind + depth if falling else beyond
        c0 = e - depth if falling else e + depth
        phi = rng.uniform(0.1, 0.9) if phi is None else phi
        span = lambda i: mp.log(1 + mp.mpf(gaps[i]))
        bd = self.bounds(P * mp.exp(phi * span(e)), e, gaps)
        if on_tick:
            cp = bd[c0]
        elif depth == 0:
            t = rng.uniform(0.1, 0.9) if psi is None else psi
            cp = P * mp.exp(t * phi * span(e)) if falling else P * mp.exp(-t * (1 - phi) * span(e))
        else:
            psi = rng.uniform(0.05, 0.95) if psi is None else psi
            cp = bd[c0] * mp.exp(-psi * span(c0))
        self.add(cp, bd, lq, g, A, c, drop_top)

    def case(self, with_v2):
        off = np.zeros(len(self.cp) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in self.lt], out=off[1:])
        c = dict(v=self.v, cp=np.array(self.cp), gamma=np.array(self.g), Ai=np.array(self.A, dtype=np.int32),
                 tick_off=off, lower_ticks=np.concatenate(self.lt), liquidity=np.concatenate(self.lq),
                 cls=np.array(self.cl, dtype=np.int8))
        if with_v2:
            c["v2"] = self.v * (1.0 + self.rng.uniform(-0.03, 0.03, len(self.v)))
        return c


def univ3_main(rng):
    n = 64
    v = _prices(rng, n)
    for j in range(56, 60):                                       # quotes of 2^±130 between these and the next four
        v[j] = _f(mp.mpf(2) ** 65 * mp.mpf(rng.uniform(1, 2)))
        v[j + 4] = _f(mp.mpf(2) ** -65 * mp.mpf(rng.uniform(1, 2)))
    Lg = Ladders(rng, v)
    pair = lambda: _pairs(rng, 1, 0, 56)[0]
    gam = lambda: float(rng.choice([0.997, 1.0, 0.9995]))
    coin = lambda: bool(rng.integers(0, 2))
    for _ in range(150):
        Lg.generic("inside", pair(), gam(), coin(), 0, int(rng.integers(0, 6)), int(rng.integers(0, 6)))
    for i in range(240):                                          # 1-4 list ticks drained; list lengths 3, 4 and 5 among them
        depth = 1 + i % 4
        beyond = [3, 4, 5][i % 3] - depth if i < 120 and depth <= 3 else int(rng.integers(0, 7))
        Lg.generic("walk_head", pair(), gam(), coin(), depth, int(rng.integers(0, 4)), max(beyond, 0))
    for i in range(220):                                          # the walk ends at list position depth − 1
        depth = [5, 8, 9, 10][i % 4] if i < 80 else int(rng.integers(5, 41))
        Lg.generic("walk_deep", pair(), gam(), coin(), depth, int(rng.integers(0, 3)), int(rng.integers(0, 6)))
    for i in range(150):
        A, g, depth, behind = pair(), gam(), int(rng.integers(0, 7)), int(rng.integers(0, 3))
        nt = behind + depth + 1
        kind = i % 3
        if kind == 0:                                             # rising past lower_ticks[0]: the end tick is scaffolding
            gaps, lq = Lg.gaps(nt + 1), Lg.liq(nt + 1)
            P = Lg.target(A, g, False)
            bd = Lg.bounds(P / (1 + mp.mpf(rng.uniform(0.01, 0.3))), 1, gaps)   # lower_ticks[0] after the drop, below P
            c0 = 1 + depth
            cp = bd[c0] / (1 + mp.mpf(gaps[c0])) ** mp.mpf(rng.uniform(0.05, 0.95))
            Lg.add(cp, bd, lq, g, A, "drained_all", drop_top=True)
        else:                                                     # falling into the last tick: it reaches price 0, or it is empty
            lq = Lg.liq(nt)
            if kind == 2:
                lq[-1] = 0.0
            Lg.generic("drained_all", A, g, True, depth, behind, 0, lq=lq, phi=rng.uniform(0.2, 5.0))
    for k in range(20, 53):                                       # P = boundary·(1 ± 2^-k): head, inside and stop bands
        for sgn in (1, -1, 0):
            for falling in (True, False):
                for _ in range(2 if sgn else 1):
                    exact = sgn == 0
                    A = np.array([int(rng.integers(4, 56)), 1]) if exact else pair()      # quotes against v = 1 are exact
                    g = 1.0 if exact else gam()
                    P = Lg.target(A, g, falling)
                    depth, behind, beyond = int(rng.integers(0, 8)), int(rng.integers(0, 3)), int(rng.integers(1, 5))
                    nt = behind + depth + 1 + beyond
                    gaps, lq = Lg.gaps(nt), Lg.liq(nt)
                    B = _f(P / (1 + sgn * mp.mpf(2) ** -k))       # the boundary as the device receives it
                    # falling walks cross boundary j on leaving tick j − 1; rising ones on leaving tick j
                    j = behind + depth + 1 if falling else beyond
                    bd = Lg.bounds(_M(B), j, gaps)
                    c0 = j - 1 - depth if falling else j + depth
                    cp = bd[c0] / (1 + mp.mpf(gaps[c0])) ** mp.mpf(rng.uniform(0.05, 0.95))
                    Lg.add(cp, bd, lq, g, A, "on_boundary")
    for i in range(84):                                           # P exactly on a boundary and 1..3 ulps beside it: where the
        falling = bool(i % 2)                                     # drain test of one tick and the entry test of the next can disagree
        A, g = np.array([int(rng.integers(4, 56)), 1]), 1.0       # quotes against v = 1 are exact: P = v[A₁] as the device forms it
        B = float(v[A[0] - 1])
        for _ in range(abs(i % 7 - 3)):
            B = float(np.nextafter(B, np.inf if i % 7 > 3 else 0.0))
        depth, behind, beyond = int(rng.integers(0, 7)), int(rng.integers(0, 3)), int(rng.integers(1, 5))
        nt = behind + depth + 1 + beyond
        gaps, lq = Lg.gaps(nt), Lg.liq(nt)
        j = behind + depth + 1 if falling else beyond
        bd = Lg.bounds(_M(B), j, gaps)
        c0 = j - 1 - depth if falling else j + depth
        cp = bd[c0] / (1 + mp.mpf(gaps[c0])) ** mp.mpf(rng.uniform(0.05, 0.95))
        Lg.add(cp, bd, lq, g, A, "on_boundary")
    for i in range(160):                                          # cp on its own tick's upper boundary, the first included
        falling = bool(i % 2)
        behind = int(rng.integers(0, 4))
        if falling:                                               # cp = lower_ticks[behind]: `behind` = 0 is the first
            Lg.generic("cp_on_tick", pair(), gam(), True, int(rng.integers(0, 6)), behind, int(rng.integers(0, 3)), on_tick=True)
        elif i % 4 == 0:                                          # rising from cp = lower_ticks[0]: nothing above it to trade
            Lg.generic("cp_on_tick", pair(), float(rng.choice([0.9, 0.997, 1.0])), False, 1, behind, 0, on_tick=True,
                       drop_top=True)                             # (the end tick was scaffolding)
        else:                                                     # rising from its own tick's upper boundary: the tick is spent
            Lg.generic("cp_on_tick", pair(), float(rng.choice([0.9, 0.997, 1.0])), False, int(rng.integers(1, 6)), behind,
                       int(rng.integers(0, 3)), on_tick=True)
    for i in range(150):                                          # empty current tick; runs of 1-5 empty ticks in the walk
        depth, behind, beyond = int(rng.integers(2, 12)), int(rng.integers(0, 3)), int(rng.integers(0, 4))
        nt = behind + depth + 1 + beyond
        falling = coin()
        lq = Lg.liq(nt)
        c0 = behind if falling else beyond + depth
        step = 1 if falling else -1
        if i % 3 != 1:
            lq[c0] = 0.0
        if i % 3 != 0:
            run = 1 + i % 5
            start = int(rng.integers(1, max(2, depth - run + 2)))
            for r in range(run):
                if 0 <= c0 + step * (start + r) < nt:
                    lq[c0 + step * (start + r)] = 0.0
        Lg.generic("empty_cur", pair(), gam(), falling, depth, behind, beyond, lq=lq)
    for k in range(7, 17):                                        # spacing 1 + 2^-k (k = 13: about 1 bp)
        for _ in range(18):
            depth, behind, beyond = int(rng.integers(0, 31)), int(rng.integers(0, 3)), int(rng.integers(0, 4))
            nt = behind + depth + 1 + beyond
            Lg.generic("narrow", pair(), gam(), coin(), depth, behind, beyond, gaps=[2.0 ** -k] * nt)
    for k in range(10, 53, 2):                                    # pr at γ·cp and cp/γ, times (1 ± 2^-k)
        for sgn in (1, -1):
            for lower in (True, False):
                A, g = pair(), float(rng.choice([0.997, 0.9995, 0.9]))
                pr = _M(v[A[0] - 1]) / _M(v[A[1] - 1])
                e = 1 + sgn * mp.mpf(2) ** -k
                cp = _M(_f(pr / (_M(g) * e) if lower else pr * _M(g) / e))
                behind, beyond = int(rng.integers(0, 4)), int(rng.integers(0, 4))
                gaps = Lg.gaps(behind + 1 + beyond, 0.2, 0.5)     # wider than the fee: cp well inside its tick
                bd = Lg.bounds(cp * (1 + mp.mpf(gaps[behind])) ** mp.mpf(rng.uniform(0.4, 0.6)), behind, gaps)
                Lg.add(cp, bd, Lg.liq(len(gaps)), g, A, "band")
    for i in range(200):
        g = [1.0, 1.0 - 2.0 ** -52, 0.997, 0.3][i % 4]
        Lg.generic("gamma", pair(), g, coin(), int(rng.integers(0, 7)), int(rng.integers(0, 3)), int(rng.integers(0, 4)))
    for i in range(150):                                          # quotes of 2^±130, liquidity scaled by 2^±100
        a = 57 + int(rng.integers(0, 4))
        A = np.array([a, a + 4] if i % 2 else [a + 4, a])
        Lg.generic("wide", A, gam(), coin(), int(rng.integers(0, 9)), int(rng.integers(0, 3)), int(rng.integers(0, 4)),
                   scale=2.0 ** (100 if i % 4 < 2 else -100))
    return Lg.case(True)


def univ3_resout(rng):
    v = _prices(rng, 16)
    Lg = Ladders(rng, v)
    for i in range(150):
        Lg.generic("res_out", _pairs(rng, 1, 0, 16)[0], float(rng.choice([0.997, 1.0])), bool(i % 2), int(rng.integers(0, 9)),
                   int(rng.integers(0, 3)), int(rng.integers(0, 4)), scale=2.0 ** (200 if i % 4 < 2 else -200))
    return Lg.case(False)


def bounded_case(rng):
    """Two-tick pools whose second tick is empty: lower_ticks = [p_upper, p_lower], liquidity = [k, 0]."""
    v = _prices(rng, 16)
    Lg = Ladders(rng, v)
    pair = lambda: _pairs(rng, 1, 0, 16)[0]
    gam = lambda: float(rng.choice([0.997, 1.0, 0.9995]))

    def put(c, A, g, cp, hi, lo):
        Lg.add(cp, [mp.mpf(hi), mp.mpf(lo), None], [_p10(rng.uniform(2, 6)), 0.0], g, A, c)

    for i in range(150):                                          # P and cp both inside (p_lower, p_upper]
        A, g, falling = pair(), gam(), bool(i % 2)
        P = Lg.target(A, g, falling)
        w = mp.mpf(rng.uniform(0.02, 0.3))
        cp = P * (1 + w) if falling else P / (1 + w)
        put("inside", A, g, cp, max(P, cp) * (1 + mp.mpf(rng.uniform(0.01, 0.3))), min(P, cp) / (1 + mp.mpf(rng.uniform(0.01, 0.3))))
    for i in range(120):                                          # P beyond the interval
        A, g, falling = pair(), gam(), bool(i % 2)
        P = Lg.target(A, g, falling)
        w, x, y = (mp.mpf(rng.uniform(0.01, 0.3)) for _ in range(3))
        if falling:
            lo = P * (1 + w)
            cp = lo * (1 + x)
            put("drained_all", A, g, cp, cp * (1 + y), lo)
        else:
            hi = P / (1 + w)
            cp = hi / (1 + x)
            put("drained_all", A, g, cp, hi, cp / (1 + y))
    for k in range(10, 53, 2):
        for sgn in (1, -1):
            for lower in (True, False):
                A, g = pair(), float(rng.choice([0.997, 0.9995, 0.9]))
                pr = _M(v[A[0] - 1]) / _M(v[A[1] - 1])
                e = 1 + sgn * mp.mpf(2) ** -k
                cp = _M(_f(pr / (_M(g) * e) if lower else pr * _M(g) / e))
                put("band", A, g, cp, cp * mp.mpf(rng.uniform(1.2, 1.5)), cp / mp.mpf(rng.uniform(1.2, 1.5)))
    for i in range(120):                                          # cp = p_upper (its own tick), or p_lower (the empty tick's)
        A, g, falling = pair(), float(rng.choice([0.9, 0.997, 1.0])), bool(i % 2)
        P = Lg.target(A, g, falling)
        w, x = (mp.mpf(rng.uniform(0.01, 0.3)) for _ in range(2))
        if i % 4 < 2:
            hi = P * (1 + w) if falling else P / (1 + w)          # rising from p_upper: nothing to trade
            put("cp_on_tick", A, g, hi, hi, hi / (1 + w) / (1 + x))
        else:
            lo = P * (1 + w) if falling else P / (1 + w)          # falling from p_lower: nothing to trade
            put("cp_on_tick", A, g, lo, lo * (1 + w) * (1 + x), lo)
    for k in range(7, 17):                                        # p_upper / p_lower = 1 + 2^-k
        for i in range(12):
            A, g, falling = pair(), gam(), bool(i % 2)
            P = Lg.target(A, g, falling)
            s = mp.mpf(2) ** -k
            t, q = mp.mpf(rng.uniform(0.05, 0.95)), mp.mpf(rng.uniform(0.0, 1.5))
            if i % 3 == 2:                                        # P beyond the narrow interval
                cp = P * (1 + s) ** (1 + q) if falling else P / (1 + s) ** (1 + q)
                hi = cp * (1 + s) ** t
            else:
                cp = P * (1 + s) ** (t * mp.mpf(0.9)) if falling else P / (1 + s) ** (t * mp.mpf(0.9))
                hi = max(cp, P) * (1 + s) ** ((1 - t) * mp.mpf(0.9))
            put("narrow", A, g, cp, hi, hi / (1 + s))
    return Lg.case(False)


# ---- rows, checks, output -----------------------------------------------------------------------------------------

def product_rows(c):
    m = len(c["gamma"])
    D, L, Z = np.empty((m, 2)), np.empty((m, 2)), np.zeros((m, 2), dtype=bool)
    for i in range(m):
        vv = c["v"][c["Ai"][i] - 1]
        d1, d2, l1, l2 = prod_truth(c["R"][i], c["gamma"][i], vv)
        D[i] = _f(d1), _f(d2)
        L[i] = _f(l1), _f(l2)
        Z[i] = prod_clear(c["R"][i], c["gamma"][i], vv)
        assert not (Z[i, 0] and (d1 or l2)) and not (Z[i, 1] and (d2 or l1))
    return D, L, Z


def pool_ticks(c, i):
    o, e = c["tick_off"][i], c["tick_off"][i + 1]
    return c["lower_ticks"][o:e], c["liquidity"][o:e]


def univ3_rows(c):
    m = len(c["gamma"])
    D, L, Z = np.empty((m, 2)), np.empty((m, 2)), np.zeros(m, dtype=bool)
    for i in range(m):
        lt, lq = pool_ticks(c, i)
        vv = c["v"][c["Ai"][i] - 1]
        d1, d2, l1, l2 = v3_truth(c["cp"][i], lt, lq, c["gamma"][i], vv)
        D[i] = _f(d1), _f(d2)
        L[i] = _f(l1), _f(l2)
        Z[i] = v3_clear(c["cp"][i], c["gamma"][i], vv)
    return D, L, Z


def _agree(a, b, scale, what):
    for x, y in zip(a, b):
        assert abs(x - y) <= mp.mpf(10) ** -40 * scale, (what, a, b)


def check_product(c, rng, count):
    for i in rng.choice(len(c["gamma"]), count, replace=False):
        vv = c["v"][c["Ai"][i] - 1]
        a, b = prod_truth(c["R"][i], c["gamma"][i], vv), prod_kkt(c["R"][i], c["gamma"][i], vv)
        _agree(a, b, max(_M(x) for x in c["R"][i]) + max(a), ("product", int(i)))


def check_univ3(c, rng, count):
    for i in rng.choice(len(c["gamma"]), count, replace=False):
        lt, lq = pool_ticks(c, i)
        vv = c["v"][c["Ai"][i] - 1]
        a, b = v3_truth(c["cp"][i], lt, lq, c["gamma"][i], vv), v3_forward(c["cp"][i], lt, lq, c["gamma"][i], vv)
        cp = _M(c["cp"][i])
        scale = max(a) + mp.fsum(mp.sqrt(_M(k)) * (mp.sqrt(cp) + 1 / mp.sqrt(cp)) for k in lq)
        _agree(a, b, scale, ("univ3", int(i)))


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same bytes on every run"""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    rng = np.random.default_rng(20261017)
    pcases = product_cases(rng)
    ucases = dict(u_main=univ3_main(rng), u_resout=univ3_resout(rng), bounded=bounded_case(rng))
    out = dict(pcases=np.array(sorted(pcases)), ucases=np.array(sorted(ucases)), pclasses=np.array(PCLASSES),
               uclasses=np.array(UCLASSES))
    for name, c in pcases.items():
        c["D"], c["L"], c["zclear"] = product_rows(c)
        out.update({f"{name}_{k}": a for k, a in c.items()})
    for name, c in ucases.items():
        c["D"], c["L"], c["zclear"] = univ3_rows(c)
        out.update({f"{name}_{k}": a for k, a in c.items()})
    chk = np.random.default_rng(7)
    check_product(pcases["p_main"], chk, 250)
    check_product(pcases["p_resout"], chk, 25)
    check_product(pcases["p_pxout"], chk, 25)
    check_univ3(ucases["u_main"], chk, 250)
    check_univ3(ucases["u_resout"], chk, 25)
    check_univ3(ucases["bounded"], chk, 60)
    save(OUT, out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {sum(len(c['gamma']) for c in pcases.values())} product pools, "
          f"{sum(len(c['gamma']) for c in ucases.values())} UniV3 pools, {sum(len(c['liquidity']) for c in ucases.values())} ticks")


if __name__ == "__main__":
    main()
