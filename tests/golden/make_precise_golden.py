"""Regenerates tests/golden/precise.npz: GeometricMeanTwoCoin and N-coin weighted trades to 60 significant digits.

    python tests/golden/make_precise_golden.py

Inputs are float64 exactly as the device receives them (R, w, γ, 1-based Ai, v); every truth is computed from those
float64 values taken as exact, in mpmath at 60 digits, and rounded ONCE to float64.  Nothing here calls libm: an input
built near a threshold is constructed in mpmath and then rounded, so the file is the same on every host.

Two-coin truth: the closed forms of src/cfmms.jl:180-196 (geom_arb_δ / geom_arb_λ, all four of them, as the reference
evaluates them), in log space so that nothing overflows.  A few hundred pools are checked against an independent KKT
solve (bisection on the tendered side's reserve ratio); the two must agree to 40 digits or the script fails.

Weighted truth: the root t* of the piecewise-linear G(t) of tests/weighted_ref.py, solved exactly -- sort the 2N
breakpoints, find the segment that holds the root, one linear solve -- and trades R·expm1(·).  N = 2 is cross-checked
against the two-coin closed forms.

Cases (`gcases` / `wcases` list their names; arrays are `<case>_<field>`):
  two-coin  g_well   n = 64, v in [0.5, 2]: classes well / both_live (γ > 1) / band_edge (c/R = 1 ± 2^-k, k = 10..52) /
                     eq_gamma1 (γ = 1, within 2^-40 of equilibrium); also v2, the prices of the update test
            g_wide   n = 64, v over 1e±6: classes wide / overflow (η·|log₁₀ R| > 308 for some power the reference takes)
            g_resout n = 16: reserves beyond 2^±150 (fast_ok = 0)
            g_pxout  n = 16: one price beyond 2^150
  weighted  w_N      N = 2..8, n = 32: classes well / wide / gamma1 / ties / on_bp / near_bp / band; w_3 also has v2
"""
import os

import mpmath as mp
import numpy as np

DPS = 60
mp.mp.dps = DPS
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "precise.npz")

GCLASSES = ["well", "both_live", "band_edge", "eq_gamma1", "wide", "overflow", "res_out", "px_out"]
WCLASSES = ["well", "wide", "gamma1", "ties", "on_bp", "near_bp", "band"]


def _f(x):
    """mpf -> the nearest float64 (ties to even): the one rounding of every stored value."""
    return mp.libmp.to_float(mp.mpf(x)._mpf_, rnd=mp.libmp.round_nearest)


def _M(x):
    return mp.mpf(float(x))


# ---- truth ------------------------------------------------------------------------------------------------------

def geo_direction(m, r1, r2, eta, g):
    """(geom_arb_δ(m, r1, r2, η, γ), geom_arb_λ(m, r1, r2, η, γ)) of src/cfmms.jl:180-181, in log space: the tendered
    side r2 ends at X = (γ·m·η·r1·r2^η)^(1/(η+1)), the received side r1 at Y = ((r2·r1^(1/η))/(η·γ·m))^(η/(1+η))."""
    lX = (mp.log(g) + mp.log(m) + mp.log(eta) + mp.log(r1) + eta * mp.log(r2)) / (eta + 1)
    lY = (mp.log(r2) + mp.log(r1) / eta - mp.log(eta) - mp.log(g) - mp.log(m)) * (eta / (1 + eta))
    d = mp.exp(lX) - r2
    lam = r1 - mp.exp(lY)
    return (d / g if d > 0 else mp.mpf(0)), (lam if lam > 0 else mp.mpf(0))


def geo_truth(R, w, g, v):
    """find_arb! of one GeometricMeanTwoCoin pool (src/cfmms.jl:184-196) from float64 inputs taken as exact
    -> (Δ₁, Δ₂, Λ₁, Λ₂) as mpf."""
    R1, R2, w1, w2, g, v1, v2 = (_M(x) for x in (R[0], R[1], w[0], w[1], g, v[0], v[1]))
    eta = w1 / w2
    d1, l2 = geo_direction(v2 / v1, R2, R1, eta, g)        # :190, :194
    d2, l1 = geo_direction(v1 / v2, R1, R2, 1 / eta, g)    # :191, :193
    return d1, d2, l1, l2


def geo_kkt(R, w, g, v):
    """Independent check of geo_truth: the KKT conditions of the find_arb! problem, solved by bisection.  Direction 1
    tenders coin 1: X = ρ·R₁ (ρ >= 1), the invariant gives Y = R₂·ρ^(−η), and optimality is the pool's marginal price
    η·Y/X equal to v₁/(γ·v₂); h(ρ) = log(η·Y/X) − log(v₁/(γ·v₂)) decreases in ρ.  Direction 2 likewise."""
    R1, R2, w1, w2, g, v1, v2 = (_M(x) for x in (R[0], R[1], w[0], w[1], g, v[0], v[1]))
    out = []
    for rb, ra, eta, vb, va in ((R1, R2, w1 / w2, v1, v2), (R2, R1, w2 / w1, v2, v1)):
        target = mp.log(vb / (g * va))
        h = lambda lr: mp.log(eta) + mp.log(ra) - eta * lr - mp.log(rb) - lr - target   # in lr = log ρ
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
        lr = (lo + hi) / 2
        out.append(((rb * mp.exp(lr) - rb) / g, ra - ra * mp.exp(-eta * lr)))
    (d1, l2), (d2, l1) = out
    return d1, d2, l1, l2


def weighted_truth(R, w, g, v):
    """Exact root of G(t) = Σ w_k [min(0, t − s_k^λ) + max(0, t − s_k^δ)] (normalised w) and the trades
    -> (Δ[N], Λ[N]) as mpf lists."""
    N = len(R)
    Rm, wm, vm, gm = [_M(x) for x in R], [_M(x) for x in w], [_M(x) for x in v], _M(g)
    ws = mp.fsum(wm)
    wn = [x / ws for x in wm]
    lg = mp.log(gm)
    sl = [mp.log(Rm[k]) + mp.log(vm[k]) - mp.log(wn[k]) for k in range(N)]
    sd = [s - lg for s in sl]
    zero = [mp.mpf(0)] * N
    if max(sl) <= min(sd):
        return zero, list(zero)
    G = lambda t: mp.fsum(wn[k] * (min(mp.mpf(0), t - sl[k]) + max(mp.mpf(0), t - sd[k])) for k in range(N))
    bps = sorted(sl + sd)
    Gs = [G(b) for b in bps]
    t = None
    for b, Gb in zip(bps, Gs):
        if Gb == 0:
            t = b
            break
    if t is None:
        if Gs[0] > 0:
            t = bps[0] - Gs[0] / mp.fsum(wn)             # below every breakpoint: every λ term live
        elif Gs[-1] < 0:
            t = bps[-1] - Gs[-1] / mp.fsum(wn)           # above every breakpoint: every δ term live
        else:
            j = max(i for i in range(len(bps)) if Gs[i] < 0)
            lo, hi = bps[j], bps[j + 1]
            mid = (lo + hi) / 2
            slope = mp.fsum((wn[k] if mid < sl[k] else 0) + (wn[k] if mid > sd[k] else 0) for k in range(N))
            t = lo - Gs[j] / slope
    D = [Rm[k] * mp.expm1(t - sd[k]) / gm if t > sd[k] else mp.mpf(0) for k in range(N)]
    L = [-Rm[k] * mp.expm1(t - sl[k]) if t < sl[k] else mp.mpf(0) for k in range(N)]
    return D, L


def geo_rows(R, w, g, Ai, v):
    """Truth of every pool of a two-coin case, rounded once -> (Δ [m, 2], Λ [m, 2])."""
    m = len(g)
    D, L = np.empty((m, 2)), np.empty((m, 2))
    for i in range(m):
        d1, d2, l1, l2 = geo_truth(R[i], w[i], g[i], v[Ai[i] - 1])
        D[i] = _f(d1), _f(d2)
        L[i] = _f(l1), _f(l2)
    return D, L


def weighted_rows(R, w, g, Ai, v):
    m, N = R.shape
    D, L = np.empty((m, N)), np.empty((m, N))
    for i in range(m):
        d, lam = weighted_truth(R[i], w[i], g[i], v[Ai[i] - 1])
        D[i] = [_f(x) for x in d]
        L[i] = [_f(x) for x in lam]
    return D, L


# ---- inputs -----------------------------------------------------------------------------------------------------

def _pairs(rng, m, n, lo=0, hi=None):
    hi = n if hi is None else hi
    a = rng.integers(lo, hi, m)
    b = rng.integers(lo, hi - 1, m)
    b = b + (b >= a)
    return np.stack([a, b], 1) + 1


def _c_over(dir1, R, w, g, v1, v2):
    """c of the live-direction test (the pow-free factor of :180) in mpmath: direction 1 trades iff c > R₁,
    c = γ·(v₂/v₁)·η·R₂; direction 2 iff c > R₂, c = γ·(v₁/v₂)·R₁/η."""
    eta = _M(w[0]) / _M(w[1])
    if dir1:
        return _M(g) * (_M(v2) / _M(v1)) * eta * _M(R[1])
    return _M(g) * (_M(v1) / _M(v2)) * _M(R[0]) / eta


def two_coin_cases(rng):
    cases = {}
    # -- g_well ------------------------------------------------------------------------------------
    n = 64
    v = rng.uniform(0.5, 2.0, n)
    v2 = v * np.exp(rng.uniform(-0.05, 0.05, n))
    Rs, ws, gs, As, cl = [], [], [], [], []

    def add(R, w, g, A, c):
        Rs.append(R), ws.append(w), gs.append(g), As.append(A), cl.append(GCLASSES.index(c))

    m = 2000
    for R, w1, g, A in zip(rng.uniform(0.5, 2, (m, 2)), rng.uniform(1 / 3, 2 / 3, m), rng.choice([0.997, 1.0], m),
                           _pairs(rng, m, n)):
        add(R, np.array([w1, 1.0 - w1]), g, A, "well")            # η = w₁/(1 − w₁) in [0.5, 2]
    for i, A in enumerate(_pairs(rng, 500, n)):                   # γ > 1: both directions live for ρ in (1, γ²)
        g = [1.001, 1.02][i % 2]
        w = np.array([rng.uniform(1 / 3, 2 / 3), 0.0])
        w[1] = 1.0 - w[0]
        R = rng.uniform(0.5, 2, 2)
        if i % 5:
            rho = mp.mpf(1) + (_M(g) ** 2 - 1) * _M(rng.uniform(0.01, 0.99))
            R[0] = _f(_c_over(True, R, w, g, *v[A - 1]) / rho)
        add(R, w, g, A, "both_live")
    for k in range(10, 53):                                       # c/R = 1 ± 2^-k in either direction
        for dir1 in (True, False):
            for sgn in (1, -1):
                for _ in range(4):
                    A = _pairs(rng, 1, n)[0]
                    w = np.array([rng.uniform(1 / 3, 2 / 3), 0.0])
                    w[1] = 1.0 - w[0]
                    g = float(rng.choice([0.997, 1.0]))
                    R = rng.uniform(0.5, 2, 2)
                    c = _c_over(dir1, R, w, g, *v[A - 1])
                    R[0 if dir1 else 1] = _f(c / (1 + sgn * mp.mpf(2) ** -k))
                    add(R, w, g, A, "band_edge")
    for i in range(300):                                          # γ = 1 within 2^-40 of equilibrium: GeoMeanOps' margin
        A = _pairs(rng, 1, n)[0]
        w = np.array([rng.uniform(1 / 3, 2 / 3), 0.0])
        w[1] = 1.0 - w[0]
        R = rng.uniform(0.5, 2, 2)
        c = _c_over(True, R, w, 1.0, *v[A - 1])
        R[0] = _f(c * (1 + mp.mpf(rng.uniform(-1, 1)) * mp.mpf(2) ** -40))
        add(R, w, 1.0, A, "eq_gamma1")
    cases["g_well"] = dict(v=v, v2=v2, R=np.array(Rs), w=np.array(ws), gamma=np.array(gs), Ai=np.array(As),
                           cls=np.array(cl, dtype=np.int8))
    # -- g_wide ------------------------------------------------------------------------------------
    v = 10.0 ** rng.uniform(-6, 6, n)
    Rs, ws, gs, As, cl = [], [], [], [], []
    m = 2000
    for R, w1, g, A in zip(10.0 ** rng.uniform(-6, 6, (m, 2)), rng.uniform(0.01, 0.99, m),
                           rng.choice([0.5, 0.9, 0.997, 0.9999, 1.0], m), _pairs(rng, m, n)):
        add(R, np.array([w1, 1.0 - w1]), g, A, "wide")
    got = 0
    while got < 300:                                              # η·|log₁₀ R| > 308: the reference's r^η leaves float64
        w1 = rng.uniform(0.9, 0.995) if got % 2 else rng.uniform(0.005, 0.1)
        R = 10.0 ** rng.uniform(-6, 6, 2)
        eta = w1 / (1.0 - w1)
        if max(eta, 1 / eta) * np.max(np.abs(np.log10(R))) <= 330:
            continue
        add(R, np.array([w1, 1.0 - w1]), float(rng.choice([0.9, 0.997, 1.0])), _pairs(rng, 1, n)[0], "overflow")
        got += 1
    cases["g_wide"] = dict(v=v, R=np.array(Rs), w=np.array(ws), gamma=np.array(gs), Ai=np.array(As),
                           cls=np.array(cl, dtype=np.int8))
    # -- g_resout: reserves beyond 2^±150 -----------------------------------------------------------
    n, m = 16, 200
    v = rng.uniform(0.5, 2.0, n)
    R = 2.0 ** (rng.uniform(151, 200, (m, 2)) * rng.choice([-1, 1], (m, 1)))
    R[::4, 1] = rng.uniform(0.5, 2, m)[::4]                      # ... and pools with one reserve outside only
    w1 = rng.uniform(0.2, 0.8, m)
    cases["g_resout"] = dict(v=v, R=R, w=np.stack([w1, 1.0 - w1], 1), gamma=rng.choice([0.997, 1.0], m),
                             Ai=_pairs(rng, m, n), cls=np.full(m, GCLASSES.index("res_out"), dtype=np.int8))
    # -- g_pxout: one price beyond 2^150 --------------------------------------------------------------
    v = rng.uniform(0.5, 2.0, n)
    v[3] = 2.0 ** 160 * 1.37
    Ai = _pairs(rng, m, n)
    Ai[::2, rng.integers(0, 2)] = 4                               # half the pools touch the out-of-window price
    Ai[::2] = np.where(Ai[::2, :1] == Ai[::2, 1:], [[4, 5]], Ai[::2])
    R = 2.0 ** rng.uniform(100, 140, (m, 2))                      # the equilibrium reserves of that token are ~2^±160
    R[1::2] = rng.uniform(0.5, 2.0, (m - m // 2, 2))
    w1 = rng.uniform(0.2, 0.8, m)
    cases["g_pxout"] = dict(v=v, R=R, w=np.stack([w1, 1.0 - w1], 1), gamma=rng.choice([0.997, 1.0], m), Ai=Ai,
                            cls=np.full(m, GCLASSES.index("px_out"), dtype=np.int8))
    for c in cases.values():
        c["Ai"] = c["Ai"].astype(np.int32)
    return cases


def _distinct(rng, N, lo, hi):
    return rng.choice(np.arange(lo, hi), N, replace=False) + 1


def weighted_case(rng, N, with_v2):
    n = 32
    v = np.concatenate([rng.uniform(0.5, 2.0, 16), 10.0 ** rng.uniform(-6, 6, 16)])
    Rs, ws, gs, As, cl = [], [], [], [], []

    def add(R, w, g, A, c):
        Rs.append(np.asarray(R, dtype=np.float64)), ws.append(np.asarray(w, dtype=np.float64)), gs.append(float(g))
        As.append(A), cl.append(WCLASSES.index(c))

    def build_R(A, w, s):
        """R_k = wn_k·e^{s_k}/v_k in mpmath, rounded: s_k = log(R_k v_k/wn_k) up to that one rounding."""
        ws_ = mp.fsum(_M(x) for x in w)
        return np.array([_f(_M(w[k]) / ws_ * mp.exp(s[k]) / _M(v[A[k] - 1])) for k in range(N)])

    for _ in range(100):
        add(rng.uniform(0.5, 2, N), rng.uniform(0.5, 2, N), rng.choice([0.997, 1.0]), _distinct(rng, N, 0, 16), "well")
    for _ in range(80):
        add(10.0 ** rng.uniform(-6, 6, N), rng.uniform(0.01, 1.0, N), rng.choice([0.5, 0.9, 0.997, 0.9999, 1.0]),
            _distinct(rng, N, 0, 32), "wide")
    for _ in range(40):
        add(10.0 ** rng.uniform(-2, 2, N), rng.uniform(0.1, 1.0, N), 1.0, _distinct(rng, N, 0, 32), "gamma1")
    for _ in range(30):                                           # tied log(R_k v_k/w_k): two or more coins share s
        A, w, g = _distinct(rng, N, 0, 32), rng.uniform(0.1, 1.0, N), rng.choice([0.997, 1.0])
        s = [mp.mpf(rng.uniform(-3, 3)) for _ in range(N)]
        tied = rng.choice(N, rng.integers(2, N + 1), replace=False)
        for k in tied:
            s[k] = s[tied[0]]
        add(build_R(A, w, s), w, g, A, "ties")
    for near in (False, True):                                    # t* on (or 2^-k next to) a breakpoint: coin j at its band edge
        for _ in range(30):
            A, w = _distinct(rng, N, 0, 32), rng.uniform(0.1, 1.0, N)
            g = float(rng.choice([0.99, 0.997, 1.0]))
            lg = mp.log(_M(g))
            wn = [_M(x) / mp.fsum(_M(y) for y in w) for x in w]
            j, i = rng.choice(N, 2, replace=False)
            s = [mp.mpf(rng.uniform(-2, 2)) for _ in range(N)]
            t = s[j] - (lg if rng.integers(0, 2) else 0)              # on coin j's λ or δ breakpoint
            off = mp.mpf(2) ** -int(rng.integers(20, 46)) * (1 if rng.integers(0, 2) else -1) if near else 0
            t = t + off
            Gx = mp.fsum(wn[k] * (min(mp.mpf(0), t - s[k]) + max(mp.mpf(0), t - (s[k] - lg))) for k in range(N) if k != i)
            # coin i closes G(t) = 0: λ side (s_i above t) if the others sum positive, δ side otherwise
            s[i] = t + Gx / wn[i] if Gx > 0 else t + Gx / wn[i] + lg
            add(build_R(A, w, s), w, g, A, "near_bp" if near else "on_bp")
    for _ in range(20):                                           # inside the fee band: no trade at all
        A, w, g = _distinct(rng, N, 0, 32), rng.uniform(0.1, 1.0, N), float(rng.choice([0.99, 0.997]))
        S = rng.uniform(-2, 2)
        span = -0.8 * np.log(g)
        add(build_R(A, w, [mp.mpf(S + rng.uniform(0, span)) for _ in range(N)]), w, g, A, "band")
    c = dict(v=v, R=np.array(Rs), w=np.array(ws), gamma=np.array(gs), Ai=np.array(As, dtype=np.int32),
             cls=np.array(cl, dtype=np.int8))
    if with_v2:
        c["v2"] = v * np.exp(rng.uniform(-0.05, 0.05, n))
    return c


# ---- checks the generator makes before it writes ----------------------------------------------------------------

def check_kkt(c, rng, count):
    for i in rng.choice(len(c["gamma"]), count, replace=False):
        a = geo_truth(c["R"][i], c["w"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
        b = geo_kkt(c["R"][i], c["w"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
        scale = max(_M(x) for x in c["R"][i]) + max(max(a), max(b))
        for x, y in zip(a, b):
            assert abs(x - y) <= mp.mpf(10) ** -40 * scale, (i, a, b)


def check_weighted_two_coin(c):
    for i in range(len(c["gamma"])):
        if c["gamma"][i] > 1:
            continue
        D, L = weighted_truth(c["R"][i], c["w"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
        d1, d2, l1, l2 = geo_truth(c["R"][i], c["w"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
        scale = max(_M(x) for x in c["R"][i]) + max(D + L)
        for x, y in zip(D + L, (d1, d2, l1, l2)):
            assert abs(x - y) <= mp.mpf(10) ** -40 * scale, (i, D, L, (d1, d2, l1, l2))


def main():
    rng = np.random.default_rng(20261016)
    gcases = two_coin_cases(rng)
    wcases = {f"w_{N}": weighted_case(rng, N, N == 3) for N in range(2, 9)}
    out = dict(gcases=np.array(sorted(gcases)), wcases=np.array(sorted(wcases)), gclasses=np.array(GCLASSES),
               wclasses=np.array(WCLASSES))
    for name, c in gcases.items():
        c["D"], c["L"] = geo_rows(c["R"], c["w"], c["gamma"], c["Ai"], c["v"])
        out.update({f"{name}_{k}": a for k, a in c.items()})
    for name, c in wcases.items():
        c["D"], c["L"] = weighted_rows(c["R"], c["w"], c["gamma"], c["Ai"], c["v"])
        out.update({f"{name}_{k}": a for k, a in c.items()})
    chk = np.random.default_rng(7)
    check_kkt(gcases["g_well"], chk, 150)
    check_kkt(gcases["g_wide"], chk, 150)
    check_kkt(gcases["g_resout"], chk, 25)
    check_kkt(gcases["g_pxout"], chk, 25)
    # N = 2 against the two-coin closed forms (as a two-coin pool: R, w, γ, v in coin order)
    check_weighted_two_coin(wcases["w_2"])
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {sum(len(c['gamma']) for c in gcases.values())} two-coin pools, "
          f"{sum(len(c['gamma']) for c in wcases.values())} weighted pools")


if __name__ == "__main__":
    main()
