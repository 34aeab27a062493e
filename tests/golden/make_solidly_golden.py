"""Regenerates tests/golden/solidly_precise.npz: trades of Solidly-style stable pairs (φ = x³y + xy³) to 60 significant
digits, with the conditioning of every trade.

    python tests/golden/make_solidly_golden.py [processes]

Inputs are float64 exactly as the device receives them (R, γ, 1-based Ai, v); every truth is computed from those float64
values taken as exact, in mpmath at 80 digits, and rounded ONCE to float64.  Nothing that decides a stored value calls
libm: an input built near a threshold is constructed in mpmath and then rounded.  (The random draws use numpy, as
tests/golden/make_precise_golden.py does.)

Truth, by a method that does not know the closed form.  The direction is the sign of the marginal gain at zero
(γ·v_b·φ_a − v_a·φ_b at R, exact rational arithmetic in mpmath).  In the frame of the tendered coin a and the received
coin b the KKT system in (x′, y′) is   φ(x′, y′) = φ(R),   φ_a(x′, y′)/φ_b(x′, y′) = π = v_a/(γ·v_b).
φ is homogeneous, so the second equation is one equation p(t) = t(3 + t²)/(1 + 3t²) = π in t = y′/x′, p increasing with
p(t)/t in [1/3, 3]: t is found by BISECTION on [π/3, 3π] down to a relative width of 1e-70, and the first equation then
gives x′ = (φ(R)/(t(1 + t²)))^¼ (φ(R) is formed in mpmath, where it cannot overflow), y′ = t·x′;
Δ_a = (x′ − r_a)/γ, Λ_b = r_b − y′.

Self-checks (the script fails before it writes if one fails), per pool: both KKT equations at (x′, y′) to 1e-60
relative; t against the closed form (1 + c)/(1 − c), c = cbrt((π − 1)/(π + 1)), to 50 digits; x′ >= r_a and y′ <= r_b.

Conditioning (stored as cd, cl, float64): Σ_j |x_j·∂T/∂x_j| over the five inputs R₁, R₂, γ, v₁, v₂, by central
differences at a relative step of 1e-20 (γ: one-sided, downwards, since γ <= 1), the perturbed trades by the closed form
that the self-check has just tied to the truth.  A pool whose perturbation crosses the band edge contributes the
one-sided slope.

One case, n = 48 tokens: 0..7 "stable" prices (1 ± 10^U[−6, −3]), 8..15 e^U[−0.5, 0.5], 16..47 e^U[−40, 40].
Classes (CLASSES), ROWS pools each:
  well       tokens 0..15, R₁ = 10^U[0, 6], t₀ = R₂/R₁ = e^U[−0.5, 0.5], γ in {0.9999, 0.9995, 0.997}
  balanced   t₀ = 1 exactly (half) or within 1e-9 of it; γ in {1, 0.9995}
  band_edge  R₂ built so that the price sits on a band limit (either side), then moved by −3..3 ulps
  band       strictly inside the band (p(t₀) = (v₁/v₂)·γ^s, |s| <= 0.9, γ < 1): the truth is +0.0
  gamma1     γ = 1
  low_gamma  γ = U[0.5, 0.9], t₀ = e^U[−3, 3]
  wide       tokens 16..47, t₀ = e^U[−40, 40]
  range      each reserve at an end of the upload range: 2^-150·(1 + U) or 2^149·(1 + U)
  drain      token pairs whose price ratio leaves less than 1e-12 of the received reserve
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

DPS = 80
mp.mp.dps = DPS
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "solidly_precise.npz")

CLASSES = ["well", "balanced", "band_edge", "band", "gamma1", "low_gamma", "wide", "range", "drain"]
ROWS = 1200
NT = 48
HSTEP = mp.mpf(10) ** -20


def p_of(t):
    return t * (3 + t * t) / (1 + 3 * t * t)


def frame(R1, R2, g, v1, v2):
    """-> (dir, r_a, r_b, v_a, v_b): the sign of the marginal gain at zero, exact in mpmath."""
    px = R2 * (3 * R1 * R1 + R2 * R2)
    py = R1 * (R1 * R1 + 3 * R2 * R2)
    if g * v2 * px > v1 * py:
        return 1, R1, R2, v1, v2
    if v2 * px < g * v1 * py:
        return 2, R2, R1, v2, v1
    return 0, R1, R2, v1, v2


def t_closed(pi):
    c3 = (pi - 1) / (pi + 1)
    c = mp.sign(c3) * mp.cbrt(abs(c3))        # the real cube root
    return pi * (1 + c + c * c) / (1 - c + c * c)   # = (1 + c)/(1 − c), without its cancellation at extreme π


def truth(R1, R2, g, v1, v2):
    """-> (dir, Δ_a, Λ_b) in mpmath, by bisection on the KKT price equation (see the module docstring)."""
    d, ra, rb, va, vb = frame(R1, R2, g, v1, v2)
    if d == 0:
        return 0, mp.mpf(0), mp.mpf(0)
    pi = va / (g * vb)
    lo, hi = pi / 3, 3 * pi
    tol = mp.mpf(10) ** -70
    while hi - lo > tol * lo:
        mid = (lo + hi) / 2
        if p_of(mid) < pi:
            lo = mid
        else:
            hi = mid
    t = (lo + hi) / 2
    k = ra * rb * (ra * ra + rb * rb)
    xa = mp.root(k / (t * (1 + t * t)), 4)
    yb = t * xa
    # self-checks: the KKT system at (x′, y′), the closed form, the side of the trade
    assert abs(xa * yb * (xa * xa + yb * yb) / k - 1) < mp.mpf(10) ** -60
    assert abs((yb * (3 * xa * xa + yb * yb)) / (xa * (xa * xa + 3 * yb * yb)) / pi - 1) < mp.mpf(10) ** -60
    assert abs(t / t_closed(pi) - 1) < mp.mpf(10) ** -50, (R1, R2, g, v1, v2)
    assert xa >= ra and yb <= rb
    return d, (xa - ra) / g, rb - yb


def closed(R1, R2, g, v1, v2, want):
    """(Δ, Λ) of direction `want` by the closed form (0 when the perturbed pool does not trade that way)."""
    d, ra, rb, va, vb = frame(R1, R2, g, v1, v2)
    if d != want:
        return mp.mpf(0), mp.mpf(0)
    t = t_closed(va / (g * vb))
    xa = mp.root(ra * rb * (ra * ra + rb * rb) / (t * (1 + t * t)), 4)
    return max(xa - ra, 0) / g, max(rb - t * xa, 0)


def solve_row(args):
    x = [mp.mpf(float(a)) for a in args]
    d, dl, lm = truth(*x)
    cd = cl = mp.mpf(0)
    # the conditioning of the trade in its own direction; a pool inside the band: of whichever direction a
    # perturbation opens
    for want in ((d,) if d else (1, 2)):
        for j in range(5):
            up, dn = list(x), list(x)
            if j == 2:                                   # γ: one-sided, downwards
                dn[j] = x[j] * (1 - HSTEP)
                span = HSTEP
            else:
                up[j], dn[j] = x[j] * (1 + HSTEP), x[j] * (1 - HSTEP)
                span = 2 * HSTEP
            du, lu = closed(*up, want)
            dd, ld = closed(*dn, want)
            cd += abs(du - dd) / span
            cl += abs(lu - ld) / span
    return d, float(dl), float(lm), float(cd), float(cl)


def ulp_shift(x, k):
    x = float(x)
    for _ in range(abs(k)):
        x = float(np.nextafter(x, np.inf if k > 0 else -np.inf))
    return x


def edge_t0(g, v1, v2, side):
    """t₀ with the price ON a band limit: γ·p(t₀) = v₁/v₂ (side 1) or p(t₀)/γ = v₁/v₂ (side 2), in mpmath."""
    g, v1, v2 = mp.mpf(float(g)), mp.mpf(float(v1)), mp.mpf(float(v2))
    return t_closed(v1 / (g * v2) if side == 1 else g * v1 / v2)


def build():
    rng = np.random.default_rng(20261017)
    v = np.empty(NT)
    v[:8] = 1.0 + rng.choice([-1.0, 1.0], 8) * 10.0 ** rng.uniform(-6, -3, 8)
    v[8:16] = np.exp(rng.uniform(-0.5, 0.5, 8))
    v[16:] = np.exp(rng.uniform(-40, 40, NT - 16))

    def pairs(lo, hi, m):
        a = rng.integers(lo, hi, m)
        b = rng.integers(lo, hi - 1, m)
        return np.stack([a, b + (b >= a)], axis=1)

    R, G, AI, CLS = [], [], [], []
    for ci, name in enumerate(CLASSES):
        m = ROWS
        ai = pairs(0, 16, m)
        g = rng.choice([0.9999, 0.9995, 0.997], m)
        r1 = 10.0 ** rng.uniform(0, 6, m)
        t0 = np.exp(rng.uniform(-0.5, 0.5, m))
        r2 = r1 * t0
        if name == "balanced":
            g = rng.choice([1.0, 0.9995], m)
            r2 = r1.copy()
            off = rng.choice([-1.0, 1.0], m // 2) * 10.0 ** rng.uniform(-16, -9, m // 2)
            r2[m // 2:] = r1[m // 2:] * (1.0 + off)
        elif name in ("band_edge", "band"):
            if name == "band":
                g = rng.choice([0.9995, 0.997, 0.99], m)
            for i in range(m):
                v1, v2 = v[ai[i, 0]], v[ai[i, 1]]
                if name == "band_edge":
                    t = edge_t0(g[i], v1, v2, 1 + i % 2)
                    r2[i] = ulp_shift(float(mp.mpf(float(r1[i])) * t), int(rng.integers(-3, 4)))
                else:
                    s = rng.uniform(-0.9, 0.9)
                    t = t_closed(mp.mpf(float(v1)) / mp.mpf(float(v2)) * mp.mpf(float(g[i])) ** s)
                    r2[i] = float(mp.mpf(float(r1[i])) * t)
        elif name == "gamma1":
            g = np.ones(m)
        elif name == "low_gamma":
            g = rng.uniform(0.5, 0.9, m)
            r2 = r1 * np.exp(rng.uniform(-3, 3, m))     # (a band this wide needs a pool this far off to trade)
        elif name == "wide":
            ai = pairs(16, NT, m)
            r1 = 10.0 ** rng.uniform(-3, 6, m)
            r2 = r1 * np.exp(rng.uniform(-40, 40, m))
        elif name == "range":
            ends = np.array([2.0 ** -150, 2.0 ** 149])
            r1 = ends[rng.integers(0, 2, m)] * (1.0 + rng.random(m))
            r2 = ends[rng.integers(0, 2, m)] * (1.0 + rng.random(m))
        elif name == "drain":
            cand = [(a, b) for a in range(16, NT) for b in range(16, NT) if a != b and abs(np.log(v[a] / v[b])) > 46.0]
            assert len(cand) >= 32, len(cand)
            ai = np.array([cand[k] for k in rng.integers(0, len(cand), m)])
        R.append(np.stack([r1, r2], axis=1))
        G.append(g)
        AI.append(ai)
        CLS.append(np.full(m, ci, dtype=np.int8))
    return v, np.concatenate(R), np.concatenate(G), np.concatenate(AI), np.concatenate(CLS)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    v, R, g, ai, cls = build()
    rows = [(R[i, 0], R[i, 1], g[i], v[ai[i, 0]], v[ai[i, 1]]) for i in range(len(g))]
    with Pool(procs) as pool:
        res = pool.map(solve_row, rows, chunksize=64)
    d = np.array([r[0] for r in res], dtype=np.int8)
    dl, lm, cd, cl = (np.array([r[k] for r in res]) for k in (1, 2, 3, 4))
    # the classes are what they claim to be
    band = cls == CLASSES.index("band")
    assert np.all(d[band] == 0) and np.all(dl[band] == 0) and np.all(cd[band] == 0)
    drain = cls == CLASSES.index("drain")
    rb = np.where(d == 1, R[:, 1], R[:, 0])
    assert np.all(d[drain] != 0) and np.all((rb - lm)[drain] < 1e-12 * rb[drain])
    edge = cls == CLASSES.index("band_edge")
    assert 0 < np.count_nonzero(d[edge] == 0) < np.count_nonzero(edge)
    for name, share in (("well", 0.9), ("gamma1", 0.9), ("low_gamma", 0.6), ("wide", 0.9), ("range", 0.9)):
        sel = cls == CLASSES.index(name)
        assert np.count_nonzero(d[sel]) > share * np.count_nonzero(sel), name
    for ci, name in enumerate(CLASSES):
        sel = cls == ci
        print(f"{name:10s} pools {np.count_nonzero(sel):5d}  trading {np.count_nonzero(d[sel]):5d}  dir1 {np.count_nonzero(d[sel] == 1):5d}")
    np.savez_compressed(OUT, classes=np.array(CLASSES), v=v, R=R, gamma=g, Ai=(ai + 1).astype(np.int16), cls=cls, dir=d,
                        d=dl, l=lm, cd=cd, cl=cl)
    print(f"wrote {OUT}: {len(g)} pools, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
