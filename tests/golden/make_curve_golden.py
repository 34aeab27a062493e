"""Regenerates tests/golden/curve_precise.npz: Curve (StableSwap) trades to 60 significant digits, with the conditioning
of every trade.

    python tests/golden/make_curve_golden.py [processes]

Inputs are float64 exactly as the device receives them (R, γ, 1-based Ai, α, β, v); every truth is computed from those
float64 values taken as exact, in mpmath at 60 digits, and rounded ONCE to float64.  Nothing that decides a stored value
calls libm: an input built near a threshold is constructed in mpmath and then rounded, so the file is the same on every
host.  (The random draws use numpy, as tests/golden/make_precise_golden.py does.)

Truth: tests/curve_ref.py's decomposition, not the device's algorithm.  The outer unknown is s = log(v_min·x/γ − α) (x the
inverse multiplier); the terms v_k·x/γ − α = c_k·eˢ + α·e_k and v_k·x − α = γ·c_k·eˢ + α·(γ·c_k − 1) are exact in mpmath.
The inner E1 (L + Σ_k max(min(L − a_k^λ, ρ_k), L − a_k^δ) = log β) is piecewise linear in L and solved exactly: its 2N
breakpoints sorted, the segment that holds the root found by bisection over them, one linear solve.  The outer E2
(α·Σ(r_k − R_k) = P − P₀, decreasing in s) is bracketed by doubling from log(P₀/R_ref) and solved by Illinois (a
bisection whenever a step fails to halve the bracket) until the bracket is below 1e-50 relative.  Trades:
Λ_k = −R_k·expm1(log r_k − ρ_k), Δ_k = R_k·expm1(log r_k − ρ_k)/γ.

Conditioning (stored as cD, cL [m, N], float64): Σ_j |x_j·∂T/∂x_j| over the 2N + 3 inputs R_k, v_k, α, β, γ, by central
differences at a relative step of 1e-20 (γ: one-sided, downwards, since γ <= 1), each perturbed solve warm-started at s*.
A backward-stable solve -- and the device's stop on E2's own residual is a backward-error criterion -- may lose u times
this.  The log-space term of the bound is computed by tests/curve_precise_ref.py from the inputs and s* (stored as s).

Self-checks (the script fails before it writes if one fails): the KKT conditions at r* to 1e-45 relative, in mpmath
(tests/curve_ref.py::optimality_ok_mp: E2 tight, the fee band at r*); every α = 0 row against the equal-weight
weighted_truth of make_precise_golden.py to 40 digits; a sample of rows against a naive (ν, P) bisection in the style of
curve_ref.solve_decimal to 40 digits.

Cases: c_N for N = 2..8, n = 43 tokens: 0..7 "stable" prices (1 + 10^U[−6, −3] apart), 8..11 one tied price, 12..25
e^U[−0.5, 0.5], 26..39 10^U[−6, 6], 40..42 the prices 1.01, 1, 2 of the examples in the issue that pinned this family.
Classes (CLASSES): see tests/curve_precise_ref.py.  c_3 also has v2, the prices of the update test.
"""
import importlib.util
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

DPS = 60
mp.mp.dps = DPS
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "curve_precise.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import curve_ref  # noqa: E402

CLASSES = ["well", "stiff", "small_a", "alpha0", "drained", "band_edge", "on_bp", "near_bp", "ties", "low_gamma", "wide",
           "range", "far_start", "band"]
ROWS = 16          # per class and N (drained / range add the examples of the issue)
NT = 43
HSTEP = mp.mpf(10) ** -20


def _precise():
    spec = importlib.util.spec_from_file_location("make_precise_golden", os.path.join(HERE, "make_precise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f(x):
    """mpf -> the nearest float64 (ties to even): the one rounding of every stored value."""
    return mp.libmp.to_float(mp.mpf(x)._mpf_, rnd=mp.libmp.round_nearest)


def _M(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


# ---- truth ------------------------------------------------------------------------------------------------------

class Pool1:
    """One pool in mpmath from (float64 or mpf) inputs taken as exact."""

    def __init__(self, R, alpha, beta, gamma, v):
        self.N = N = len(R)
        self.R = [_M(x) for x in R]
        self.v = [_M(x) for x in v]
        self.a, self.b, self.g = _M(alpha), _M(beta), _M(gamma)
        self.rho = [mp.log(x) for x in self.R]
        self.lb = mp.log(self.b)
        self.L0 = self.lb - mp.fsum(self.rho)
        vmin = min(self.v)
        self.ref = self.v.index(vmin)
        self.c = [x / vmin for x in self.v]
        self.e = [(x - vmin) / vmin for x in self.v]
        self.el = [self.g * self.c[k] - 1 for k in range(N)]

    def band(self):
        P0 = mp.exp(self.L0)
        q = [(self.a + P0 / self.R[k]) / self.v[k] for k in range(self.N)]
        return max(self.g * x for x in q) <= min(q)

    def state(self, s):
        """-> (L, log r [N]) at s: E1's exact root."""
        N, es = self.N, mp.exp(s)
        ad = [mp.log(self.c[k] * es + self.a * self.e[k]) for k in range(N)]
        tl = [self.g * self.c[k] * es + self.a * self.el[k] for k in range(N)]
        al = [mp.log(t) if t > 0 else None for t in tl]

        def lr(L, k):
            t = self.rho[k] if al[k] is None else min(L - al[k], self.rho[k])
            return max(t, L - ad[k])

        F = lambda L: L + mp.fsum(lr(L, k) for k in range(N)) - self.lb
        bps = sorted([self.rho[k] + al[k] for k in range(N) if al[k] is not None] + [self.rho[k] + ad[k] for k in range(N)])
        lo, hi = 0, len(bps) - 1
        if F(bps[0]) >= 0:
            j = None                                     # the root lies below every breakpoint (or on the first)
        elif F(bps[-1]) <= 0:
            j = len(bps) - 1
        else:
            while hi - lo > 1:                           # F(bps[lo]) < 0 < F(bps[hi])
                mid = (lo + hi) // 2
                if F(bps[mid]) < 0:
                    lo = mid
                else:
                    hi = mid
            j = lo
        if j is None:
            b = bps[0]
        else:
            b = bps[j]
        Fb = F(b)
        if Fb == 0:
            L = b
        else:
            probe = b - 1 if j is None else (b + 1 if j == len(bps) - 1 else (b + bps[j + 1]) / 2)
            slope = 1 + sum((1 if al[k] is not None and probe < self.rho[k] + al[k] else 0) +
                            (1 if probe > self.rho[k] + ad[k] else 0) for k in range(N))
            L = b - Fb / slope
        return L, [lr(L, k) for k in range(N)]

    def e2(self, s):
        L, lr = self.state(s)
        h = self.a * mp.fsum(self.R[k] * mp.expm1(lr[k] - self.rho[k]) for k in range(self.N)) - \
            mp.exp(self.L0) * mp.expm1(L - self.L0)
        return h, L, lr

    def solve(self, hint=None):
        """-> (s*, log r*) or None in the fee band."""
        if self.band():
            return None
        if hint is None:
            s0, d = self.L0 - self.rho[self.ref], mp.mpf(1)
        else:
            s0, d = hint, mp.mpf(10) ** -12 * (1 + abs(hint))
        lo, hi = s0 - d, s0 + d
        flo, fhi = self.e2(lo)[0], self.e2(hi)[0]
        step = 2 * d
        while flo <= 0:
            hi, fhi = lo, flo
            lo -= step
            step *= 2
            flo = self.e2(lo)[0]
        while fhi >= 0:
            lo, flo = hi, fhi
            hi += step
            step *= 2
            fhi = self.e2(hi)[0]
        side, width = 0, hi - lo
        tol = mp.mpf(10) ** -50
        while hi - lo > tol * max(1, abs(lo), abs(hi)):
            x = hi - fhi * (hi - lo) / (fhi - flo)
            if not (lo < x < hi) or (hi - lo) > width / 2:
                x = (lo + hi) / 2                        # a step that did not halve the bracket: bisect
            width = hi - lo
            fx = self.e2(x)[0]
            if fx == 0:
                lo = hi = x
                break
            if fx > 0:
                lo, flo = x, fx
                if side == 1:
                    fhi /= 2                             # Illinois
                side = 1
            else:
                hi, fhi = x, fx
                if side == -1:
                    flo /= 2
                side = -1
        s = (lo + hi) / 2
        return s, self.state(s)[1]

    def trades(self, lr):
        D = [self.R[k] * mp.expm1(lr[k] - self.rho[k]) / self.g if lr[k] > self.rho[k] else mp.mpf(0) for k in range(self.N)]
        L = [-self.R[k] * mp.expm1(lr[k] - self.rho[k]) if lr[k] < self.rho[k] else mp.mpf(0) for k in range(self.N)]
        return D, L


def curve_truth(R, alpha, beta, gamma, v, hint=None, with_r=False):
    """-> (Δ [N], Λ [N] as mpf, s* or None[, r* [N]])."""
    p = Pool1(R, alpha, beta, gamma, v)
    out = p.solve(hint)
    if out is None:
        z = [mp.mpf(0)] * p.N
        return (z, list(z), None, list(p.R)) if with_r else (z, list(z), None)
    s, lr = out
    D, L = p.trades(lr)
    return (D, L, s, [mp.exp(x) for x in lr]) if with_r else (D, L, s)


def conditioning(R, alpha, beta, gamma, v, D, L, s):
    """Σ_j |x_j·∂T/∂x_j| per trade -> (cD [N], cL [N]) as mpf."""
    N = len(R)
    x = [_M(t) for t in R] + [_M(t) for t in v] + [_M(alpha), _M(beta), _M(gamma)]
    cD, cL = [mp.mpf(0)] * N, [mp.mpf(0)] * N

    def run(xx):
        return curve_truth(xx[:N], xx[2 * N], xx[2 * N + 1], xx[2 * N + 2], xx[N:2 * N], hint=s)

    for j in range(len(x)):
        if x[j] == 0:
            continue
        if j == 2 * N + 2:                                   # γ: one-sided, downwards
            up, dn, span = x, list(x), HSTEP
            dn[j] = x[j] * (1 - HSTEP)
            Du, Lu = D, L
            Dd, Ld, _ = run(dn)
        else:
            up, dn, span = list(x), list(x), 2 * HSTEP
            up[j] = x[j] * (1 + HSTEP)
            dn[j] = x[j] * (1 - HSTEP)
            Du, Lu, _ = run(up)
            Dd, Ld, _ = run(dn)
        for k in range(N):
            cD[k] += abs(Du[k] - Dd[k]) / span
            cL[k] += abs(Lu[k] - Ld[k]) / span
    return cD, cL


def naive_truth(R, alpha, beta, gamma, v, digits=50):
    """The naive (ν, P) form in mpmath, in the style of curve_ref.solve_decimal: terms v_k·x − α formed as they read,
    bisection on log(x − α·γ/v_min), inner bisection on L."""
    with mp.workdps(digits + 10):
        p = Pool1(R, alpha, beta, gamma, v)
        if p.band():
            return [mp.mpf(0)] * p.N, [mp.mpf(0)] * p.N
        N, a, g, vm = p.N, p.a, p.g, min(p.v)

        def state(y):
            xx = a * g / vm + mp.exp(y)
            ad = [mp.log(p.v[k] * xx / g - a) for k in range(N)]
            al = [mp.log(p.v[k] * xx - a) if p.v[k] * xx - a > 0 else None for k in range(N)]
            lr = lambda L, k: max(p.rho[k] if al[k] is None else min(L - al[k], p.rho[k]), L - ad[k])
            F = lambda L: L + mp.fsum(lr(L, k) for k in range(N)) - p.lb
            lo, hi = p.L0 - 1, p.L0 + 1
            while F(lo) > 0:
                lo -= 2 * (hi - lo)
            while F(hi) < 0:
                hi += 2 * (hi - lo)
            for _ in range(4 * digits):
                mid = (lo + hi) / 2
                lo, hi = (mid, hi) if F(mid) < 0 else (lo, mid)
            Lr = (lo + hi) / 2
            r = [mp.exp(lr(Lr, k)) for k in range(N)]
            return r, a * mp.fsum(r[k] - p.R[k] for k in range(N)) - (mp.exp(Lr) - mp.exp(p.L0))

        ylo, yhi = mp.mpf(-1), mp.mpf(1)
        base = mp.log(max((a + mp.exp(p.L0) / p.R[k]) / p.v[k] for k in range(N)))
        while state(base + ylo)[1] <= 0:
            ylo -= 2 * (yhi - ylo)
        while state(base + yhi)[1] >= 0:
            yhi += 2 * (yhi - ylo)
        for _ in range(4 * digits):
            mid = (ylo + yhi) / 2
            ylo, yhi = (mid, yhi) if state(base + mid)[1] > 0 else (ylo, mid)
        r, _ = state(base + (ylo + yhi) / 2)
        D = [(r[k] - p.R[k]) / g if r[k] > p.R[k] else mp.mpf(0) for k in range(N)]
        L = [p.R[k] - r[k] if r[k] < p.R[k] else mp.mpf(0) for k in range(N)]
        return D, L


def row_job(args):
    """One row: truth, s*, conditioning and the KKT self-check -> float64 arrays."""
    R, alpha, beta, gamma, v = args
    D, L, s, r = curve_truth(R, alpha, beta, gamma, v, with_r=True)
    N = len(R)
    if s is None:
        z = np.zeros(N)
        return z, z.copy(), 0.0, z.copy(), z.copy()
    assert curve_ref.optimality_ok_mp(v, D, L, R, alpha, beta, gamma, rtol=mp.mpf(10) ** -45, Rp=r), (R, alpha, beta, gamma, v)
    cD, cL = conditioning(R, alpha, beta, gamma, v, D, L, s)
    return (np.array([_f(x) for x in D]), np.array([_f(x) for x in L]), _f(s), np.array([_f(x) for x in cD]),
            np.array([_f(x) for x in cL]))


# ---- inputs -----------------------------------------------------------------------------------------------------

def prices(rng):
    v = np.concatenate([1.0 + 10.0 ** rng.uniform(-6, -3, 8) * rng.choice([-1, 1], 8), np.full(4, 1.25),
                        np.exp(rng.uniform(-0.5, 0.5, 14)), 10.0 ** rng.uniform(-6, 6, 14), [1.01, 1.0, 2.0]])
    return v


def _toks(rng, N, lo, hi):
    return rng.choice(np.arange(lo, hi), N, replace=False) + 1


def _ss(bal, A):
    """(α, β) of a StableSwap pool: α = A·nⁿ, β = D^{n+1}/nⁿ with D the invariant, in mpmath, rounded once."""
    n = len(bal)
    x = [_M(t) for t in bal]
    Ann = _M(A) * n ** n
    S, Px = mp.fsum(x), mp.fprod(x)
    f = lambda D: Ann * S + D - Ann * D - D ** (n + 1) / (mp.mpf(n) ** n * Px)
    lo, hi = mp.mpf(0), S                                    # f(0) > 0 >= f(S) (AM-GM)
    for _ in range(220):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    D = (lo + hi) / 2
    return _f(Ann), _f(D ** (n + 1) / mp.mpf(n) ** n)


def case_inputs(rng, N, v):
    rows = []   # (R, α, β, γ, Ai, class)

    def add(R, a, b, g, A, c):
        rows.append((np.asarray(R, dtype=np.float64), float(a), float(b), float(g), np.asarray(A, dtype=np.int32),
                     CLASSES.index(c)))

    def logu(lo, hi):
        return 10.0 ** rng.uniform(lo, hi)

    for _ in range(ROWS):                                    # well
        A = logu(0, 3.7)
        bal = logu(-3, 6) * rng.uniform(0.9, 1.1, N)
        add(bal, *_ss(bal, A), rng.choice([0.9996, 0.997, 1.0]), _toks(rng, N, 12, 26), "well")
    for _ in range(ROWS):                                    # stiff: prices 1e-6..1e-3 apart, A up to 1e5
        A = logu(3, 5)
        bal = logu(0, 6) * rng.uniform(0.99, 1.01, N)
        add(bal, *_ss(bal, A), rng.choice([1.0, 1.0 - 2.0 ** -20, 0.99999]), _toks(rng, N, 0, 8), "stiff")
    for _ in range(ROWS):                                    # small_a
        A = logu(-2, 0)
        bal = logu(-3, 6) * rng.uniform(0.5, 2.0, N)
        add(bal, *_ss(bal, A), rng.choice([0.997, 1.0]), _toks(rng, N, 12, 26), "small_a")
    for i in range(ROWS):                                    # alpha0: β over 1e±300
        R = 10.0 ** rng.uniform(-3, 6, N)
        add(R, 0.0, logu(-300, 300), rng.choice([0.997, 1.0]), _toks(rng, N, 12, 40), "alpha0")
    if N == 2:                                               # the drained pool of the issue, both directions
        for A in ([41, 42], [42, 41]):
            add([1e12, 1e-6], *_ss([1e12, 1e-6], 1000.0), 0.9996, A, "drained")
    for _ in range(ROWS - (2 if N == 2 else 0)):             # drained: 1..N−1 coins at 1e-9..1e-3 of the others
        A = logu(1, 3.7)
        bal = logu(0, 9) * rng.uniform(0.9, 1.1, N)
        few = rng.choice(N, rng.integers(1, N), replace=False)
        bal[few] *= 10.0 ** rng.uniform(-9, -3, len(few))
        add(bal, *_ss(bal, A), rng.choice([0.9996, 0.997, 1.0]), _toks(rng, N, 12, 26), "drained")
    def band_row(k, sgn, c):
        """max γ∇φ/v = min ∇φ/v·(1 + sgn·2^-k) at R, on log β (bisection in mpmath); False if the prices cannot reach it."""
        A = _toks(rng, N, 12, 26)
        vl = [_M(v[t - 1]) for t in A]
        g = _M(rng.choice([0.997, 0.9996]))
        B = mp.mpf(logu(0, 4))
        R = [_f(B / x * (1 + mp.mpf(rng.uniform(-1e-4, 1e-4)))) for x in vl]
        al = _M(logu(-1, 2))
        Rm = [_M(x) for x in R]
        sr = mp.fsum(mp.log(x) for x in Rm)
        target = mp.log(1 + sgn * mp.mpf(2) ** -k)

        def h(lb):
            q = [(al + mp.exp(lb - sr) / Rm[j]) / vl[j] for j in range(N)]
            return mp.log(max(g * x for x in q)) - mp.log(min(q)) - target

        lo, hi = mp.log(al) + sr + mp.log(B) - 40, mp.log(al) + sr + mp.log(B) + 40   # h(lo) > 0 > h(hi)
        if not (h(lo) > 0 > h(hi)):
            return False
        for _ in range(230):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if h(mid) > 0 else (lo, mid)
        add(R, _f(al), _f(mp.exp((lo + hi) / 2)), _f(g), A, c)
        return True

    got = 0
    while got < ROWS:                                        # band_edge: k = 10..52, both sides of the edge
        got += band_row(10 + got % 43, 1 if got % 2 else -1, "band_edge")
    for near in (False, True):                               # on_bp / near_bp: built backwards from the optimum
        got = 0
        while N == 2 and got < ROWS:                         # two coins: the threshold of the idle coin is the band edge
            got += band_row(int(rng.integers(20, 46)), rng.choice([-1, 1]), "near_bp") if near else \
                band_row(10 ** 6, 1, "on_bp")
        while got < ROWS:
            A = _toks(rng, N, 12, 40)
            vl = [_M(v[t - 1]) for t in A]
            g = _M(rng.choice([0.997, 0.9996, 1.0]))
            al = _M(logu(-1, 3)) if rng.integers(0, 4) else mp.mpf(0)
            x = al * (1 + mp.mpf(rng.uniform(0.2, 3))) / min(vl) + max(vl) / min(vl) * mp.mpf(rng.uniform(0.01, 1))
            P = mp.mpf(logu(-2, 4))
            # roles: 0 leaves, 1 enters, 2 idle (inside its band), 3 = coin j on its threshold
            role = list(rng.integers(0, 3, N))
            j, mcoin = rng.choice(N, 2, replace=False)
            role[j], role[mcoin] = 3, 0
            if 1 not in role:                                # a coin must enter to pay for the one that leaves
                role[[k for k in range(N) if k not in (j, mcoin)][0]] = 1
            if all(vl[k] * x - al <= 0 for k in range(N)):
                continue
            r, Rr = [None] * N, [None] * N
            ok = True
            for k in range(N):
                tl, td = vl[k] * x - al, vl[k] * x / g - al
                if role[k] in (0, 3) and tl <= 0:
                    ok = False
                    break
                if role[k] == 0:
                    r[k] = P / tl
                elif role[k] == 1:
                    r[k] = P / td
                    Rr[k] = r[k] * mp.mpf(rng.uniform(0.2, 0.9))
                elif role[k] == 2:
                    hi_r = P / tl if tl > 0 else P / td * 10
                    r[k] = Rr[k] = P / td + (hi_r - P / td) * mp.mpf(rng.uniform(0.1, 0.9))
                else:
                    onl = rng.integers(0, 2) or g == 1
                    r[k] = Rr[k] = P / tl if onl else P / td       # leave or enter threshold
            if not ok:
                continue
            for k in range(N):
                if role[k] == 0 and k != mcoin:
                    Rr[k] = r[k] * mp.mpf(rng.uniform(1.1, 5))
            beta = P * mp.fprod(r)
            # E2 closes on R of coin mcoin: −α·R² + (α·r_m + C1 − P)·R + β/C2 = 0
            C1 = al * mp.fsum(r[k] - Rr[k] for k in range(N) if k != mcoin)
            C2 = mp.fprod(Rr[k] for k in range(N) if k != mcoin)
            if al == 0:
                Rm = beta / (C2 * P)
            else:
                bq = al * r[mcoin] + C1 - P
                Rm = (bq + mp.sqrt(bq * bq + 4 * al * beta / C2)) / (2 * al)
            if not Rm > r[mcoin] * (1 + mp.mpf(10) ** -6):
                continue
            Rr[mcoin] = Rm
            if near:
                Rr[j] = Rr[j] * (1 + mp.mpf(2) ** -int(rng.integers(10, 46)) * (1 if rng.integers(0, 2) else -1))
            add([_f(t) for t in Rr], _f(al), _f(beta), _f(g), A, "near_bp" if near else "on_bp")
            got += 1
    for _ in range(ROWS):                                    # ties: equal prices (e_k = 0) and, beside an untied coin, reserves
        nt = 2 if N == 2 else int(rng.integers(2, min(N - 1, 4) + 1))
        A = np.concatenate([_toks(rng, nt, 8, 12), _toks(rng, N - nt, 12, 26)])
        rng.shuffle(A)
        bal = logu(0, 6) * rng.uniform(0.5, 2.0, N)
        tied = [k for k in range(N) if A[k] <= 12]
        if N > 2:
            bal[tied] = bal[tied[0]]
        add(bal, *_ss(bal, logu(0, 3)), rng.choice([0.997, 1.0]), A, "ties")
    for i in range(ROWS):                                    # low_gamma
        A = logu(-1, 3)
        bal = logu(-3, 6) * rng.uniform(0.5, 2.0, N)
        add(bal, *_ss(bal, A), [0.5, 0.3, 0.1, 2.0 ** -10][i % 4], _toks(rng, N, 12, 40), "low_gamma")
    for _ in range(ROWS):                                    # wide: reserves 1e±12, prices 1e±6
        bal = 10.0 ** rng.uniform(-12, 12, N)
        a, b = _ss(bal, logu(-2, 3))
        add(bal, a, b, rng.choice([0.5, 0.9, 0.997, 0.9999, 1.0]), _toks(rng, N, 26, 40), "wide")
    if N == 2:                                               # range: the two examples of the issue
        add([1e10, 1e10], 0.0, 1e-300, 1.0, [42, 43], "range")
        add([1e10, 1e10], 1.0, 1e-300, 1.0, [42, 43], "range")
        add([1e-100, 1e-100], 0.0, 1e300, 1.0, [42, 43], "range")
    while sum(1 for r in rows if r[5] == CLASSES.index("range")) < ROWS:   # log P₀ − ρ_k beyond ±709
        R = 10.0 ** rng.uniform(-3, 9, N)
        a = 0.0 if rng.integers(0, 2) else logu(-2, 4)
        lb = float(np.sum(np.log(R))) + rng.choice([-1, 1]) * rng.uniform(720, 1200) + np.log(R[0])
        if abs(lb) > 700:
            continue
        add(R, a, _f(mp.exp(_M(lb))), rng.choice([0.997, 1.0]), _toks(rng, N, 12, 40), "range")
    for _ in range(ROWS):                                    # far_start: α·R_k/P₀ ~ e^300..e^560, s* far below the start
        R = 10.0 ** rng.uniform(0, 6, N)
        a = logu(-1, 2)
        x = rng.uniform(-560, -300)
        lb = _M(float(np.sum(np.log(R))) + float(np.log(R[0]))) + mp.log(_M(a)) + _M(x)
        add(R, a, _f(mp.exp(lb)), rng.choice([0.997, 1.0]), _toks(rng, N, 12, 26), "far_start")
    for _ in range(ROWS):                                    # band: equal value per coin, γ·spread inside the band
        A = _toks(rng, N, 0, 8)
        bal = logu(0, 6) * rng.uniform(0.9999, 1.0001, N) / v[A - 1]
        add(bal, *_ss(bal, logu(0, 3)), rng.choice([0.99, 0.997]), A, "band")
    return rows


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    rng = np.random.default_rng(20261017)
    cases, jobs = {}, []
    for N in range(2, 9):
        v = prices(rng)
        rows = case_inputs(rng, N, v)
        c = dict(v=v, R=np.array([r[0] for r in rows]), alpha=np.array([r[1] for r in rows]),
                 beta=np.array([r[2] for r in rows]), gamma=np.array([r[3] for r in rows]),
                 Ai=np.array([r[4] for r in rows], dtype=np.int32), cls=np.array([r[5] for r in rows], dtype=np.int8))
        if N == 3:
            c["v2"] = v * np.exp(rng.uniform(-0.05, 0.05, NT))
        cases[f"c_{N}"] = c
        for i in range(len(rows)):
            jobs.append((c["R"][i], c["alpha"][i], c["beta"][i], c["gamma"][i], v[c["Ai"][i] - 1]))
    with Pool(procs) as pool:
        res = pool.map(row_job, jobs, chunksize=1)
    k = 0
    for name in sorted(cases, key=lambda s: int(s[2:])):
        c = cases[name]
        m = len(c["gamma"])
        part = res[k:k + m]
        k += m
        c["D"], c["L"] = np.array([p[0] for p in part]), np.array([p[1] for p in part])
        c["s"] = np.array([p[2] for p in part])
        c["cD"], c["cL"] = np.array([p[3] for p in part]), np.array([p[4] for p in part])
    check(cases, procs)
    out = dict(cases=np.array(sorted(cases)), classes=np.array(CLASSES))
    for name, c in cases.items():
        out.update({f"{name}_{key}": a for key, a in c.items()})
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {sum(len(c['gamma']) for c in cases.values())} Curve pools")


# ---- checks the generator makes before it writes ----------------------------------------------------------------

def _close(a, b, scale, digits=40):
    return all(abs(x - y) <= mp.mpf(10) ** -digits * scale for x, y in zip(a, b))


def alpha0_job(args):
    R, beta, g, v = args
    D, L, _ = curve_truth(R, 0.0, beta, g, v)
    Dw, Lw = _precise().weighted_truth(R, np.full(len(R), 1.0 / len(R)), g, v)
    scale = max(_M(x) for x in R) + max(D + L)
    return _close(D + L, Dw + Lw, scale)


def naive_job(args):
    R, a, b, g, v = args
    D, L, _ = curve_truth(R, a, b, g, v)
    Dn, Ln = naive_truth(R, a, b, g, v)
    scale = max(_M(x) for x in R) + max(D + L)
    return _close(D + L, Dn + Ln, scale)


def check(cases, procs):
    a0, nv = [], []
    chk = np.random.default_rng(7)
    for name, c in sorted(cases.items()):
        vl = c["v"][c["Ai"] - 1]
        for i in np.flatnonzero(c["alpha"] == 0):
            a0.append((c["R"][i], c["beta"][i], c["gamma"][i], vl[i]))
        # the naive form forms v·x − α as it reads: keep to rows whose terms it can resolve in 60 digits
        ok = np.flatnonzero(np.isin(c["cls"], [CLASSES.index(k) for k in ("well", "small_a", "drained", "ties", "wide",
                                                                           "low_gamma", "on_bp", "near_bp", "band")]))
        for i in chk.choice(ok, 6, replace=False):
            nv.append((c["R"][i], c["alpha"][i], c["beta"][i], c["gamma"][i], vl[i]))
    with Pool(procs) as pool:
        r0 = pool.map(alpha0_job, a0, chunksize=1)
        r1 = pool.map(naive_job, nv, chunksize=1)
    assert all(r0), [a0[i] for i in range(len(a0)) if not r0[i]][:3]
    assert all(r1), [nv[i] for i in range(len(nv)) if not r1[i]][:3]
    print(f"self-checks: KKT on every trading row, {len(a0)} α = 0 rows against weighted_truth, {len(nv)} naive solves")


if __name__ == "__main__":
    main()
