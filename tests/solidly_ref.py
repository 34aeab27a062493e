"""CPU reference for Solidly-style stable pairs, φ(x, y) = x³y + xy³.  numpy only.

The problem is the one of the reference's find_arb! docstring (src/cfmms.jl:21-33): maximise
v₁(λ₁ − δ₁) + v₂(λ₂ − δ₂) subject to φ(R + γΔ − Λ) >= φ(R), Δ, Λ >= 0, with 0 < γ <= 1.

  solve         the closed form, float64.  The marginal price of the tendered coin a in the received coin b depends on
                t = r_b/r_a only, p(t) = t(3 + t²)/(1 + 3t²), and p(t) = π ⇔ (t − 1)/(t + 1) = cbrt((π − 1)/(π + 1)).
  solve_bisect  a separate solver that knows none of that: it bisects on the tendered amount δ, takes the received
                coin's new reserve from the invariant by Newton, and chooses the direction by the sign of the marginal
                gain at δ = 0.
  optimality_ok the reference's predicate (test/cfmms.jl:3-22) restated for this φ.
"""
import numpy as np


def _fms(a, b, c):
    """c − a·b with ONE rounding (Dekker's error-free product; numpy has no fma): the numerator v_a − γ·v_b of c³
    cancels for pools near the fee band, and the device forms it with a fused multiply-add."""
    with np.errstate(over="ignore", invalid="ignore"):
        split = 134217729.0                      # 2^27 + 1
        a1 = (a * split) - ((a * split) - a)
        a2 = a - a1
        b1 = (b * split) - ((b * split) - b)
        b2 = b - b1
        p = a * b
        e = ((a1 * b1 - p) + a1 * b2 + a2 * b1) + a2 * b2    # a·b = p + e exactly
    return (c - p) - e


def marginal_price(R):
    """p = φₓ/φ_y at R [m, 2]: the price of coin 1 in coin 2."""
    x, y = R[:, 0], R[:, 1]
    return (y * (3.0 * x * x + y * y)) / (x * (x * x + 3.0 * y * y))


def direction(R, gamma, v):
    """[m] int: 1 (tender coin 1), 2 (tender coin 2) or 0 (inside the fee band) -- decided without a division."""
    x, y, v1, v2 = R[:, 0], R[:, 1], v[:, 0], v[:, 1]
    A = v2 * (y * (3.0 * x * x + y * y))
    B = v1 * (x * (x * x + 3.0 * y * y))
    return np.where(gamma * A > B, 1, np.where(A < gamma * B, 2, 0))


def solve(R, gamma, v):
    """R, v: [m, 2] (v = the prices of each pool's two coins); gamma: [m].  -> (Δ, Λ) [m, 2]."""
    R = np.asarray(R, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    g = np.asarray(gamma, dtype=np.float64).reshape(-1)
    d = direction(R, g, v)
    one = d != 2                                   # the frame of the tendered coin a / received coin b
    ra, rb = np.where(one, R[:, 0], R[:, 1]), np.where(one, R[:, 1], R[:, 0])
    va, vb = np.where(one, v[:, 0], v[:, 1]), np.where(one, v[:, 1], v[:, 0])
    with np.errstate(all="ignore"):
        c = np.cbrt(_fms(g, vb, va) / (va + g * vb))      # c³ = (π − 1)/(π + 1), π = v_a/(γ·v_b)
        t = (va * (1.0 + c + c * c)) / ((g * vb) * (1.0 - c + c * c))   # (1 + c)/(1 − c) without its cancellation
        t0 = rb / ra
        xa = ra * np.sqrt(np.sqrt((t0 * (1.0 + t0 * t0)) / (t * (1.0 + t * t))))   # φ(r′) = φ(r), r_b′ = t·r_a′
        dl = np.maximum(xa - ra, 0.0) / g
        lm = np.maximum(rb - t * xa, 0.0)
    dl, lm = np.where(d == 0, 0.0, dl), np.where(d == 0, 0.0, lm)
    z = np.zeros_like(dl)
    D = np.stack([np.where(d == 1, dl, z), np.where(d == 2, dl, z)], axis=1)
    L = np.stack([np.where(d == 2, lm, z), np.where(d == 1, lm, z)], axis=1)
    return D, L


def _other_reserve(xa, ra, rb):
    """y with φ(xa, y) = φ(ra, rb), by Newton on f(y) = xa·y·(xa² + y²) − k in the scale-free variables of r_a
    (f is increasing and convex for y > 0: from above the root the iteration descends monotonically)."""
    X, k = xa / ra, (rb / ra) * (1.0 + (rb / ra) ** 2)
    y = np.minimum(rb / ra, np.cbrt(k / X))        # f(y) >= 0 at both candidates (X >= 1): start from the nearer one
    for _ in range(200):
        f = X * y * (X * X + y * y) - k
        yn = y - f / (X * (X * X + 3.0 * y * y))
        if np.all(np.abs(yn - y) <= 2 * np.finfo(float).eps * y):
            y = yn
            break
        y = yn
    return y * ra


def solve_bisect(R, gamma, v):
    """Same problem, other algorithm: per pool the gain G(δ) = v_b·(r_b − y(r_a + γδ)) − v_a·δ is concave in the tendered
    amount δ; the direction is the coin whose G′(0) = γ·v_b·p − v_a is positive, and δ* is found by bisection on the sign
    of G′(δ) (a marginal price, no cube root anywhere), y(·) by Newton on the invariant."""
    R = np.asarray(R, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    g = np.asarray(gamma, dtype=np.float64).reshape(-1)
    p12 = marginal_price(R)
    gain1 = g * v[:, 1] * p12 - v[:, 0]            # marginal gain of tendering coin 1 at δ = 0
    gain2 = g * v[:, 0] / p12 - v[:, 1]
    d = np.where(gain1 > 0, 1, np.where(gain2 > 0, 2, 0))
    one = d != 2
    ra, rb = np.where(one, R[:, 0], R[:, 1]), np.where(one, R[:, 1], R[:, 0])
    va, vb = np.where(one, v[:, 0], v[:, 1]), np.where(one, v[:, 1], v[:, 0])

    def slope(xa):                                 # G′ at the tendered coin's reserve xa (up to the factor 1/γ... sign only)
        y = _other_reserve(xa, ra, rb)
        p = (y * (3.0 * xa * xa + y * y)) / (xa * (xa * xa + 3.0 * y * y))
        return g * vb * p - va

    lo = ra.copy()                                 # slope(lo) > 0 on trading pools
    hi = ra * 2.0
    for _ in range(1100):                          # gallop until the slope turns negative
        grow = slope(hi) > 0
        if not np.any(grow & (d != 0)):
            break
        lo = np.where(grow, hi, lo)
        hi = np.where(grow, hi * 2.0, hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        pos = slope(mid) > 0
        lo = np.where(pos, mid, lo)
        hi = np.where(pos, hi, mid)
        if np.all(hi - lo <= 2 * np.finfo(float).eps * hi):
            break
    xa = 0.5 * (lo + hi)
    dl = np.where(d == 0, 0.0, np.maximum(xa - ra, 0.0) / g)
    lm = np.where(d == 0, 0.0, np.maximum(rb - _other_reserve(xa, ra, rb), 0.0))
    z = np.zeros_like(dl)
    D = np.stack([np.where(d == 1, dl, z), np.where(d == 2, dl, z)], axis=1)
    L = np.stack([np.where(d == 2, lm, z), np.where(d == 1, lm, z)], axis=1)
    return D, L


def sweep(batch, v):
    """One Solidly PoolBatch (1-based Ai [m, 2]) at global prices v -> (Δ, Λ) [m, 2]."""
    return solve(batch.R, batch.γ, np.asarray(v, dtype=np.float64)[batch.Ai - 1])


def netflows(D, L, Ai0, n_tokens):
    return np.bincount(np.asarray(Ai0).ravel(), weights=(L - D).ravel(), minlength=n_tokens)[:n_tokens]


def dual_acc(D, L, Ai0, v):
    vl = np.asarray(v, dtype=np.float64)[Ai0]
    return float(np.sum((L * vl).sum(axis=1) - (D * vl).sum(axis=1)))


def phi(R):
    return R[0] * R[1] * (R[0] * R[0] + R[1] * R[1])


def grad_phi(R):
    x, y = R[0], R[1]
    return np.array([y * (3.0 * x * x + y * y), x * (x * x + 3.0 * y * y)])


def optimality_ok(v_local, D, L, R, gamma):
    """The reference's optimality predicate (test/cfmms.jl:3-22) for one pool: primal feasibility, the trading function
    kept (ϕ(R⁺) ≈ ϕ(R), ϕ(R⁺) >= ϕ(R) − √eps·ϕ(R)) and max γ∇ϕ_i/c_i <= min ∇ϕ_i/c_i·(1 + √eps) at R⁺ = R + γΔ − Λ.
    (φ has degree 4: the two tolerances are relative, where the reference's are absolute on φ of degree 1 or 2.)"""
    R = np.asarray(R, dtype=np.float64)
    Rp = R + gamma * D - L
    se = np.sqrt(np.finfo(float).eps)
    pfeas = bool(np.all(D >= 0) and np.all(L >= 0))
    pR, pRp = phi(R), phi(Rp)
    sat = bool(np.isclose(pR, pRp, rtol=se, atol=0.0) and pRp >= pR * (1.0 - se))
    q = grad_phi(Rp) / np.asarray(v_local, dtype=np.float64)
    opt = bool(np.max(gamma * q) <= np.min(q) * (1.0 + se))
    return pfeas and sat and opt
