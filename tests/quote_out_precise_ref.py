"""Exact-output swap quotes against an 80-digit truth: the fixture's loader, the bound, the K table and a numpy restatement
of the inverse forms of csrc/quote_pool.h (quote_out_*: the instrument K was measured with).  No device, no library: plain
numpy.  Patterned on quote_precise_ref.py, whose record preparation and helpers it reuses.

The truth (tests/golden/make_quote_out_golden.py -> tests/golden/quote_out_precise.npz) does not use the project's
arithmetic: per row it is the root `a` of φ(R + γ·a·e_in − o·e_out) = φ(R), found by bracketing bisection on φ itself
(weighted pools: log φ) in mpmath at 80 digits, stored as the nearest double (UniV3: the reference's tick-by-tick walk,
src/cfmms.jl:401-434, inverted tick by tick in mpmath from the ladder).  The rows are those of quote_precise.npz -- same
states, coins and classes -- with o = that fixture's stored `out`, plus the classes that only the inverse has.

The bound.  First-order error propagation through a short composition of correctly rounded operations, applied to the
state AS THE DEVICE HOLDS IT:
    |a − a*|  <=  K·u·( R_i/γ  +  a*  +  Σ_j |x_j · ∂a/∂x_j| ),   u = 2^-53
where R_i/γ (`scale`) covers a final subtraction from the input reserve (Solidly forms u·y′ − R_i), a* the rounding of the
result and its last operations, and the conditioning sum (`cond`, from the truth's side, stored per row) what a relative
perturbation u of every input does to the result.  The inputs are
    Product, Solidly   R_i, R_o, γ, o
    weighted           R_i, R_o, w_i, w_o, γ, o
    Curve              R_i, R_o, α, γ, o, and the LOGS the device holds: log β and every log R_k enter through
                       P₀ = exp(log β − Σ log R_k), so with g = ∂a/∂log P₀ their share is (|log β| + Σ_k |log R_k|)·|g|
    UniV3              o, γ and the prepared constants (csrc/univ3_pool.h): a drained tick j contributes δmax_j = k_j/β_j − s_in,j,
                       conditioned by (k_j/β_j + s_in,j)/γ, and its R_out,j = s_out,j − β_j moves o_t = o − ΣR_out, conditioned by
                       (s_out,j + β_j)·∂a/∂o; the landing tick d = s_in·o_t/(s_out − o_t) by d/γ (s_in) and s_out·∂a/∂o (s_out);
                       o itself by o·∂a/∂o, with ∂a/∂o = s_in·s_out/(s_out − o_t)²/γ.  `scale` is (Σ_j (k_j/β_j + s_in,j) + s_in)/γ:
                       the roots that the walked δmax are differences of, and the landing tick's.
Near a drained pool (o → R_o) ∂a/∂R_o and ∂a/∂o grow without bound and the conditioning sum with them: the bound is
honest about a question that is ill-conditioned there, it is not slack in the form.

Rows whose truth is +inf (no finite input yields o) are compared for equality, not by the bound.  The UniV3 classes
`exhausted`, `closing_exact`, `on_boundary` and `asymptotic` take o BIT FOR BIT from the sums the upload prepares
(quote_precise_ref.univ3_prepare: the closing record's or a record's ΣR_out): the answer is discontinuous at a direction's
total, and the semantics are defined on the sums the device holds ("o equal to the closing record's ΣR_out gives Σδmax/γ").
Their truth is the exact Σδmax/γ of the ladder (closing rows) or the exact inverse walk at that o (boundary rows).

K per class: the numpy restatement below is run over the fixture on the CPU; K is the next power of two >= 2x its worst
ratio in the class, capped at 16 on `typical` and 64 elsewhere (quote_precise_ref.K_of's convention).  The host build of
quote_pool.h and the device are held to the same K.  `python tests/quote_out_precise_ref.py` prints the table.
"""
import math
import os

import numpy as np

import quote_precise_ref as F

ROOT = F.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "quote_out_precise.npz")
U = F.U
GROUPS, CURVE, family, next_pow2 = F.GROUPS, F.CURVE, F.family, F.next_pow2
MAX_INF_SHARE = 0.05

# worst ratio |a − a*| / (u·(R_i/γ + a* + cond)) of the numpy restatement per (family, class), finite rows; see K_of
K_MEASURED = {
    ('curve', 'alpha0'): 0.126,
    ('curve', 'huge'): 2.62e-10,
    ('curve', 'lopsided'): 0.144,
    ('curve', 'low_gamma'): 0.595,
    ('curve', 'near_drain'): 0.196,
    ('curve', 'o_gt_Ri'): 0.7,
    ('curve', 'small_a'): 0.0762,
    ('curve', 'stiff'): 0.384,
    ('curve', 'tiny'): 2.31e-11,
    ('curve', 'typical'): 0.577,
    ('geomean', 'huge'): 0.0893,
    ('geomean', 'lopsided'): 0.0432,
    ('geomean', 'low_gamma'): 0.124,
    ('geomean', 'near_drain'): 0.223,
    ('geomean', 'tiny'): 1.29e-12,
    ('geomean', 'typical'): 0.144,
    ('geomean', 'w02_98'): 0.257,
    ('product', 'huge'): 0,
    ('product', 'lopsided'): 0.182,
    ('product', 'low_gamma'): 0.0386,
    ('product', 'near_drain'): 0,
    ('product', 'tiny'): 1.77e-12,
    ('product', 'typical'): 0.135,
    ('solidly', 'balanced'): 0.154,
    ('solidly', 'huge'): 0,
    ('solidly', 'lopsided'): 0.00724,
    ('solidly', 'low_gamma'): 0.39,
    ('solidly', 'near_drain'): 0.191,
    ('solidly', 't0_hi'): 0.0493,
    ('solidly', 't0_lo'): 0.123,
    ('solidly', 'tiny'): 3.17e-12,
    ('solidly', 'typical'): 0.269,
    ('univ3', 'asymptotic'): 0,
    ('univ3', 'beyond'): 0,
    ('univ3', 'boundary_dn'): 0.254,
    ('univ3', 'boundary_up'): 0.254,
    ('univ3', 'closing_exact'): 0.234,
    ('univ3', 'depth1'): 0.149,
    ('univ3', 'depth4'): 0.0692,
    ('univ3', 'depth5'): 0.0969,
    ('univ3', 'depth64'): 0.0249,
    ('univ3', 'empty_current'): 0.0581,
    ('univ3', 'empty_in_path'): 0.0691,
    ('univ3', 'exhausted'): 0.234,
    ('univ3', 'in_tick'): 0.0136,
    ('univ3', 'last_tick'): 0.234,
    ('univ3', 'on_boundary'): 0.679,
    ('weighted', 'huge'): 0.202,
    ('weighted', 'lopsided'): 0.128,
    ('weighted', 'low_gamma'): 0.321,
    ('weighted', 'near_drain'): 0.246,
    ('weighted', 'pairs'): 0.0856,
    ('weighted', 'tiny'): 2.08e-12,
    ('weighted', 'typical'): 0.152,
    ('weighted', 'w02_98'): 0.294,
}
K_CAP_TYPICAL, K_CAP = F.K_CAP_TYPICAL, F.K_CAP


def K_of(group, cls):
    """K of a (family, class): next power of two >= 2x the restatement's worst ratio, at least 1, capped."""
    worst = K_MEASURED[(family(group), cls)]
    k = max(1, next_pow2(2.0 * worst))
    cap = K_CAP_TYPICAL if cls == "typical" else K_CAP
    assert k <= cap, f"{group}/{cls}: K = {k} exceeds the cap {cap}: a finding about the form, not a reason to raise the cap"
    return k


def load():
    z = np.load(FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files}


group = F.group


def ratios(a, g):
    """|a − a*| in units of u·(R_i/γ + a* + cond) per row; rows whose truth is +inf: 0 where a is +inf too, else +inf"""
    fin = np.isfinite(g["a"])
    r = np.where(np.asarray(a) == g["a"], 0.0, np.inf)
    with np.errstate(all="ignore"):
        r[fin] = np.abs(np.asarray(a)[fin] - g["a"][fin]) / (U * (g["scale"][fin] + g["a"][fin] + g["cond"][fin]))
    return np.where(np.isnan(r), np.inf, r)


# ---------------------------------------------------------------------------------------------------------------
# numpy restatement of the quote_out_* functions of csrc/quote_pool.h (same operation order, numpy's libm)
# ---------------------------------------------------------------------------------------------------------------
def qo_product(Ri, Ro, g, o):
    with np.errstate(all="ignore"):
        return np.where(o >= Ro, np.inf, (Ri * o) / ((Ro - o) * g))


def qo_weighted(Ri, Ro, wi, wo, g, o):
    with np.errstate(all="ignore"):
        a = (Ri * np.expm1(-((wo / wi) * np.log1p(-(o / Ro))))) / g
    return np.where(o == 0.0, 0.0, np.where(o >= Ro, np.inf, a))


def cubic(c):
    hc = 0.5 * c
    s = np.cbrt(hc + np.hypot(hc, 0.19245008972987526))
    u = s - 1.0 / (3.0 * s)
    for _ in range(2):
        uu = u * u
        u = u - (u * (uu + 1.0) - c) / (3.0 * uu + 1.0)
    return u


def qo_solidly(Ri, Ro, g, o):
    with np.errstate(all="ignore"):
        yp = Ro - o
        s0, r = Ri / Ro, Ro / yp
        r2 = r * r
        c = (s0 * (s0 * s0 + 1.0)) * (r2 * r2)
        x = cubic(c) * yp - Ri
        x = np.where(x < 0.0, 0.0, x)
        A, B = 3.0 * Ri, 3.0 * (Ri * Ri) + yp * yp
        Q = ((Ri * o) * ((Ri * Ri + Ro * Ro) + (Ro * yp + yp * yp))) / yp
        for _ in range(2):
            p = (x + A) * x + B
            x = x - (x * p - Q) / (p + x * (2.0 * x + A))
        a = np.where(x < 0.0, 0.0, x) / g
    return np.where(o == 0.0, 0.0, np.where(o >= Ro, np.inf, a))


def qo_curve(Ri, Ro, srho, alpha, lbeta, g, o):
    with np.errstate(all="ignore"):
        y = Ro - o
        P0 = np.exp(lbeta - srho)
        E = alpha * (Ri - o) + P0
        G = (Ri * o) * (alpha + P0 / y)
        h = np.hypot(E, 2.0 * (np.sqrt(alpha) * np.sqrt(G)))
        x = np.where(E < 0.0, (h - E) / (2.0 * alpha), (2.0 * G) / (E + h))
        a = x / g
    return np.where(o == 0.0, 0.0, np.where(o >= Ro, np.inf, a))


def _tick_inv(s_in, s_out, dmax, ot):
    d = (s_in * ot) / (s_out - ot) if s_out != ot else (math.inf if s_in * ot > 0 else math.nan)
    return 0.0 if d < 0.0 else (dmax if d > dmax else d)


def qo_univ3(prep, g, cin, o):
    """prep: quote_precise_ref.univ3_prepare's records (k, s_in, δmax, s_out, R_out, Σδmax, ΣR_out)"""
    cur, up, lo = prep
    if o == 0.0:
        return 0.0
    if o != o:
        return o
    k = cur[0]
    s_in, s_out = (cur[1], cur[2]) if cin == 0 else (cur[2], cur[1])
    dmax, rout = (cur[3], cur[6]) if cin == 0 else (cur[4], cur[5])
    if k != 0.0 and o < rout:
        return _tick_inv(s_in, s_out, dmax, o) / g
    lst = up if cin == 0 else lo
    cnt = len(lst) - 1
    lo_i, hi_i = 0, cnt + 1
    while hi_i - lo_i > 1:
        mid = lo_i + ((hi_i - lo_i) >> 1)
        if lst[mid][6] <= o:
            lo_i = mid
        else:
            hi_i = mid
    e = lst[lo_i]
    if lo_i == cnt:
        return e[5] / g if o == e[6] else (math.inf if o > e[6] else math.nan)
    return (e[5] + _tick_inv(e[1], e[3], e[2], o - e[6])) / g


def univ3_unit(prep, g, cin, o):
    """(scale, cond, ∂a/∂o) of one UniV3 exact-output quote in doubles, from the inverse walk ACTUALLY taken through the prepared
    records: the two sums of the module docstring (make_quote_out_golden.mp_inverse_walk forms the same in mpmath;
    tests/test_quote_out_precise_cpu.py holds this restatement to them).  The unit of the bound is u·(scale + a + cond).
    None where no finite input yields o."""
    cur, up, lo = prep
    recs = [(cur[0], cur[1], cur[3], cur[2], cur[6]) if cin == 0 else (cur[0], cur[2], cur[4], cur[1], cur[5])]
    recs = [r for r in recs if r[0] != 0.0] + [r[:5] for r in (up if cin == 0 else lo)[:-1]]   # (k, s_in, δmax, s_out, R_out)
    sd = sr = roots = routs = 0.0
    for k, s_in, dmax, s_out, rout in recs:
        if o - sr < rout:
            ot = o - sr
            d = s_in * ot / (s_out - ot)
            slope = k / (s_out - ot) ** 2 / g
            return (roots + s_in) / g, (sd + d) / g + roots / g + routs * slope + d / g + s_out * slope + o * slope, slope
        if not math.isfinite(dmax):
            return None
        sd, sr = sd + dmax, sr + rout
        roots, routs = roots + dmax + 2.0 * s_in, routs + s_out + (s_out - rout)   # k/β + s_in: δmax = k/β − s_in; s_out + β
    return None


def univ3_totals(prep, cin):
    """(Σδmax, ΣR_out) of the closing record of the direction, as the upload prepares them"""
    e = (prep[1] if cin == 0 else prep[2])[-1]
    return e[5], e[6]


def restatement(fx, gname):
    """the numpy forms over one group -> a [rows]"""
    g = group(fx, gname)
    if gname == "univ3":
        preps = [F.univ3_prepare(*F.univ3_pool(g, p)[:3]) for p in range(g["current_price"].size)]
        return np.array([qo_univ3(preps[p], float(g["pool_gamma"][p]), int(ci), float(o))
                         for p, ci, o in zip(g["pool"], g["cin"], g["o"])]), g
    rows = np.arange(g["o"].size)
    Ri, Ro = g["R"][rows, g["cin"]], g["R"][rows, g["cout"]]
    fam = family(gname)
    if fam == "product":
        a = qo_product(Ri, Ro, g["gamma"], g["o"])
    elif fam == "solidly":
        a = qo_solidly(Ri, Ro, g["gamma"], g["o"])
    elif fam in ("geomean", "weighted"):
        a = qo_weighted(Ri, Ro, g["w"][rows, g["cin"]], g["w"][rows, g["cout"]], g["gamma"], g["o"])
    else:
        a = qo_curve(Ri, Ro, F.sum_logs(g["R"]), g["alpha"], np.log(g["beta"]), g["gamma"], g["o"])
    return a, g


def worst_by_class(fx, answers=None):
    """{(family, class): worst ratio}; answers: {group: a} (default: the numpy restatement)"""
    worst = {}
    for gname in GROUPS:
        if answers is None:
            a, g = restatement(fx, gname)
        else:
            a, g = answers[gname], group(fx, gname)
        r = ratios(a, g)
        for c in np.unique(g["cls"]):
            key = (family(gname), str(c))
            worst[key] = max(worst.get(key, 0.0), float(np.max(r[g["cls"] == c])))
    return worst


if __name__ == "__main__":
    w = worst_by_class(load())
    for key in sorted(w):
        print(f"    {key!r}: {w[key]:.3g},")
