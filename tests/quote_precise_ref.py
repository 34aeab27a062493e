"""Exact-input swap quotes against a 60-digit truth: the fixture's loader, the bound, the K table and a numpy restatement
of the forms of csrc/quote_pool.h (the instrument K was measured with).  No device, no library: plain numpy.

The truth (tests/golden/make_quote_golden.py -> tests/golden/quote_precise.npz) does not use the project's arithmetic: per
row it is the root `out` of the defining equation φ(R + γ·a·e_in − out·e_out) = φ(R), found by mpmath's bracketing root
finder on φ itself at 80 digits (UniV3: the reference's tick-by-tick walk, src/cfmms.jl:401-434, in mpmath from the pool's
ladder), stored as the nearest double.

The bound.  Every quote function is a short composition of correctly rounded operations and library functions good to
about an ulp, applied to the state AS THE DEVICE HOLDS IT: inputs x_j that are themselves roundings (each off by up to
u = 2^-53 relative, several for a prepared constant).  First-order error propagation gives
    |out − out*|  <=  K·u·( R_o  +  out*  +  Σ_j |x_j · ∂out/∂x_j| )
where R_o covers a final subtraction from the output reserve (Solidly forms R_o − u·x′), out* the rounding of the result
and its last operations, and the conditioning sum what a relative perturbation u of every input does to the result.  K
counts the roundings per input and the library functions' ulps; it is measured (below), not derived.  The inputs are
    Product, Solidly   R_i, R_o, γ, a
    weighted           R_i, R_o, w_i, w_o, γ, a
    Curve              R_i, R_o, α, γ, a, and the LOGS the device holds: log β and every log R_k enter through
                       P₀ = exp(log β − Σ log R_k), so with g = ∂out/∂log P₀ their share is (|log β| + Σ_k |log R_k|)·|g|
    UniV3              a, γ, and per tick the prepared constants (csrc/univ3_pool.h): a drained tick contributes
                       R_out = √(k·p) − β, conditioned by s_out + β (the two roots it is the difference of); the landing
                       tick s_out − k/(s_in + d) with d = γa − Σδmax, conditioned by s_out + k/(s_in + d) and by
                       (s_in + 2γa + Σ_j (k_j/β_j + s_in,j))·k/(s_in + d)²; R_o is ΣR_out walked + R_out of the landing tick.
The conditioning sum is computed from the truth's side (mpmath, exact inputs) and stored per row as `cond`.

K per class: the numpy restatement below is run over the fixture on the CPU; K is the next power of two >= 2x its worst
ratio in the class, capped at 16 on `typical` and 64 elsewhere (the project's convention: DESIGN §3.0c,
tests/test_curve_precise_cpu.py).  The host build of quote_pool.h and the device are held to the same K.
Measured worst ratios of the restatement (python tests/quote_precise_ref.py prints them) are in K_MEASURED.
"""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "quote_precise.npz")
U = 2.0 ** -53

TWO_COIN = ("product", "solidly", "geomean")
WEIGHTED = ("weighted2", "weighted3", "weighted8")
CURVE = ("curve2", "curve3", "curve4")
GROUPS = TWO_COIN + WEIGHTED + CURVE + ("univ3",)

# worst ratio |out − out*| / (u·(R_o + out* + cond)) of the numpy restatement per (family, class); see K_of
K_MEASURED = {
    ('curve', 'alpha0'): 0.132,
    ('curve', 'huge'): 0.638,
    ('curve', 'lopsided'): 1.27,
    ('curve', 'low_gamma'): 0.598,
    ('curve', 'small_a'): 0.134,
    ('curve', 'stiff'): 0.392,
    ('curve', 'tiny'): 2.72e-11,
    ('curve', 'typical'): 0.424,
    ('geomean', 'huge'): 0,
    ('geomean', 'lopsided'): 0.0258,
    ('geomean', 'low_gamma'): 0.182,
    ('geomean', 'tiny'): 2.36e-12,
    ('geomean', 'typical'): 0.163,
    ('geomean', 'w02_98'): 0.0416,
    ('product', 'huge'): 0,
    ('product', 'lopsided'): 0.0857,
    ('product', 'low_gamma'): 0.175,
    ('product', 'tiny'): 1.44e-12,
    ('product', 'typical'): 0.0187,
    ('solidly', 'balanced'): 1.47,
    ('solidly', 'huge'): 0,
    ('solidly', 'lopsided'): 1.89,
    ('solidly', 'low_gamma'): 1.13,
    ('solidly', 't0_hi'): 1.16,
    ('solidly', 't0_lo'): 1.78,
    ('solidly', 'tiny'): 3.07,
    ('solidly', 'typical'): 1.67,
    ('univ3', 'boundary_dn'): 0.507,
    ('univ3', 'boundary_up'): 0.178,
    ('univ3', 'depth1'): 0.193,
    ('univ3', 'depth4'): 0.203,
    ('univ3', 'depth5'): 0.164,
    ('univ3', 'depth64'): 0.0329,
    ('univ3', 'empty_current'): 0.182,
    ('univ3', 'empty_in_path'): 0.197,
    ('univ3', 'exhausted'): 0.494,
    ('univ3', 'in_tick'): 0.734,
    ('univ3', 'last_tick'): 0,
    ('weighted', 'huge'): 0,
    ('weighted', 'lopsided'): 0.266,
    ('weighted', 'low_gamma'): 0.171,
    ('weighted', 'pairs'): 0.134,
    ('weighted', 'tiny'): 3.78e-11,
    ('weighted', 'typical'): 0.168,
    ('weighted', 'w02_98'): 0.044,
}
K_CAP_TYPICAL, K_CAP = 16, 64
# oracle.UniV3.forward_trade (the reference's sequential walk in doubles) against the same truth over the fixture's UniV3
# rows, same units (tests/test_quote_precise_cpu.py measures it); the GPU comparison with the oracle allows the device's K
# plus ORACLE_UNIV3_K = the next power of two >= 2x this, because two correct roundings can differ by their sum
ORACLE_UNIV3_WORST = 0.734
ORACLE_UNIV3_K = 2


def family(group):
    return group if group == "univ3" else group.rstrip("0123456789")


def next_pow2(x):
    return 1 if x <= 1 else 2 ** int(math.ceil(math.log2(x)))


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


def group(fx, g):
    """the arrays of one group, prefix stripped; `cls` as class names"""
    out = {k[len(g) + 1:]: v for k, v in fx.items() if k.startswith(g + "_")}
    names = [str(s) for s in fx["classes"]]
    out["cls"] = np.array([names[c] for c in out["cls"]])
    return out


def bound(K, scale, out_true, cond):
    return K * U * (scale + out_true + cond)


def ratios(out, g):
    """|out − out*| in units of u·(R_o + out* + cond), per row"""
    return np.abs(out - g["out"]) / (U * (g["scale"] + g["out"] + g["cond"]))


# ---------------------------------------------------------------------------------------------------------------
# numpy restatement of csrc/quote_pool.h (same operation order, numpy's libm)
# ---------------------------------------------------------------------------------------------------------------
def q_product(Ri, Ro, g, a):
    x = g * a
    return Ro * (x / (Ri + x))


def q_weighted(Ri, Ro, wi, wo, g, a):
    x = g * a
    return Ro * (0.0 - np.expm1(-((wi / wo) * np.log1p(x / Ri))))


def q_solidly(Ri, Ro, g, a):
    x = g * a
    xp = Ri + x
    t0, r = Ro / Ri, Ri / xp
    r2 = r * r
    c = (t0 * (t0 * t0 + 1.0)) * (r2 * r2)
    hc = 0.5 * c
    s = np.cbrt(hc + np.hypot(hc, 0.19245008972987526))
    u = s - 1.0 / (3.0 * s)
    for _ in range(2):
        uu = u * u
        u = u - (u * (uu + 1.0) - c) / (3.0 * uu + 1.0)
    out = Ro - u * xp
    return np.where(a == 0.0, 0.0, np.maximum(out, 0.0))


def q_curve(Ri, Ro, srho, alpha, lbeta, g, a):
    x = g * a
    xp = Ri + x
    P0 = np.exp(lbeta - srho)
    C = alpha * (Ro - x) - P0
    B = (P0 * Ro) * (Ri / xp)
    h = np.hypot(C, 2.0 * (np.sqrt(alpha) * np.sqrt(B)))
    E = alpha * (Ro + x) + P0
    G = (Ro * x) * (alpha + P0 / xp)
    return (2.0 * G) / (E + h)


def sum_logs(R):
    """Σ_k log R_k in coin order, as the kernel adds the uploaded logs"""
    s = np.zeros(R.shape[0])
    for k in range(R.shape[1]):
        s = s + np.log(R[:, k])
    return s


def univ3_prepare(cp, lt, lq):
    """One pool's records as csrc/univ3_pool.h prepares them (IEEE doubles, the same operation order):
    -> cur = (k, sA, sB, dmax0, dmax1, R1, R2), up, lo: lists of (k, s_in, dmax, s_out, rout, Σδmax, ΣR_out), each closed
    by a record that carries only the sums."""
    lt, lq = [float(x) for x in lt], [float(x) for x in lq]
    nt = len(lt)
    ct = 0
    for j in range(nt):                      # searchsortedlast(lower_ticks, cp, rev=true), 1-based
        if lt[j] >= cp:
            ct = j + 1
    sq = math.sqrt

    def at(idx):
        k, pp = lq[idx - 1], lt[idx - 1]
        pm = lt[idx] if idx < nt else 0.0
        al, be = sq(k / pp), sq(k * pm)
        p = pp if idx > ct else (pm if idx < ct else cp)
        return k, al, be, sq(k / p) - al, sq(k * p) - be

    def div(a, b):
        return a / b if b != 0.0 else (math.inf if a > 0 else math.nan)

    k, al, be, R1, R2 = at(ct)
    sA, sB = R1 + al, R2 + be
    d0, d1 = div(k, be) - sA, div(k, al) - sB
    if k == 0:
        d0 = d1 = 0.0
    cur = (k, sA, sB, d0, d1, R1, R2)
    up, run = [], ((d0, R2) if k != 0 else (0.0, 0.0))
    for idx in range(ct + 1, nt + 1):
        kk, al, be, R1, R2 = at(idx)
        if kk == 0:
            continue
        s_in = R1 + al
        dm = div(kk, be) - s_in
        up.append((kk, s_in, dm, R2 + be, R2, run[0], run[1]))
        run = (run[0] + dm, run[1] + R2)
    up.append((0.0, 0.0, 0.0, 0.0, 0.0, run[0], run[1]))
    lo, run = [], ((d1, cur[5]) if k != 0 else (0.0, 0.0))
    for idx in range(ct - 1, 0, -1):
        kk, al, be, R1, R2 = at(idx)
        if kk == 0:
            continue
        s_in = R2 + be
        dm = div(kk, al) - s_in
        lo.append((kk, s_in, dm, R1 + al, R1, run[0], run[1]))
        run = (run[0] + dm, run[1] + R1)
    lo.append((0.0, 0.0, 0.0, 0.0, 0.0, run[0], run[1]))
    return cur, up, lo


def _tick(k, s_in, s_out, rout, d):
    l = s_out - k / (s_in + d)
    return 0.0 if l < 0.0 else (rout if l > rout else l)


def q_univ3(prep, g, cin, a):
    cur, up, lo = prep
    d = g * a
    if a == 0.0:
        return 0.0
    k = cur[0]
    s_in, s_out = (cur[1], cur[2]) if cin == 0 else (cur[2], cur[1])
    dmax, rout = (cur[3], cur[6]) if cin == 0 else (cur[4], cur[5])
    if k != 0.0 and d < dmax:
        return _tick(k, s_in, s_out, rout, d)
    lst = up if cin == 0 else lo
    cnt = len(lst) - 1
    lo_i, hi_i = 0, cnt + 1
    while hi_i - lo_i > 1:
        mid = lo_i + ((hi_i - lo_i) >> 1)
        if lst[mid][5] <= d:
            lo_i = mid
        else:
            hi_i = mid
    e = lst[lo_i]
    if lo_i == cnt:
        return e[6]
    return e[6] + _tick(e[0], e[1], e[3], e[4], d - e[5])


def univ3_unit(prep, g, cin, a):
    """(scale, cond) of one UniV3 quote in doubles, from the walk ACTUALLY taken through the prepared records: scale = ΣR_out
    walked + R_out of the landing tick, cond = the conditioning sum of the module docstring (make_quote_golden.mp_walk forms the
    same two in mpmath; tests/test_quote_precise_cpu.py holds this restatement to them).  The unit of the bound is
    u·(scale + out + cond)."""
    cur, up, lo = prep
    d = g * a
    recs = [(cur[0], cur[1], cur[3], cur[2], cur[6]) if cin == 0 else (cur[0], cur[2], cur[4], cur[1], cur[5])]
    recs = [r for r in recs if r[0] != 0.0] + [r[:5] for r in (up if cin == 0 else lo)[:-1]]   # (k, s_in, δmax, s_out, R_out)
    scale = cond = drained = 0.0
    for k, s_in, dmax, s_out, rout in recs:
        if dmax > d:
            rate = k / (s_in + d) ** 2
            return scale + rout, cond + s_out + k / (s_in + d) + (s_in + 2.0 * g * a + drained) * rate
        scale += rout
        cond += s_out + (s_out - rout)            # s_out + β: R_out = s_out − β
        drained += dmax + 2.0 * s_in              # k/β + s_in: δmax = k/β − s_in
        d -= dmax
    return scale, cond


def univ3_pool(g, p):
    """(current_price, lower_ticks, liquidity, gamma) of pool p of the univ3 group"""
    a, b = int(g["tick_off"][p]), int(g["tick_off"][p + 1])
    return float(g["current_price"][p]), g["lower_ticks"][a:b], g["liquidity"][a:b], float(g["pool_gamma"][p])


def restatement(fx, gname):
    """the numpy forms over one group -> out [rows]"""
    g = group(fx, gname)
    if gname == "univ3":
        preps = [univ3_prepare(*univ3_pool(g, p)[:3]) for p in range(g["current_price"].size)]
        return np.array([q_univ3(preps[p], float(g["pool_gamma"][p]), int(ci), float(a))
                         for p, ci, a in zip(g["pool"], g["cin"], g["a"])]), g
    rows = np.arange(g["a"].size)
    Ri, Ro = g["R"][rows, g["cin"]], g["R"][rows, g["cout"]]
    fam = family(gname)
    with np.errstate(all="ignore"):
        if fam == "product":
            out = q_product(Ri, Ro, g["gamma"], g["a"])
        elif fam == "solidly":
            out = q_solidly(Ri, Ro, g["gamma"], g["a"])
        elif fam in ("geomean", "weighted"):
            out = q_weighted(Ri, Ro, g["w"][rows, g["cin"]], g["w"][rows, g["cout"]], g["gamma"], g["a"])
        else:
            out = q_curve(Ri, Ro, sum_logs(g["R"]), g["alpha"], np.log(g["beta"]), g["gamma"], g["a"])
    return out, g


def worst_by_class(fx, outputs=None):
    """{(family, class): worst ratio}; outputs: {group: out} (default: the numpy restatement)"""
    worst = {}
    for gname in GROUPS:
        if outputs is None:
            out, g = restatement(fx, gname)
        else:
            out, g = outputs[gname], group(fx, gname)
        r = ratios(out, g)
        for c in np.unique(g["cls"]):
            key = (family(gname), str(c))
            worst[key] = max(worst.get(key, 0.0), float(np.max(r[g["cls"] == c])))
    return worst


if __name__ == "__main__":
    w = worst_by_class(load())
    for key in sorted(w):
        print(f"    {key!r}: {w[key]:.3g},")
