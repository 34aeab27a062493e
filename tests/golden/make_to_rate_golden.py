"""Writes tests/golden/to_rate_precise.npz: for every pool and coin pair of tests/golden/quote_precise.npz and a ladder of limits
r (doubles), the amount a >= 0 at which the pool's marginal rate has fallen to r -- an 80-digit truth stored as the nearest
double -- with the two conditioning sums of tests/to_rate_precise_ref.py per row.

The truth does not use the project's closed forms.  Reserve families: rate(a) = γ·(∂φ/∂R_in)/(∂φ/∂R_out) at the state the
trade leaves, the partial derivatives taken numerically (mp.diff) of φ ITSELF (weighted pools: of log φ) at the root y′ of
φ(R + γa·e_in, R_out := y′) = φ(R), and a solves rate(a) = r.  Both roots are found by a bracketed Illinois iteration in mpmath;
where an iteration STARTS (the numpy restatement's double) has no bearing on where it ends, and every root is CERTIFIED, or the script
fails: φ changes sign across y′(1 ± 1e-70), and rate − r changes sign across a(1 ± 1e-60) (the rate is monotone).  The truth
is exactly 0 where the 80-digit spot rate is <= r.
UniV3: the reference's ticks in mpmath (make_rate_golden.mp_records); inside a tick φ = x·y, so the rate γ·y′/x′ = γk/x′² falls
to r at x′ = √(γk/r); the walk picks the tick whose rate range holds r, the boundary in front of an empty tick's range, or
the direction's capacity.
The closed forms of make_rate_golden.py appear here, in mpmath, for one thing only: the conditioning sums (the implicit
function theorem on rate(inputs, a) = r).

Limits per pool and pair, s the 80-digit spot rate's double (the a = 0 rows of rate_precise.npz):
    r/s in {1 − 2^-40, 0.999, 0.9, 0.5, 1e-3, 1e-9}      the ladder
    r/s in {1 + 2^-40, 2}                                truth exactly 0 (a quarter of the rows)
No row is emitted whose resulting state cfmm_pools_set_* would refuse (a reserve not finite and > 0 as a double; an amount
that overflows).  UniV3 in addition, per pool and direction, where the ladder has them: a limit in the middle (geometric) of the
rate range of the record at depth 1, 4, 5, 64 and of the last one, a limit at a live boundary's rate, in an empty tick's range,
and below the end of the last tick (the capacity).  Classes: the quote fixture's class of the pool (reserve families); UniV3
by where the limit lands.
usage: python tests/golden/make_to_rate_golden.py        (needs mpmath; deterministic: no random numbers)"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_quote_golden as Q  # noqa: E402
import make_rate_golden as RG  # noqa: E402
import quote_precise_ref as P  # noqa: E402
import rate_precise_ref as RP  # noqa: E402
import to_rate_precise_ref as TP  # noqa: E402

mp.mp.dps = 120   # 80 digits of truth and guard digits: R_in + γa must resolve a(1 ± 1e-60) where a is 1e-22 of R_in
M = mp.mpf
TEN = M(10)
CLASSES = RG.CLASSES
OUT = os.path.join(HERE, "to_rate_precise.npz")
LADDER = [1.0 - 2.0 ** -40, 0.999, 0.9, 0.5, 1e-3, 1e-9]
ABOVE = [1.0 + 2.0 ** -40, 2.0]


def bracketed(f, x0, tol, floor=None):
    """the root of a monotone f near x0 > 0: a bracket [x0/(1 + δ), x0(1 + δ)] widened from δ = 1e-13 by factors of 100 until f changes
    sign across it (never below `floor`), then the Illinois iteration on the bracket until it is tol of the root"""
    d = TEN ** -13
    for _ in range(40):
        lo, hi = x0 / (1 + d), x0 * (1 + d)
        if floor is not None and lo < floor:
            lo = floor
        flo, fhi = f(lo), f(hi)
        if flo == 0:
            return lo
        if fhi == 0:
            return hi
        if (flo > 0) != (fhi > 0):
            break
        d *= 100
    else:
        raise AssertionError(("no bracket", mp.nstr(x0, 20)))
    side = 0
    for _ in range(400):
        c = hi - fhi * (hi - lo) / (fhi - flo)
        if not lo < c < hi:
            c = (lo + hi) / 2
        fc = f(c)
        if fc == 0:
            return c
        if (fc > 0) == (flo > 0):
            lo, flo = c, fc
            if side == -1:
                fhi /= 2
            side = -1
        else:
            hi, fhi = c, fc
            if side == 1:
                flo /= 2
            side = 1
        if hi - lo <= tol * hi:
            break
    return (lo + hi) / 2


def certified_root(f, x, eps, what):
    """x with a sign change of f across x(1 ± eps), or the script fails"""
    lo, hi = f(x * (1 - eps)), f(x * (1 + eps))
    assert (lo > 0) != (hi > 0) or lo == 0 or hi == 0, (what, mp.nstr(x, 30), mp.nstr(lo, 10), mp.nstr(hi, 10))
    return x


def state_after(phi, Rm, k0, g, cin, cout, a, y0):
    """the reserves the trade of a leaves: R_in + γa and the certified root y′ of φ = φ(R) in R_out, started from y0"""
    Rn = list(Rm)
    Rn[cin] = Rm[cin] + g * a

    def f(y):
        Rn[cout] = y
        return phi(Rn) - k0
    y = bracketed(f, y0, TEN ** -76)
    assert y > 0, ("y'", mp.nstr(y, 20))
    certified_root(f, y, TEN ** -70, "y'")
    Rn[cout] = y
    return Rn


def rate_at(phi, Rm, k0, g, cin, cout, a, y0):
    """(γ·φ_in/φ_out at the state a leaves, y′)"""
    Rn = state_after(phi, Rm, k0, g, cin, cout, a, y0)

    def partial(j):   # as make_rate_golden.rate_truth: a step relative to R_j
        return mp.diff(lambda t: phi([Rn[k] * mp.exp(t) if k == j else Rn[k] for k in range(len(Rn))]), M(0)) / Rn[j]
    return g * partial(cin) / partial(cout), Rn[cout]


def family_of(g, fam, r):
    """(phi, closed form of the rate, its arguments [.., a last], the indices of the arguments that are inputs, a weight
    function for the Curve logs or None) of fixture row r"""
    R, ci, co = g["R"][r], int(g["cin"][r]), int(g["cout"][r])
    Rm = [M(float(x)) for x in R]
    gam = M(float(g["gamma"][r]))
    if fam == "product":
        return (lambda RR: RR[ci] * RR[co]), RG.cf_product, [Rm[ci], Rm[co], gam], None, Rm
    if fam == "solidly":
        return Q.phi_solidly, RG.cf_solidly, [Rm[ci], Rm[co], gam], None, Rm
    if fam in ("geomean", "weighted"):
        wm = [M(float(x)) for x in g["w"][r]]
        return (lambda RR: Q.phi_weighted(RR, wm)), RG.cf_weighted, [Rm[ci], Rm[co], wm[ci], wm[co], gam], None, Rm
    al, be = M(float(g["alpha"][r])), M(float(g["beta"][r]))
    pr = M(1)
    for x in Rm:
        pr *= x
    lP0 = mp.log(be / pr)
    logs = abs(mp.log(be)) + sum(abs(mp.log(x)) for x in Rm)
    return (lambda RR: Q.phi_curve(RR, al, be)), RG.cf_curve, [Rm[ci], Rm[co], al, lP0, gam], (3, logs), Rm


def conds(cf, xs, logs, a, r):
    """(cond of a, cond of the rate) at the truth: Σ_j |x_j ∂rate/∂x_j| over the inputs (the Curve logs by their own weight),
    S; |∂rate/∂a| = D.  cond_a = (S + r)/D, rcond = S + a·D"""
    S = M(0)
    full = xs + [a]
    for j, xj in enumerate(xs):
        d = mp.diff(lambda t, j=j: cf(*[t if k == j else full[k] for k in range(len(full))]), xj)
        if logs is not None and j == logs[0]:
            S += logs[1] * abs(d)
        elif xj != 0:
            S += abs(xj * d)
    D = abs(mp.diff(lambda t: cf(*(xs + [t])), a)) if a != 0 else abs(mp.diff(lambda t: cf(*(xs + [t])), a, direction=1))
    # (a balanced Solidly pair at a = 0: ∂rate/∂a = 0, the amount is infinitely ill-conditioned in the limit)
    return ((S + r) / D if D != 0 else mp.inf), S + a * D


def storable(x):
    return np.isfinite(float(x)) and float(x) > 0.0


def make_reserve_group(fxs, out, name, approx):
    """approx: the numpy restatement's amounts for the rows emitted so far are not known yet, so the start is found here"""
    qfx, rfx = fxs
    g = P.group(qfx, name)
    rg = RP.group((qfx, rfx), name)
    fam = P.family(name)
    n = g["a"].size
    spot = rg["rate"][n:]                      # the a = 0 rows: the 80-digit spot rate's double, per fixture row
    rows = []
    for r in range(n):
        phi, cf, xs, logs, Rm = family_of(g, fam, r)
        ci, co, gam = int(g["cin"][r]), int(g["cout"][r]), xs[-1]
        k0 = phi(Rm)
        s_true, _ = rate_at(phi, Rm, k0, gam, ci, co, M(0), Rm[co])
        assert abs(float(s_true) - spot[r]) <= 2.0 ** -52 * spot[r], (name, r, float(s_true), spot[r])
        for ratio in LADDER + ABOVE:
            rd = float(spot[r]) * ratio
            rm = M(rd)
            what = (name, r, ratio)
            if s_true <= rm:
                assert ratio > 1.0, what
                ca, cr = conds(cf, xs, logs, M(0), rm)
                rows.append((r, rd, 0.0, float(ca), float(cr), False))
                continue
            assert ratio < 1.0, what
            a0 = M(float(approx(g, fam, r, rd)))
            assert a0 > 0 and mp.isfinite(a0), what
            state = {"y": None}

            def f(a):
                if state["y"] is None:   # the first y′: from φ alone, by bisection (make_rate_golden.state_root)
                    state["y"] = RG.state_root(phi, g["R"][r], float(gam), ci, co, float(a))[0]
                rate, y = rate_at(phi, Rm, k0, gam, ci, co, a, state["y"])
                state["y"] = y
                return rate - rm
            a = bracketed(f, a0, TEN ** -70)
            assert a > 0, what
            certified_root(f, a, TEN ** -60, what)
            Rn = state_after(phi, Rm, k0, gam, ci, co, a, state["y"])
            if not (storable(a) and storable(Rn[ci]) and storable(Rn[co])):
                continue                        # a state cfmm_pools_set_* would refuse: no row
            ca, cr = conds(cf, xs, logs, a, rm)
            rows.append((r, rd, float(a), float(ca), float(cr), True))
    out[f"{name}_row"] = np.array([x[0] for x in rows], dtype=np.int64)
    out[f"{name}_r"] = np.array([x[1] for x in rows])
    out[f"{name}_a"] = np.array([x[2] for x in rows])
    out[f"{name}_cond"] = np.array([x[3] for x in rows])
    out[f"{name}_rcond"] = np.array([x[4] for x in rows])
    out[f"{name}_interior"] = np.array([x[5] for x in rows], dtype=np.bool_)
    out[f"{name}_cls"] = np.array([CLASSES.index(str(g["cls"][x[0]])) for x in rows], dtype=np.int32)
    return len(rows)


def approx_amount(g, fam, r, rd):
    """the numpy restatement's amount for row r of the quote fixture's group at limit rd: where the secant starts"""
    F = np.float64
    ci, co = int(g["cin"][r]), int(g["cout"][r])
    Ri, Ro, gam = F(g["R"][r, ci]), F(g["R"][r, co]), F(g["gamma"][r])
    with np.errstate(all="ignore"):
        if fam == "product":
            return TP.t_product(Ri, Ro, gam, F(rd))
        if fam == "solidly":
            return TP.t_solidly(Ri, Ro, gam, F(rd))
        if fam in ("geomean", "weighted"):
            return TP.t_weighted(Ri, Ro, F(g["w"][r, ci]), F(g["w"][r, co]), gam, F(rd))
        return TP.t_curve(Ri, Ro, P.sum_logs(g["R"][r:r + 1])[0], F(g["alpha"][r]), np.log(F(g["beta"][r])), gam, F(rd))[0]


# ---- UniV3 ----------------------------------------------------------------------------------------------------------
def univ3_truth(recs, gam, rm):
    """-> (a, cond, rcond, kind, depth) for limit rm over the records (k, s_in, s_out, δmax, R_out) of the direction, the
    current tick first; kind: zero / interior / boundary / gap / capacity"""
    S, drained = M(0), M(0)
    for e, (k, s_in, s_out, dmax, rout) in enumerate(recs):
        start = gam * k / s_in ** 2
        end = gam * k / (s_in + dmax) ** 2 if dmax != mp.inf else M(0)
        if rm >= start:   # the limit lies in front of this record: at the spot (e = 0), or in an empty tick's range
            kind = "zero" if e == 0 else "gap"
            return S / gam, (drained + S) / gam, M(0), kind, e
        if rm > end:
            q = mp.sqrt(gam * k / rm)
            d = q - s_in
            a = (S + d) / gam
            cond = (q + s_in + drained + abs(S - s_in + q / 2)) / gam
            ga = gam * a
            rcond = rm * (1 + abs(1 - 2 * ga / q) + 2 * (ga + s_in + drained) / q)
            return a, cond, rcond, "interior", e
        S += dmax
        drained += dmax + 2 * s_in
    return S / gam, (drained + S) / gam, M(0), "capacity", len(recs)


def make_univ3(fxs, out):
    qfx, rfx = fxs
    g = P.group(qfx, "univ3")
    rg = RP.group((qfx, rfx), "univ3")
    npools = g["current_price"].size
    rows = []
    for p in range(npools):
        cp, lt, lq, gamd = P.univ3_pool(g, p)
        gam = M(gamd)
        for ci in (0, 1):
            recs = RG.mp_records(cp, lt, lq, ci)
            if not recs:
                continue
            sel = (rg["cls"] == "spot") & (rg["pool"] == p) & (rg["cin"] == ci)
            s = float(rg["rate"][sel][0])
            empty_current = Q.mp_ticks(cp, lt, lq)[0][Q.mp_ticks(cp, lt, lq)[1]][0] == 0
            limits = [(s * x, None) for x in LADDER + ABOVE]
            starts = [gam * k / s_in ** 2 for k, s_in, _, _, _ in recs]
            ends = [gam * k / (s_in + dm) ** 2 if dm != mp.inf else M(0) for k, s_in, _, dm, _ in recs]
            for depth in (1, 4, 5, 64, len(recs) - 1):
                if 0 < depth < len(recs) and ends[depth] > 0:
                    limits.append((float(mp.sqrt(starts[depth] * ends[depth])), None))
                elif 0 < depth < len(recs):
                    limits.append((float(starts[depth] / 2), None))
            for e in range(1, len(recs)):
                if ends[e - 1] <= starts[e] * (1 + M(2) ** -30):
                    limits.append((float(starts[e]), "boundary"))      # a live boundary: the first one
                    break
            for e in range(1, len(recs)):
                if ends[e - 1] > starts[e] * (1 + M(2) ** -20):
                    limits.append((float(mp.sqrt(ends[e - 1] * starts[e])), None))   # inside an empty tick's range: the first one
                    break
            if ends[-1] > 0:
                limits.append((float(ends[-1] / 2), None))             # below the last tick's end: the capacity
            for rd, tag in limits:
                rm = M(rd)
                a, cond, rcond, kind, e = univ3_truth(recs, gam, rm)
                if tag == "boundary":
                    # the double nearest a boundary's rate lies a rounding to either side of it: both sides answer the
                    # boundary's amount to that rounding, which cond covers; not an interior row
                    kind = "boundary"
                if not np.isfinite(float(a)):
                    continue
                if kind == "zero":
                    cls = "spot"
                elif kind == "capacity":
                    cls = "exhausted"
                elif kind == "gap":
                    cls = "empty_in_path"
                elif kind == "boundary":
                    cls = "boundary_dn" if ci == 0 else "boundary_up"
                elif empty_current and e == 0:
                    cls = "empty_current"
                elif e == 0:
                    cls = "in_tick"
                elif e == len(recs) - 1:
                    cls = "last_tick"
                else:
                    cls = "depth1" if e == 1 else ("depth4" if e <= 4 else ("depth5" if e < 32 else "depth64"))
                rows.append((p, ci, rd, float(a), float(cond), float(rcond), kind == "interior", kind == "zero", kind == "capacity", cls))
    out["univ3_pool"] = np.array([x[0] for x in rows], dtype=np.int64)
    out["univ3_cin"] = np.array([x[1] for x in rows], dtype=np.int32)
    out["univ3_r"] = np.array([x[2] for x in rows])
    out["univ3_a"] = np.array([x[3] for x in rows])
    out["univ3_cond"] = np.array([x[4] for x in rows])
    out["univ3_rcond"] = np.array([x[5] for x in rows])
    out["univ3_interior"] = np.array([x[6] for x in rows], dtype=np.bool_)
    out["univ3_zero"] = np.array([x[7] for x in rows], dtype=np.bool_)
    out["univ3_capacity"] = np.array([x[8] for x in rows], dtype=np.bool_)
    out["univ3_cls"] = np.array([CLASSES.index(x[9]) for x in rows], dtype=np.int32)
    print("univ3 classes:", sorted(set(x[9] for x in rows)))
    return len(rows)


def main():
    fxs = RP.load()
    out = {"classes": np.array(CLASSES)}
    sizes = {}
    only = sys.argv[1:]
    for name in P.GROUPS:
        if only and name not in only:
            continue
        sizes[name] = make_univ3(fxs, out) if name == "univ3" else make_reserve_group(fxs, out, name, approx_amount)
        print(name, sizes[name], flush=True)
    if only:   # a dry run of some groups: nothing is written
        return
    total = sum(sizes.values())
    zeros = sum(int(np.sum(out[f"{n}_a"] == 0.0)) for n in sizes)
    assert 8 * zeros >= total, (zeros, total)
    RG.save(OUT, out)
    print(OUT, os.path.getsize(OUT), "bytes;", sizes, "truth 0:", zeros)


if __name__ == "__main__":
    main()
