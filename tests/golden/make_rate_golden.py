"""Writes tests/golden/rate_precise.npz: the marginal rate of every exact-input quote of tests/golden/quote_precise.npz -- its
pools and queries, all ten groups, every class -- with an 80-digit truth (stored as the nearest double) and the conditioning
sum of tests/rate_precise_ref.py per row.  Every row appears a second time with a = 0 (the spot rate); UniV3 instead gets one
a = 0 row per pool and direction (class `spot`: every fixture pool has its current price well inside its tick, or an empty
current tick, so the right derivative at 0 is unambiguous).

The truth does not use the project's closed forms: rate = γ·(∂φ/∂R_in)/(∂φ/∂R_out) at R′ = R + γa·e_in − out·e_out, the
partial derivatives taken numerically (mp.diff) of φ ITSELF (weighted pools: of log φ), `out` the 80-digit root that
make_quote_golden.py finds by bisection on φ.  UniV3: the reference's tick-by-tick walk in mpmath; in the tick the amount
lands in, φ = x·y, so the rate is γ·y′/x′ at the state the walk leaves that tick in.
INDEPENDENT CHECK, or the script fails: a central difference of the 80-digit quote at h = a·1e-20 -- at a = 0 the one-sided
five-point forward difference (error O(h⁴)), h = 1e-20·R_i (UniV3: 1e-20·s_in) -- agrees with `rate` to 30 digits.
UniV3 rows flagged `at_boundary` (the exact δ′ = γa within 2^-40 relative of a Σδmax) are exempt; there `rate` is the rate
at the start of the tick behind the boundary, `rate_left` the rate at the end of the tick in front of it, each with its own
conditioning sum, and a test accepts whichever is nearer.  The flagged rows must be the 10 rows of the classes boundary_dn /
boundary_up and no others (asserted).
The closed forms appear here, in mpmath, for two things only: a cross-check of every rate (1e-30), and the conditioning sum.
usage: python tests/golden/make_rate_golden.py        (needs mpmath; deterministic: no random numbers)"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_quote_golden as Q  # noqa: E402
import quote_precise_ref as P  # noqa: E402

mp.mp.dps = 80
M = mp.mpf
CLASSES = Q.CLASSES + ["spot"]
OUT = os.path.join(HERE, "rate_precise.npz")
TEN = M(10)


def agree(a, b, digits, what):
    assert abs(a - b) <= TEN ** -digits * max(abs(a), abs(b)), (what, mp.nstr(a, 40), mp.nstr(b, 40))


# ---- the truth: implicit differentiation of φ at the root ------------------------------------------------------------
def state_root(phi, R, g, cin, cout, a):
    """y′ = R_o − out, the reserve the trade leaves: the root in (0, R_o] of φ(R + γa·e_in with R_out := y) = φ(R), by bisection
    on φ itself until the bracket is 1e-72 of the ROOT (φ is increasing in every reserve).  make_quote_golden.py brackets `out`;
    after a large trade y′ is far below the last digit of such an `out`, and the rate is proportional to y′."""
    Rm = [M(float(x)) for x in R]
    k0 = phi(Rm)
    Rn = list(Rm)
    Rn[cin] = Rm[cin] + M(g) * M(a)
    if a == 0:
        return Rm[cout], Rn
    lo, hi = M(0), Rm[cout]
    for _ in range(2000):
        mid = (lo + hi) / 2
        Rn[cout] = mid
        if phi(Rn) < k0:
            lo = mid
        else:
            hi = mid
        if hi - lo <= hi * TEN ** -72:
            break
    Rn[cout] = (lo + hi) / 2
    return Rn[cout], Rn


def rate_truth(phi, R, g, cin, cout, a):
    """(out, rate) of one reserve-family row: the 80-digit root, then γ·φ_in/φ_out at the state it leaves"""
    yp, Rn = state_root(phi, R, g, cin, cout, a)

    def partial(j):   # ∂φ/∂R_j = (d/dt φ(.., R_j·e^t, ..) at t = 0)/R_j: a step relative to R_j, however small y′ is
        return mp.diff(lambda t: phi([Rn[k] * mp.exp(t) if k == j else Rn[k] for k in range(len(Rn))]), M(0)) / Rn[j]
    return M(float(R[cout])) - yp, M(g) * partial(cin) / partial(cout)


def one_sided(q, h):
    """the five-point forward difference of q at 0, error O(h⁴) (a lopsided Curve pool bends over a length far below R_i: the
    three-point formula gave 25 digits there)"""
    return (-25 * q(M(0)) + 48 * q(h) - 36 * q(2 * h) + 16 * q(3 * h) - 3 * q(4 * h)) / (12 * h)


def difference_check(phi, R, g, cin, cout, a, rate, what):
    q = lambda aa: -state_root(phi, R, g, cin, cout, aa)[0]   # noqa: E731  the quote less the constant R_o (aa: an mpf)
    if a != 0.0:
        h = M(a) * TEN ** -20
        fd = (q(M(a) + h) - q(M(a) - h)) / (2 * h)
    else:
        h = M(float(R[cin])) * TEN ** -20
        fd = one_sided(q, h)
    agree(fd, rate, 30, what)


# ---- closed forms in mpmath: cross-check + conditioning -------------------------------------------------------------
def cf_product(Ri, Ro, g, a):
    return g * Ri * Ro / (Ri + g * a) ** 2


def cf_weighted(Ri, Ro, wi, wo, g, a):
    xp = Ri + g * a
    return g * (wi / wo) * Ro * (Ri / xp) ** (wi / wo) / xp


def cf_solidly(Ri, Ro, g, a):
    xp = Ri + g * a
    c = (Ro / Ri) * (1 + (Ro / Ri) ** 2) * (Ri / xp) ** 4
    s = mp.cbrt(c / 2 + mp.sqrt(c * c / 4 + M(1) / 27))
    u = s - 1 / (3 * s)
    return g * u * (3 + u * u) / (1 + 3 * u * u)


def cf_curve(Ri, Ro, alpha, lP0, g, a):
    xp = Ri + g * a
    yp = Ro - Q.cf_curve(Ri, Ro, alpha, lP0, g, a)
    Pp = mp.e ** lP0 * Ri * Ro / (xp * yp)
    return g * (alpha + Pp / xp) / (alpha + Pp / yp)


def make_reserve_group(fx, out, name):
    g = P.group(fx, name)
    fam = P.family(name)
    n = g["a"].size
    rows = []
    for zero in (False, True):
        for r in range(n):
            R, gam, ci, co = g["R"][r], float(g["gamma"][r]), int(g["cin"][r]), int(g["cout"][r])
            a = 0.0 if zero else float(g["a"][r])
            Rm = [M(float(x)) for x in R]
            if fam == "product":
                phi = lambda RR: RR[0] * RR[1]   # noqa: E731
                xs, cf = [Rm[ci], Rm[co], M(gam), M(a)], cf_product
            elif fam == "solidly":
                phi = Q.phi_solidly
                xs, cf = [Rm[ci], Rm[co], M(gam), M(a)], cf_solidly
            elif fam in ("geomean", "weighted"):
                wm = [M(float(x)) for x in g["w"][r]]
                phi = lambda RR, wm=wm: Q.phi_weighted(RR, wm)   # noqa: E731
                xs, cf = [Rm[ci], Rm[co], wm[ci], wm[co], M(gam), M(a)], cf_weighted
            else:
                al, be = M(float(g["alpha"][r])), M(float(g["beta"][r]))
                phi = lambda RR, al=al, be=be: Q.phi_curve(RR, al, be)   # noqa: E731
                pr = M(1)
                for x in Rm:
                    pr *= x
                lP0 = mp.log(be / pr)
                xs, cf = [Rm[ci], Rm[co], al, lP0, M(gam), M(a)], cf_curve
            o, rate = rate_truth(phi, R, gam, ci, co, a)
            what = (name, r, "a=0" if zero else "a")
            agree(rate, cf(*xs), 30, what)
            difference_check(phi, R, gam, ci, co, a, rate, what)
            if fam == "curve":
                # the logs the device holds: log β and every log R_k enter through log P₀ (argument 3)
                logs = abs(mp.log(be)) + sum(abs(mp.log(x)) for x in Rm)
                cond = M(0)
                for j in (0, 1, 2, 4, 5):
                    if xs[j] != 0:
                        cond += abs(xs[j] * mp.diff(lambda t, j=j: cf(*[t if k == j else xs[k] for k in range(6)]), xs[j]))
                cond += logs * abs(mp.diff(lambda t: cf(xs[0], xs[1], xs[2], t, xs[4], xs[5]), lP0))
            else:
                cond = Q.cond_sum(cf, xs)
            if not zero:   # the quote fixture's own truth, to the double
                assert abs(float(o) - float(g["out"][r])) <= 2.0 ** -52 * float(g["out"][r]), (what, float(o), float(g["out"][r]))
            rows.append((r, a, float(o), float(rate), float(cond)))
    out[f"{name}_row"] = np.array([r[0] for r in rows], dtype=np.int64)     # the row of quote_precise.npz's group
    out[f"{name}_a"] = np.array([r[1] for r in rows])
    out[f"{name}_out"] = np.array([r[2] for r in rows])
    out[f"{name}_rate"] = np.array([r[3] for r in rows])
    out[f"{name}_cond"] = np.array([r[4] for r in rows])
    out[f"{name}_cls"] = np.array([CLASSES.index(c) for c in g["cls"]] * 2, dtype=np.int32)
    return len(rows)


# ---- UniV3 ----------------------------------------------------------------------------------------------------------
def mp_records(cp, lt, lq, cin):
    """the non-empty ticks of the direction in walk order, the current one first: (k, s_in, s_out, δmax, R_out)"""
    t, ct = Q.mp_ticks(cp, lt, lq)
    nt = len(lt)
    recs = []
    for idx in (range(ct, nt + 1) if cin == 0 else range(ct, 0, -1)):
        k, al, be, R1, R2 = t[idx]
        if cin == 1:
            al, be, R1, R2 = be, al, R2, R1
        if k == 0:
            continue
        recs.append((k, R1 + al, R2 + be, k / be - (R1 + al) if be > 0 else mp.inf, R2))
    return recs


def mp_out(recs, dp):
    """the walk's amount out for δ′ = dp (an mpf: the difference check needs more than a double's digits of it)"""
    lam, d = M(0), dp
    for k, s_in, s_out, dmax, rout in recs:
        if dmax > d:
            return lam + min(rout, s_out - k / (s_in + d))
        lam += rout
        d -= dmax
    return lam


def tick_rate(rec, g, a, S, drained, d):
    """(rate, cond) inside one tick entered with d of δ′ = γa: rate = γk/s², s = s_in + γa − S with S = Σ_j (k_j/β_j − s_in,j)
    over the drained ticks; cond = Σ |x ∂rate/∂x| over k, γ, a, s_in and the drained ticks' k_j/β_j and s_in,j"""
    k, s_in = rec[0], rec[1]
    s = s_in + d
    rate = M(g) * k / s ** 2
    ga = M(g) * M(a)
    return rate, rate * (1 + abs(1 - 2 * ga / s) + 2 * (ga + s_in + drained) / s)


def mp_rate(cp, lt, lq, g, cin, a):
    """-> (rate, cond, rate_left, cond_left, at_boundary) by the reference's walk (src/cfmms.jl:416-434) in mpmath"""
    recs = mp_records(cp, lt, lq, cin)
    dp = M(g) * M(a)
    S, drained = M(0), M(0)
    sums = [M(0)]
    for rec in recs:
        sums.append(sums[-1] + rec[3])
    # the boundary the exact δ′ is nearest to (Σδmax_e, e >= 1), and whether it is within 2^-40 relative of it
    flagged = None
    for e in range(1, len(sums)):
        if sums[e] != mp.inf and abs(dp - sums[e]) <= sums[e] * M(2) ** -40:
            flagged = e
    if flagged is not None:
        e = flagged
        drained_l = sum((r[3] + 2 * r[1] for r in recs[:e - 1]), M(0))      # k/β + s_in = δmax + 2 s_in
        left = tick_rate(recs[e - 1], g, a, sums[e - 1], drained_l, min(dp, sums[e]) - sums[e - 1])
        if e < len(recs):
            drained_r = drained_l + recs[e - 1][3] + 2 * recs[e - 1][1]
            right = tick_rate(recs[e], g, a, sums[e], drained_r, max(dp - sums[e], M(0)))
        else:
            right = (M(0), M(0))
        return right[0], right[1], left[0], left[1], True
    d = dp
    for rec in recs:
        if rec[3] > d:
            rate, cond = tick_rate(rec, g, a, S, drained, d)
            return rate, cond, rate, cond, False
        S += rec[3]
        drained += rec[3] + 2 * rec[1]
        d -= rec[3]
    return M(0), M(0), M(0), M(0), False      # "We've exhausted all liquidity"


def make_univ3(fx, out):
    g = P.group(fx, "univ3")
    npools = g["current_price"].size
    queries = [(str(c), int(p), int(ci), float(a)) for c, p, ci, a in zip(g["cls"], g["pool"], g["cin"], g["a"])]
    queries += [("spot", p, ci, 0.0) for p in range(npools) for ci in (0, 1)]
    rows = []
    for cls, p, ci, a in queries:
        cp, lt, lq, gam = P.univ3_pool(g, p)
        rate, cond, rl, cl, flag = mp_rate(cp, lt, lq, gam, ci, a)
        recs = mp_records(cp, lt, lq, ci)
        q = lambda aa: mp_out(recs, M(gam) * aa)   # noqa: E731
        if not flag:
            if a != 0.0:
                h = M(a) * TEN ** -20
                fd = (q(M(a) + h) - q(M(a) - h)) / (2 * h)
            else:
                h = (recs[0][1] if recs else M(1)) * TEN ** -20
                fd = one_sided(q, h)
            if rate == 0:
                assert fd == 0, (cls, p, ci, a, fd)
            else:
                agree(fd, rate, 30, ("univ3", cls, p, ci, a))
        assert a == 0.0 or q(M(a)) == Q.mp_walk(cp, lt, lq, gam, ci, a)[0], (cls, p, ci, a)
        rows.append((cls, p, ci, a, float(q(M(a))) if a != 0.0 else 0.0, float(rate), float(cond), float(rl), float(cl), flag))
    flagged = [r[0] for r in rows if r[9]]
    assert len(flagged) == 10 and set(flagged) == {"boundary_dn", "boundary_up"}, flagged
    assert all(r[9] for r in rows if r[0] in ("boundary_dn", "boundary_up"))
    assert all(np.isfinite(r[5]) and r[5] > 0 for r in rows if r[0] == "spot"), "a spot row without liquidity in its direction"
    out["univ3_pool"] = np.array([r[1] for r in rows], dtype=np.int64)
    out["univ3_cin"] = np.array([r[2] for r in rows], dtype=np.int32)
    out["univ3_a"] = np.array([r[3] for r in rows])
    out["univ3_out"] = np.array([r[4] for r in rows])
    out["univ3_rate"] = np.array([r[5] for r in rows])
    out["univ3_cond"] = np.array([r[6] for r in rows])
    out["univ3_rate_left"] = np.array([r[7] for r in rows])
    out["univ3_cond_left"] = np.array([r[8] for r in rows])
    out["univ3_at_boundary"] = np.array([r[9] for r in rows], dtype=np.bool_)
    out["univ3_cls"] = np.array([CLASSES.index(r[0]) for r in rows], dtype=np.int32)
    return len(rows)


def save(path, arrays):
    """np.savez_compressed with every member's time stamp fixed: the same arrays give the same bytes"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def main():
    fx = P.load()
    out = {"classes": np.array(CLASSES)}
    sizes = {}
    for name in P.GROUPS:
        sizes[name] = make_univ3(fx, out) if name == "univ3" else make_reserve_group(fx, out, name)
    save(OUT, out)
    print(OUT, os.path.getsize(OUT), "bytes;", sizes)


if __name__ == "__main__":
    main()
