"""ProductTwoCoin and UniV3 / BoundedProduct trades on the device against the 60-digit truth of tests/golden/cp_precise.npz.

Every path that reaches these pools is run on every case of the fixture: host-pointer sweeps with fast_math = 1 and 0,
device-pointer sweeps (cfmm_sweep_dev: the Auto kernels, and dev_prices_in_window = 1: the fast kernels alone; not on
p_pxout, whose price breaks the promise that option makes), non-materialising evaluations (Ψ and acc only), pack = 0,
compact_trades = 0, univ3_heads = 0 (UniV3), UniV3 pools uploaded at another current price -- up to three ticks away --
and moved to the fixture's with cfmm_pools_set_prices, both families in one context (the fused launch), and a <= 512-pool
subset (`direct`: one block whose row is the result, no fold).  A one-family context of up to 2048 pools would take that
single-block launch on EVERY path, so all the other paths upload the case as many times over as it takes to exceed 2048
pools (every copy is held to the truth) and the launch geometry is asserted: more than one block there, one block on
`direct`.  The truth knows nothing of walk lists, prefix sums, thresholds, heads or bands.

Bounds (derivation in tests/cp_precise_ref.py): with u = 2⁻⁵³,
    product   |Δ − Δ*| <= K·u·(X* + R_in)/γ,   |Λ − Λ*| <= K·u·(Y* + R_out)
    univ3     |Δ − Δ*| <= K·u·S_in/γ,          |Λ − Λ*| <= K·u·S_out
K per class (cp_precise_ref.K_PRODUCT / K_UNIV3): the next power of two >= 2x the largest ratio observed on the CPU oracle
and on an MI355X over every path (printed with -s: profiles/cp_precise_gpu_tests.log), at most 16 on well / inside /
walk_head / walk_deep and 64 elsewhere.  Trades whose truth is zero with the no-trade condition clear by more than 2^-40
must be exactly zero.  Ψ and acc are checked twice (helpers.reduction_checks): against math.fsum of the device's own
trades and against the truth.  Every materialised row is also bit-equal to the CPU oracle on the same inputs.
"""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import cp_precise_ref as P
from helpers import dev_sweep, oracle_sweep, reduction_checks

pytestmark = pytest.mark.gpu

PC, UC, PCLS, UCLS = P.load()
CASES = [(name, c, PCLS, P.K_PRODUCT) for name, c in sorted(PC.items())] + \
        [(name, c, UCLS, P.K_UNIV3) for name, c in sorted(UC.items())]
OPTS = {"host_full": {"fast_math": 0}, "dev_window": {"dev_prices_in_window": 1}, "pack0": {"pack": 0},
        "compact0": {"compact_trades": 0}, "heads0": {"univ3_heads": 0}}


def _k(table, names, cls):
    return np.array([table[names[c]] for c in cls], dtype=np.float64)


def _is_univ3(c):
    return "cp" in c


def _batch(c, idx=None, cp=None):
    """the case's pools (idx: a subset, in that order) as one batch; cp: another current price per pool"""
    m = len(c["gamma"])
    idx = np.arange(m) if idx is None else np.asarray(idx)
    if not _is_univ3(c):
        return cr.ProductTwoCoin.batch(c["R"][idx], c["gamma"][idx], c["Ai"][idx])
    off = c["tick_off"]
    sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx])
    noff = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(off[idx + 1] - off[idx], out=noff[1:])
    cp = c["cp"] if cp is None else cp
    return cr.UniV3.batch(cp[idx], noff, c["lower_ticks"][sel], c["liquidity"][sel], c["gamma"][idx], c["Ai"][idx])


def _scales(c):
    return P.univ3_scale(c) if _is_univ3(c) else P.product_scale(c["R"], c["gamma"], c["D"], c["L"])


def _elsewhere(c):
    """a current price up to three ticks away from the fixture's, inside the ladder (the middle of that tick)"""
    off, lt = c["tick_off"], c["lower_ticks"]
    cp0 = np.empty_like(c["cp"])
    for i in range(len(cp0)):
        t = lt[off[i]:off[i + 1]]
        j = min(max(np.count_nonzero(t >= c["cp"][i]) - 1 + (i % 7 - 3), 0), len(t) - 1)
        cp0[i] = 0.5 * (t[j] + (t[j + 1] if j + 1 < len(t) else 0.0))
    return cp0


def _sweep(be, c, path):
    """-> (Δ flat or None, Λ, Ψ, acc)"""
    if path == "eval":
        return (None, None) + tuple(be.eval(c["v"]))
    psi, acc = dev_sweep(be, c["v"]) if path in ("dev_auto", "dev_window") else be.find_arb(c["v"])
    D, L = be.trades()
    return np.reshape(D, (-1, 2)), np.reshape(L, (-1, 2)), psi, acc


DIRECT_POOLS = 2048    # a one-family context of up to this many pools is swept by a single block (launch_plan.cpp)


def _copies(m):
    """how many copies of an m-pool case make a segment that no longer fits the single-block launch"""
    return -(-(DIRECT_POOLS + 1) // m)


def _run(c, path, idx):
    """the pools idx of the case through one path -> (Δ or None, Λ, Ψ, acc, the segment's launch geometry)"""
    moved = path == "moved"
    be = cr.DeviceBackend(len(c["v"]), [_batch(c, idx, _elsewhere(c) if moved else None)])
    try:
        for k, val in OPTS.get(path, {}).items():
            be.ctx.set_option(k, val)
        if moved:
            be.find_arb(c["v"])                                   # the lists of the first upload have been swept once
            be.ctx.set_prices(0, np.arange(len(idx)), c["cp"][idx])
        out = _sweep(be, c, path)
        return out + (be.ctx.segments()[0],)
    finally:
        be.close()


def _paths(name, c):
    paths = ["host_fast", "host_full", "dev_auto", "eval", "direct", "pack0", "compact0"]
    if name != "p_pxout":                   # a price outside the window breaks the promise dev_prices_in_window makes
        paths.append("dev_window")
    if _is_univ3(c):
        paths += ["heads0", "moved"]
    return paths


RATIOS = {}    # (case, path) -> (per-pool normalised error, classes, names)
ORACLE = {}    # case -> the CPU oracle's (Δ, Λ) on the fixture's inputs


def _oracle(name, c):
    if name not in ORACLE:
        with np.errstate(all="ignore"):
            D, L, _, _ = oracle_sweep([_batch(c)], len(c["v"]), c["v"])
        ORACLE[name] = (np.reshape(D, (-1, 2)), np.reshape(L, (-1, 2)))
    return ORACLE[name]


@pytest.fixture(scope="module")
def report():
    yield RATIOS
    lines = ["", "observed max ratio |err| / (u·scale) per case, path and class:"]
    worst = {}
    for (name, path), (r, cls, names) in sorted(RATIOS.items()):
        if r is None:
            lines.append(f"  {name:9s} {path:10s} (no trades materialised: Ψ and acc within the bounds)")
            continue
        cm = P.class_max(r, cls, names)
        for k, x in cm.items():
            fam = "univ3" if names is UCLS else "product"
            worst[(fam, k)] = max(worst.get((fam, k), 0.0), x)
        lines.append(f"  {name:9s} {path:10s} " + "  ".join(f"{k}={x:.3g}" for k, x in cm.items()))
    lines.append("largest ratio per family and class over every path, and the K the rule gives:")
    for (fam, k), x in sorted(worst.items()):
        lines.append(f"  {fam:8s} {k:12s} {x:.4g}  K = {P.k_from(x)}")
    print("\n".join(lines))


def _check_rows(name, path, c, names, table, rows, D, L, bD, bL):
    r = P.ratios(D, L, c["D"][rows], c["L"][rows], bD[rows], bL[rows])
    cls = c["cls"][rows]
    RATIOS[(name, path)] = (r, cls, names)
    kk = _k(table, names, cls)
    assert np.all(r <= kk), (name, path, np.flatnonzero(r > kk)[:8], r[r > kk][:8], cls[r > kk][:8])
    assert P.zero_rows_exact(D, L, c["zclear"][rows]), (name, path)
    Do, Lo = _oracle(name, c)
    np.testing.assert_array_equal(D, Do[rows], err_msg=f"{name} {path}")
    np.testing.assert_array_equal(L, Lo[rows], err_msg=f"{name} {path}")


def _tiled(c, reps):
    """the fields helpers.reduction_checks reads, for `reps` copies of the case one after the other"""
    return dict(v=c["v"], Ai=np.tile(c["Ai"], (reps, 1)), D=np.tile(c["D"], (reps, 1)), L=np.tile(c["L"], (reps, 1)))


@pytest.mark.parametrize("name,c,names,table", CASES, ids=[x[0] for x in CASES])
def test_trades_psi_and_acc_against_the_truth(name, c, names, table, report):
    bD, bL = _scales(c)
    m = len(c["gamma"])
    reps = _copies(m)
    for path in _paths(name, c):
        if path == "direct":           # every ceil(m/512)-th pool, so that every class is in it
            rows = slice(0, m, -(-m // 512))
            D, L, psi, acc, seg = _run(c, path, np.arange(m)[rows])
            assert seg["grid"] == 1 and seg["block"] == 1024, (name, path, seg)
            _check_rows(name, path, c, names, table, rows, D, L, bD, bL)
            reduction_checks(c, rows, D, L, psi, acc, _k(table, names, c["cls"][rows]), bD[rows], bL[rows])
            continue
        D, L, psi, acc, seg = _run(c, path, np.tile(np.arange(m), reps))
        assert seg["m"] == reps * m > DIRECT_POOLS and seg["grid"] > 1, (name, path, seg)   # partial rows and the fold
        if D is not None:
            D, L = D.reshape(reps, m, 2), L.reshape(reps, m, 2)
            _check_rows(name, path, c, names, table, slice(None), D[0], L[0], bD, bL)
            for r in range(1, reps):                              # every copy: the same bits wherever its block sits
                np.testing.assert_array_equal(D[r], D[0], err_msg=f"{name} {path} copy {r}")
                np.testing.assert_array_equal(L[r], L[0], err_msg=f"{name} {path} copy {r}")
            D, L = D.reshape(-1, 2), L.reshape(-1, 2)
        reduction_checks(_tiled(c, reps), slice(None), D, L, psi, acc, np.tile(_k(table, names, c["cls"]), reps),
                         np.tile(bD, (reps, 1)), np.tile(bL, (reps, 1)), check_self=D is not None)
        RATIOS.setdefault((name, path), (None, None, names))


@pytest.mark.parametrize("vcase", ["p_main", "u_main"])
def test_both_families_in_one_context(vcase, report):
    """The fused launch: p_main and u_main as two segments of one context, swept at either case's prices.  Both segments
    are bit-equal to the oracle; the segment whose prices they are is held to its truth; Ψ and acc of the fused
    reduction are held to the device's own trades and to the truth (for the other segment, whose trades ARE the
    oracle's, the oracle's trades stand in with no allowance)."""
    p, u = PC["p_main"], UC["u_main"]
    v = (p if vcase == "p_main" else u)["v"]
    batches = [_batch(p), _batch(u)]
    mp_ = len(p["gamma"])
    be = cr.DeviceBackend(len(v), batches)
    try:
        psi, acc = be.find_arb(v)
        D, L = (np.reshape(x, (-1, 2)) for x in be.trades())
        segs = be.ctx.segments()
        psi_e, acc_e = be.eval(v)
    finally:
        be.close()
    assert len(segs) == 2 and all(sg["grid"] > 1 for sg in segs), segs
    with np.errstate(all="ignore"):
        Do, Lo, _, _ = oracle_sweep(batches, len(v), v)
    Do, Lo = np.reshape(Do, (-1, 2)), np.reshape(Lo, (-1, 2))
    np.testing.assert_array_equal(D, Do)
    np.testing.assert_array_equal(L, Lo)
    c, names, table, rows = (p, PCLS, P.K_PRODUCT, slice(0, mp_)) if vcase == "p_main" else (u, UCLS, P.K_UNIV3, slice(mp_, None))
    bD, bL = _scales(c)
    _check_rows(vcase, "mixed", c, names, table, slice(None), D[rows], L[rows], bD, bL)
    both = dict(v=v, Ai=np.concatenate([p["Ai"], u["Ai"]]), D=Do.copy(), L=Lo.copy())
    both["D"][rows], both["L"][rows] = c["D"], c["L"]
    kk, sD, sL = np.zeros(len(D)), np.zeros_like(D), np.zeros_like(L)
    kk[rows], sD[rows], sL[rows] = _k(table, names, c["cls"]), bD, bL
    reduction_checks(both, slice(None), D, L, psi, acc, kk, sD, sL)
    reduction_checks(both, slice(None), None, None, psi_e, acc_e, kk, sD, sL, check_self=False)   # the fused, non-materialising launch


# ---- after update_reserves ----------------------------------------------------------------------------------------

def test_update_reserves_product_matches_a_fresh_upload():
    c = PC["p_main"]
    m, n = len(c["gamma"]), len(c["v"])
    kk = _k(P.K_PRODUCT, PCLS, c["cls"])[:, None]
    bD, bL = _scales(c)
    be = cr.DeviceBackend(n, [_batch(c)])
    try:
        be.find_arb(c["v"])
        be.ctx.update_reserves()
        Rr = be.ctx.reserves(0, m, 2)
        g = c["gamma"][:, None]
        Rt = c["R"] + g * c["D"] - c["L"]
        tol = kk * (g * bD + bL) + 2 * P.U * (c["R"] + g * c["D"] + c["L"])
        assert np.all(np.abs(Rr - Rt) <= tol), np.max(np.abs(Rr - Rt) / tol)
        be.find_arb(c["v2"])
        DA, LA = (np.reshape(x, (m, 2)) for x in be.trades())
    finally:
        be.close()
    fresh = cr.ProductTwoCoin.batch(Rr, c["gamma"], c["Ai"])
    be = cr.DeviceBackend(n, [fresh])
    try:
        be.find_arb(c["v2"])
        DB, LB = (np.reshape(x, (m, 2)) for x in be.trades())
    finally:
        be.close()
    np.testing.assert_array_equal(DA, DB)
    np.testing.assert_array_equal(LA, LB)
    Do, Lo, _, _ = oracle_sweep([fresh], n, c["v2"])
    np.testing.assert_array_equal(DA, np.reshape(Do, (m, 2)))
    np.testing.assert_array_equal(LA, np.reshape(Lo, (m, 2)))
    assert np.count_nonzero(DA) > m // 4


def test_update_reserves_univ3_matches_a_fresh_upload():
    """update_reserves moves a trading pool to its target price P (at most the first tick's upper price) and prepares it
    again: the next sweep equals that of a fresh upload at the read-back prices, and the CPU oracle's."""
    c = UC["u_main"]
    m, n = len(c["gamma"]), len(c["v"])
    be = cr.DeviceBackend(n, [_batch(c)])
    try:
        be.find_arb(c["v"])
        be.ctx.update_reserves()
        q = be.ctx.prices(0, m)
        vp, g, cp = c["v"][c["Ai"] - 1], c["gamma"], c["cp"]
        pr = vp[:, 0] / vp[:, 1]
        top = c["lower_ticks"][c["tick_off"][:-1]]
        want = np.where((g * cp <= pr) & (pr <= cp / g), cp, np.minimum(np.where(pr < g * cp, pr / g, g * pr), top))
        np.testing.assert_array_equal(q, want)
        traded = np.any(c["D"] > 0, axis=1)
        assert np.count_nonzero(q[traded] != cp[traded]) >= 0.9 * np.count_nonzero(traded)
        be.find_arb(c["v2"])
        DA, LA = (np.reshape(x, (m, 2)) for x in be.trades())
    finally:
        be.close()
    fresh = _batch(c, cp=q)
    be = cr.DeviceBackend(n, [fresh])
    try:
        be.find_arb(c["v2"])
        DB, LB = (np.reshape(x, (m, 2)) for x in be.trades())
    finally:
        be.close()
    np.testing.assert_array_equal(DA, DB)
    np.testing.assert_array_equal(LA, LB)
    with np.errstate(all="ignore"):
        Do, Lo, _, _ = oracle_sweep([fresh], n, c["v2"])
    np.testing.assert_array_equal(DA, np.reshape(Do, (m, 2)))
    np.testing.assert_array_equal(LA, np.reshape(Lo, (m, 2)))
    assert np.count_nonzero(DA) > m // 4
