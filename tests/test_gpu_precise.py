"""GeometricMeanTwoCoin and N-coin weighted trades on the device against the 60-digit truth of tests/golden/precise.npz.

Every path that reaches these pools is run on every case of the fixture: host-pointer sweeps with fast_math = 1 (the
own exp and the refined reciprocals) and 0 (the library's exp and /), device-pointer sweeps (cfmm_sweep_dev: the Auto
kernels, and dev_prices_in_window = 1: the fast kernels alone), geomean_exact = 1 (pow in the reference's order), a
<= 512-pool slice (the single-block direct path) and non-materialising evaluations (Ψ and acc only).

Bounds (derivation in tests/precise_ref.py): with u = 2⁻⁵³ and the scale computed from the inputs and the truth,
    two-coin   |Δ − Δ*| <= K·u·(κ·X* + r_b)/γ,   |Λ − Λ*| <= K·u·(κ·Y* + r_a),
               κ = 1 + (|ln γ| + |ln η| + |ln v₁| + |ln v₂| + |ln r_a| + e·|ln r_b|)/(e + 1)
    weighted   |Δ_k − Δ*_k| <= K·u·κ·(R_k + γΔ*_k)/γ,   |Λ_k − Λ*_k| <= K·u·κ·R_k,   κ = 1 + |ln γ| + max_k |s_k|.
K is per class (the reference-order path has its own): the next power of two >= 2× the largest ratio observed on an
MI355X over every path (printed with -s), at most 16 on the well-conditioned classes and 64 elsewhere.  Ψ and acc are checked twice: against math.fsum of the device's own
trades (isolates the LDS scatter and the folds: (c + 2)·u·Σ|terms| for c nonzero terms), and against the truth (the sum
of the per-pool bounds plus that reduction bound).
"""
import ctypes

import numpy as np
import pytest

import cfmmrouter_amd as cr
import precise_ref as P
import weighted_ref as wr
from cfmmrouter_amd._lib import KIND_WEIGHTED
from helpers import reduction_checks as _reduction_checks

pytestmark = pytest.mark.gpu

U = P.U
GC, WC, GCLS, WCLS = P.load()

# K per class (the next power of two >= 2x the largest ratio observed over every path, at most 16 on the well-conditioned
# classes and 64 elsewhere); the reference-order path has its own.  Observed maxima: profiles/precise_gpu_tests.log.
K_TWO = {"well": 4, "both_live": 4, "band_edge": 4, "eq_gamma1": 4, "wide": 8, "overflow": 4, "res_out": 8, "px_out": 8}
K_TWO_EXACT = {"well": 4, "both_live": 4, "band_edge": 4, "eq_gamma1": 4, "wide": 4, "overflow": 4, "res_out": 4, "px_out": 4}
K_W = {"well": 4, "wide": 8, "gamma1": 8, "ties": 16, "on_bp": 16, "near_bp": 16, "band": 1}
K_UPDATE = {"two": 4, "weighted": 2}   # refreshed store against a fresh upload of the read-back reserves


def _k(table, names, cls):
    return np.array([table[names[c]] for c in cls], dtype=np.float64)


# ---- device-pointer sweeps: the HIP runtime the library already loaded ------------------------------------------

def _hip():
    import cfmmrouter_amd._lib as lib
    lib.lib()
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                path = line.split()[-1]
                break
    assert path, "libamdhip64 is not loaded"
    h = ctypes.CDLL(path)
    h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipFree.argtypes = [ctypes.c_void_p]
    return h


def _dev_sweep(be, v, materialize=True):
    h = _hip()
    n = len(v)
    dv, dout = ctypes.c_void_p(), ctypes.c_void_p()
    assert h.hipMalloc(ctypes.byref(dv), 8 * n) == 0 and h.hipMalloc(ctypes.byref(dout), 8 * (n + 1)) == 0
    try:
        vh = np.ascontiguousarray(v, dtype=np.float64)
        out = np.empty(n + 1)
        assert h.hipMemcpy(dv, vh.ctypes.data, 8 * n, 1) == 0
        be.ctx.sweep_dev(dv.value, dout.value, materialize)
        assert h.hipDeviceSynchronize() == 0
        assert h.hipMemcpy(out.ctypes.data, dout, 8 * (n + 1), 2) == 0
        return out[:n], float(out[n])
    finally:
        h.hipFree(dv)
        h.hipFree(dout)


def _batch(c, R=None, rows=slice(None)):
    R = c["R"][rows] if R is None else R
    if c["R"].shape[1] == 2 and "weighted" not in c:
        return cr.GeometricMeanTwoCoin.batch(R, c["w"][rows], c["gamma"][rows], c["Ai"][rows])
    return cr.PoolBatch(KIND_WEIGHTED, R=R, w=c["w"][rows], γ=c["gamma"][rows], Ai=c["Ai"][rows])


def _run(c, path, rows=slice(None)):
    """-> (Δ [m, N] or None, Λ, Ψ, acc) for one path."""
    N = c["R"].shape[1]
    b = _batch(c, rows=rows)
    m = len(b)
    be = cr.DeviceBackend(len(c["v"]), [b])
    try:
        opts = {"host_full": {"fast_math": 0}, "dev_window": {"dev_prices_in_window": 1},
                "exact": {"geomean_exact": 1}}.get(path, {})
        for k, val in opts.items():
            be.ctx.set_option(k, val)
        if path == "eval":
            psi, acc = be.eval(c["v"])
            return None, None, psi, acc
        if path in ("dev_auto", "dev_window"):
            psi, acc = _dev_sweep(be, c["v"])
        else:
            psi, acc = be.find_arb(c["v"])
        D, L = be.trades()
        return np.reshape(D, (m, N)), np.reshape(L, (m, N)), psi, acc
    finally:
        be.close()


def _scales(c, rows=slice(None)):
    R, w, g, Ai = c["R"][rows], c["w"][rows], c["gamma"][rows], c["Ai"][rows]
    Dt, Lt = c["D"][rows], c["L"][rows]
    vl = c["v"][Ai - 1]
    if "weighted" in c:
        return P.weighted_scale(R, w, g, vl, Dt, Lt)
    return P.two_coin_scale(R, w, g, vl, Dt, Lt)


# ---- one pass over every case and path, shared by the tests below -----------------------------------------------

RATIOS = {}    # (case, path) -> per-pool normalised error (the K each pool needs), or None for eval


def _paths(name, c):
    paths = ["host_fast", "host_full", "dev_auto", "eval"]
    if name != "g_pxout":                  # a price outside the window breaks the promise dev_prices_in_window makes
        paths.append("dev_window")
    if "weighted" not in c:
        paths += ["exact", "direct"]
    return paths


def _cases():
    out = []
    for name, c in sorted(GC.items()):
        out.append((name, c, GCLS))
    for name, c in sorted(WC.items()):
        c = dict(c, weighted=True)
        out.append((name, c, WCLS))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def report():
    yield RATIOS
    lines = ["", "observed max ratio |err| / (u·scale) per case, path and class:"]
    for (name, path), (r, cls, names) in sorted(RATIOS.items()):
        lines.append(f"  {name:9s} {path:10s} " + "  ".join(f"{k}={v:.3g}" for k, v in P.class_max(r, cls, names).items()))
    print("\n".join(lines))


@pytest.mark.parametrize("name,c,names", CASES, ids=[x[0] for x in CASES])
def test_trades_psi_and_acc_against_the_truth(name, c, names, report):
    weighted = "weighted" in c
    Ktab = K_W if weighted else K_TWO
    vp = c["v"][c["Ai"] - 1]
    pred = np.zeros(len(c["gamma"]), dtype=bool) if weighted else P.pow_out_of_range(c["R"], c["w"], c["gamma"], vp)
    bD, bL = _scales(c)
    m = len(c["gamma"])
    for path in _paths(name, c):
        # the reference-order path on the pools whose powers stay inside float64; on the others its powers overflow
        # and the library refuses the evaluation (non-finite Ψ) instead of returning numbers
        rows = slice(0, min(m, 512)) if path == "direct" else (~pred if path == "exact" else slice(None))
        if path == "exact" and np.any(pred):
            with pytest.raises(RuntimeError, match="overflow"):
                _run(c, path, pred)
        D, L, psi, acc = _run(c, path, rows)
        cls = c["cls"][rows]
        kk = _k(K_TWO_EXACT if path == "exact" else Ktab, names, cls)
        sD, sL = bD[rows], bL[rows]
        if D is not None:
            r = P.ratios(D, L, c["D"][rows], c["L"][rows], sD, sL)
            RATIOS[(name, path)] = (r, cls, names)
            ok = r <= kk
            assert np.all(ok), (name, path, np.flatnonzero(~ok)[:8], r[~ok][:8], cls[~ok][:8])
        _reduction_checks(c, rows, D, L, psi, acc, kk, sD, sL, check_self=D is not None)
    if not weighted:
        # no regression from the log-space default: on every class its worst error is within 2× the reference order's
        rf, re = RATIOS[(name, "host_fast")][0][~pred], RATIOS[(name, "exact")][0]
        for k in np.unique(c["cls"][~pred]):
            sel = c["cls"][~pred] == k
            assert np.max(rf[sel]) <= 2.0 * max(np.max(re[sel]), 1.0), (name, names[k])


# ---- after update_reserves: the device's refresh of {Q1, Q2} / q against a fresh upload ---------------------------

def _approx_two_coin(R, w, g, vp):
    """The closed forms in float64 log space: a scale for the bound when no 60-digit truth exists (read-back reserves)."""
    eta = w[:, 0] / w[:, 1]
    D, L = np.zeros_like(R), np.zeros_like(R)
    for e, ra, rb, lm, dcol, lcol in ((eta, R[:, 1], R[:, 0], np.log(vp[:, 1] / vp[:, 0]), 0, 1),
                                      (1 / eta, R[:, 0], R[:, 1], np.log(vp[:, 0] / vp[:, 1]), 1, 0)):
        X = np.exp((np.log(g) + lm + np.log(e) + np.log(ra) + e * np.log(rb)) / (e + 1))
        Y = np.exp((np.log(rb) + np.log(ra) / e - np.log(e) - np.log(g) - lm) * (e / (1 + e)))
        D[:, dcol] = np.maximum(X - rb, 0) / g
        L[:, lcol] = np.maximum(ra - Y, 0)
    return D, L


@pytest.mark.parametrize("name", ["g_well", "w_3"])
def test_update_reserves_refresh_matches_a_fresh_upload(name):
    weighted = name.startswith("w_")
    c = dict(WC[name], weighted=True) if weighted else GC[name]
    names = WCLS if weighted else GCLS
    m, N = c["R"].shape
    kk = _k(K_W if weighted else K_TWO, names, c["cls"])     # the sweep at v: the trades' own K
    bD, bL = _scales(c)
    be = cr.DeviceBackend(len(c["v"]), [_batch(c)])
    try:
        be.find_arb(c["v"])
        be.ctx.update_reserves()
        Rr = be.ctx.reserves(0, m, N)
        g = c["gamma"][:, None]
        Rt = c["R"] + g * c["D"] - c["L"]
        tol = kk[:, None] * (g * bD + bL) + 2 * U * (c["R"] + g * c["D"] + c["L"])
        assert np.all(np.abs(Rr - Rt) <= tol), np.max(np.abs(Rr - Rt) / tol)
        be.find_arb(c["v2"])
        DA, LA = (np.reshape(x, (m, N)) for x in be.trades())
    finally:
        be.close()
    fresh = cr.DeviceBackend(len(c["v"]), [_batch(c, R=Rr)])
    try:
        fresh.find_arb(c["v2"])
        DB, LB = (np.reshape(x, (m, N)) for x in fresh.trades())
    finally:
        fresh.close()
    vl = c["v2"][c["Ai"] - 1]
    if weighted:
        Dp, Lp = wr.solve(Rr, c["w"], c["gamma"], vl)
        sD, sL = P.weighted_scale(Rr, c["w"], c["gamma"], vl, Dp, Lp)
    else:
        Dp, Lp = _approx_two_coin(Rr, c["w"], c["gamma"], vl)
        sD, sL = P.two_coin_scale(Rr, c["w"], c["gamma"], vl, Dp, Lp)
    r = P.ratios(DA, LA, DB, LB, sD, sL)
    print(f"\n[update] {name}: refreshed vs fresh upload, max ratio by class {P.class_max(r, c['cls'], names)}")
    K = K_UPDATE["weighted" if weighted else "two"]
    assert np.all(r <= K), (np.flatnonzero(r > K)[:8], r[r > K][:8])
    assert np.count_nonzero(DA) > m // 4
