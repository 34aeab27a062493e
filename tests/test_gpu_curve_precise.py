"""Curve (StableSwap) trades on the device against the 60-digit truth of tests/golden/curve_precise.npz.

Every path that reaches Curve pools is run on every case of the fixture: a materialising host-pointer sweep (find_arb),
a non-materialising evaluation (Ψ and acc only), a device-pointer sweep (cfmm_sweep_dev), the second evaluation of one
backend (the alternating tile order) and a multi-device parent (device=[0, 0]).  The pools the upload refuses (α > 0 with
log(P₀/R_k) outside ±600, tests/curve_precise_ref.py) are swept without them, and their upload is checked to fail.

Bound (derivation in tests/curve_precise_ref.py), with u = 2⁻⁵³ and r* = R + γΔ* − Λ*:
    |Δ_k − Δ*_k| <= K·u·(κ·(r*_k + R_k)/γ + cΔ_k),   |Λ_k − Λ*_k| <= K·u·(κ·(r*_k + R_k) + cΛ_k),
    κ = 1 + |ln γ| + |ln β| + max_k |ρ_k| + |s*|, cΔ / cΛ the conditioning Σ_j |x_j·∂T/∂x_j| over the inputs.
K is per class: the next power of two >= 2× the largest ratio observed on an MI355X over every path (printed with -s),
at most 16 on the well-conditioned classes and 64 elsewhere.  Ψ and acc are checked against math.fsum of the device's own
trades and against the truth (helpers.reduction_checks).
"""
import ctypes

import numpy as np
import pytest

import cfmmrouter_amd as cr
import curve_precise_ref as P
from helpers import reduction_checks

pytestmark = pytest.mark.gpu

C, CLS = P.load()

# The host build's K (tests/test_curve_precise_cpu.py: the rule and its two exceptions there).
K_DEV = {"well": 8, "stiff": 2, "small_a": 4, "alpha0": 2, "drained": 32, "band_edge": 4, "on_bp": 2, "near_bp": 2,
         "ties": 8, "low_gamma": 32, "wide": 64, "range": 1, "far_start": 4, "band": 1}
K_UPDATE = 16   # refreshed log R against a fresh upload of the read-back reserves


def _k(cls):
    return np.array([K_DEV[CLS[c]] for c in cls], dtype=np.float64)


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


def _dev_sweep(be, v):
    h = _hip()
    n = len(v)
    dv, dout = ctypes.c_void_p(), ctypes.c_void_p()
    assert h.hipMalloc(ctypes.byref(dv), 8 * n) == 0 and h.hipMalloc(ctypes.byref(dout), 8 * (n + 1)) == 0
    try:
        vh = np.ascontiguousarray(v, dtype=np.float64)
        out = np.empty(n + 1)
        assert h.hipMemcpy(dv, vh.ctypes.data, 8 * n, 1) == 0
        be.ctx.sweep_dev(dv.value, dout.value, True)
        assert h.hipDeviceSynchronize() == 0
        assert h.hipMemcpy(out.ctypes.data, dout, 8 * (n + 1), 2) == 0
        return out[:n], float(out[n])
    finally:
        h.hipFree(dv)
        h.hipFree(dout)


def _batch(c, rows, R=None):
    return cr.Curve.batch(c["R"][rows] if R is None else R, c["gamma"][rows], c["Ai"][rows], c["alpha"][rows],
                          c["beta"][rows])


def _run(c, rows, path, v=None):
    """-> (Δ [m, N] or None, Λ, Ψ, acc) for one path."""
    v = c["v"] if v is None else v
    b = _batch(c, rows)
    m, N = len(b), c["R"].shape[1]
    be = cr.DeviceBackend(len(c["v"]), [b], device=[0, 0] if path == "multi" else 0)
    try:
        if path == "eval":
            psi, acc = be.eval(v)
            return None, None, psi, acc
        if path == "dev":
            psi, acc = _dev_sweep(be, v)
        elif path == "second":
            be.find_arb(v * 1.1)
            psi, acc = be.find_arb(v)
        else:
            psi, acc = be.find_arb(v)
        D, L = be.trades()
        return np.reshape(D, (m, N)), np.reshape(L, (m, N)), psi, acc
    finally:
        be.close()


RATIOS = {}


@pytest.fixture(scope="module")
def report():
    yield RATIOS
    lines = ["", "observed max ratio |err| / (u·scale) per case, path and class:"]
    for (name, path), (r, cls) in sorted(RATIOS.items()):
        lines.append(f"  {name:4s} {path:8s} " + "  ".join(f"{k}={v:.3g}" for k, v in P.class_max(r, cls, CLS).items()))
    print("\n".join(lines))


@pytest.mark.parametrize("name", sorted(C))
def test_trades_psi_and_acc_against_the_truth(name, report):
    c = C[name]
    ref = P.refused(c["R"], c["alpha"], c["beta"])
    rows = np.flatnonzero(~ref)
    if np.any(ref):
        ctx = cr.Context(len(c["v"]), 0)
        try:
            i = int(np.flatnonzero(ref)[0])
            with pytest.raises(cr.ArgumentError, match="log"):
                ctx.add_curve(c["R"][i:i + 1], c["gamma"][i:i + 1], c["Ai"][i:i + 1] - 1, c["alpha"][i:i + 1],
                              c["beta"][i:i + 1])
            assert ctx.pool_count == 0
        finally:
            ctx.close()
    bD, bL = P.scale(c, rows)
    cls = c["cls"][rows]
    kk = _k(cls)
    for path in ("host", "eval", "dev", "second", "multi"):
        D, L, psi, acc = _run(c, rows, path)
        if D is not None:
            r = P.ratios(D, L, c["D"][rows], c["L"][rows], bD, bL)
            RATIOS[(name, path)] = (r, cls)
            ok = r <= kk
            assert np.all(ok), (name, path, rows[~ok][:8], r[~ok][:8], [CLS[k] for k in cls[~ok][:8]])
            band = cls == CLS.index("band")
            assert np.all(D[band] == 0) and np.all(L[band] == 0) and not np.any(np.signbit(D[band]))
        reduction_checks(c, rows, D, L, psi, acc, kk, bD, bL, check_self=D is not None)


@pytest.mark.parametrize("name", ["c_2", "c_5", "c_8"])
def test_scaling_all_prices_by_a_power_of_two_is_bit_identical(name):
    c = C[name]
    rows = np.flatnonzero(~P.refused(c["R"], c["alpha"], c["beta"]))
    D0, L0, _, _ = _run(c, rows, "host")
    for j in (-37, 60):
        D, L, _, _ = _run(c, rows, "host", v=c["v"] * 2.0 ** j)
        np.testing.assert_array_equal(D, D0)
        np.testing.assert_array_equal(L, L0)


def test_update_reserves_refresh_matches_a_fresh_upload():
    """update_ncoin<CurveFamily> refreshes log R on the device: the sweep at v2 after it against a fresh upload of the
    read-back reserves."""
    c = C["c_3"]
    # (pools that drain a coin below the ulp of its reserve -- far_start -- read back a reserve of 0: R + γΔ − Λ rounds at
    #  the old reserve's ulp, and such a reserve is no pool to upload)
    Rt = c["R"] + c["gamma"][:, None] * c["D"] - c["L"]
    kept = np.all(Rt > 4 * P.U * (c["R"] + c["gamma"][:, None] * c["D"] + c["L"]), axis=1)
    rows = np.flatnonzero(~P.refused(c["R"], c["alpha"], c["beta"]) & kept)
    m, N = len(rows), 3
    bD, bL = P.scale(c, rows)
    kk = _k(c["cls"][rows])
    be = cr.DeviceBackend(len(c["v"]), [_batch(c, rows)])
    try:
        be.find_arb(c["v"])
        be.ctx.update_reserves()
        Rr = be.ctx.reserves(0, m, N)
        g = c["gamma"][rows][:, None]
        Rt = c["R"][rows] + g * c["D"][rows] - c["L"][rows]
        tol = kk[:, None] * (g * bD + bL) + 2 * P.U * (c["R"][rows] + g * c["D"][rows] + c["L"][rows])
        assert np.all(np.abs(Rr - Rt) <= tol), np.max(np.abs(Rr - Rt) / tol)
        be.find_arb(c["v2"])
        DA, LA = (np.reshape(x, (m, N)) for x in be.trades())
    finally:
        be.close()
    fresh = cr.DeviceBackend(len(c["v"]), [_batch(c, rows, R=Rr)])
    try:
        fresh.find_arb(c["v2"])
        DB, LB = (np.reshape(x, (m, N)) for x in fresh.trades())
    finally:
        fresh.close()
    # the scale of the pools before the update (the refreshed reserves are within a trade of them)
    r = P.ratios(DA, LA, DB, LB, bD + P.U * np.abs(DB), bL + P.U * np.abs(LB))
    print(f"\n[update] c_3: refreshed vs fresh upload, max ratio by class {P.class_max(r, c['cls'][rows], CLS)}")
    assert np.all(r <= K_UPDATE), (np.flatnonzero(r > K_UPDATE)[:8], r[r > K_UPDATE][:8])
    assert np.count_nonzero(DA) > m // 4
