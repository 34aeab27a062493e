"""Solidly-style stable pairs on the device against the 60-digit truth of tests/golden/solidly_precise.npz.

Every path that reaches the kernel is run on every pool of every class, none left out: a materialising host-pointer sweep
(find_arb), a device-pointer sweep (cfmm_sweep_dev), the second evaluation of one backend (the alternating tile order), a
non-materialising evaluation (Ψ and acc only), the fixture cut into slices of 2048 pools (each a single-block direct
launch) and a multi-device parent (device=[0, 0]).

Bound (derivation in tests/solidly_precise_ref.py), u = 2⁻⁵³, κ = 4, x′* / y′* the exact new reserves of the tendered
and the received coin:
    |Δ − Δ*| <= K·u·(κ·(x′* + r_a)/γ + cΔ),   |Λ − Λ*| <= K·u·(κ·(y′* + r_b) + cΛ).
K per class: the next power of two >= 2× the worst ratio the NUMPY reference shows on that class
(tests/test_solidly_precise_cpu.py: well 0.36, balanced 0.29, band_edge 0.32, band 0, gamma1 0.34, low_gamma 0.46,
wide 0.62, range 0.47, drain 0.62), capped at 16 on well / gamma1 / band and 64 elsewhere: K = 2 on wide and drain, 1 on
every other class.  `band` must be exact +0.0.  Ψ and acc are checked against math.fsum of the device's own trades and
against the truth (helpers.reduction_checks).  The observed device maxima (printed with -s) are kept in
profiles/solidly_gpu_tests.log.
"""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import solidly_precise_ref as P
from helpers import reduction_checks
from solidly_dev import dev_sweep
from test_solidly_precise_cpu import K as K_CLASS

pytestmark = pytest.mark.gpu

C, CLS = P.load()
M = len(C["gamma"])
DIRECT = 2048          # sweep.h kDirectPools


def _k(cls):
    return np.array([K_CLASS[CLS[c]] for c in cls], dtype=np.float64)


def _batch(rows):
    return cr.SolidlyStableTwoCoin.batch(C["R"][rows], C["gamma"][rows], C["Ai"][rows])


def _run(rows, path):
    """-> (Δ [m, 2] or None, Λ, Ψ, acc) for one path over the fixture's `rows`."""
    v = C["v"]
    b = _batch(rows)
    m = len(b)
    be = cr.DeviceBackend(len(v), [b], device=[0, 0] if path == "multi" else 0)
    try:
        if path == "eval":
            psi, acc = be.eval(v)
            return None, None, psi, acc
        if path == "dev":
            psi, acc = dev_sweep(be, v)
        elif path == "second":
            be.find_arb(v * 1.1)
            psi, acc = be.find_arb(v)
        else:
            psi, acc = be.find_arb(v)
        if path == "direct":
            assert be.ctx.segments()[0]["grid"] == 1
        D, L = be.trades()
        return np.reshape(D, (m, 2)), np.reshape(L, (m, 2)), psi, acc
    finally:
        be.close()


RATIOS = {}


@pytest.fixture(scope="module")
def report():
    yield RATIOS
    lines = ["", "observed max ratio |err| / (u·scale) per path and class:"]
    for path, (r, cls) in sorted(RATIOS.items()):
        lines.append(f"  {path:8s} " + "  ".join(f"{k}={v:.3g}" for k, v in P.class_max(r, cls, CLS).items()))
    print("\n".join(lines))


def _check(rows, path, report):
    bD, bL = P.scale(C, rows)
    cls = C["cls"][rows]
    kk = _k(cls)
    D, L, psi, acc = _run(rows, path)
    if D is not None:
        r = P.ratios(D, L, C["D"][rows], C["L"][rows], bD, bL)
        if path in report:
            r0, c0 = report[path]
            report[path] = (np.concatenate([r0, r]), np.concatenate([c0, cls]))
        else:
            report[path] = (r, cls)
        ok = r <= kk
        assert np.all(ok), (path, rows[~ok][:8], r[~ok][:8], [CLS[k] for k in cls[~ok][:8]])
        band = cls == CLS.index("band")
        assert not D[band].any() and not L[band].any() and not np.signbit(D[band]).any() and not np.signbit(L[band]).any()
        assert np.all(D >= 0) and np.all(L >= 0) and not np.signbit(D).any() and not np.signbit(L).any()
    case = {"v": C["v"], "Ai": C["Ai"], "D": C["D"], "L": C["L"]}
    reduction_checks(case, rows, D, L, psi, acc, kk, bD, bL, check_self=D is not None)


@pytest.mark.parametrize("path", ["host", "dev", "second", "eval", "multi"])
def test_trades_psi_and_acc_against_the_truth(path, report):
    _check(np.arange(M), path, report)


def test_direct_slices_against_the_truth(report):
    """every pool of the fixture through the single-block direct path, 2048 pools at a time"""
    for lo in range(0, M, DIRECT):
        _check(np.arange(lo, min(lo + DIRECT, M)), "direct", report)


def test_scaling_all_reserves_by_a_power_of_two_scales_the_trades_exactly():
    """the closed form is scale-free in R (ratios only): reserves × 2^j give trades × 2^j, bit for bit"""
    rows = np.flatnonzero(C["cls"] != CLS.index("range"))       # (range sits at the ends of the upload range already)
    b = _batch(rows)
    v = C["v"]
    out = []
    for j in (0, -40, 60):
        be = cr.DeviceBackend(len(v), [cr.SolidlyStableTwoCoin.batch(b.R * 2.0 ** j, b.γ, b.Ai)])
        try:
            be.find_arb(v)
            D, L = be.trades()
            out.append((np.reshape(D, (-1, 2)) * 2.0 ** -j, np.reshape(L, (-1, 2)) * 2.0 ** -j))
        finally:
            be.close()
    for D, L in out[1:]:
        np.testing.assert_array_equal(D, out[0][0])
        np.testing.assert_array_equal(L, out[0][1])
