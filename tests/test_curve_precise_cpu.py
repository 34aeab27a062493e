"""The 60-digit Curve fixture tests/golden/curve_precise.npz on the CPU: its truth re-derived at 80 digits, the CPU reference
(tests/curve_ref.py) and the device's own solve built for the host (tests/native/curve_host.cpp: curve_pool.h's
curve_solve<N>, the template the kernel runs) held to the scale-aware bounds of tests/curve_precise_ref.py on every row,
and metamorphic relations the solve must keep.  The device paths are held to the same bounds in
tests/test_gpu_curve_precise.py."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
import curve_precise_ref as P
import curve_ref as cv

C, CLS = P.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "curve_host.cpp")

# K per class: the next power of two >= 2x the largest ratio measured over every path (printed with -s; the device and
# this host build give the same ratios), at most 16 on the well-conditioned classes and 64 elsewhere.  Two exceptions:
# band_edge 4 (0.28 on the fixture, 1.01 once R -> 2^-8·R in the metamorphic check) and wide 64 (36.2 measured: the cap,
# 1.8x headroom).  Measured maxima: profiles/curve_precise_gpu_tests.log.
K_HOST = {"well": 8, "stiff": 2, "small_a": 4, "alpha0": 2, "drained": 32, "band_edge": 4, "on_bp": 2, "near_bp": 2,
          "ties": 8, "low_gamma": 32, "wide": 64, "range": 1, "far_start": 4, "band": 1}
K_REF = {"well": 4, "stiff": 8, "small_a": 4, "alpha0": 16, "drained": 32, "band_edge": 8, "on_bp": 16, "near_bp": 16,
         "ties": 4, "low_gamma": 32, "wide": 32, "range": 16, "far_start": 16, "band": 1}

def _k(table, cls):
    return np.array([table[CLS[c]] for c in cls], dtype=np.float64)


def _generator():
    path = os.path.join(ROOT, "tests", "golden", "make_curve_golden.py")
    spec = importlib.util.spec_from_file_location("make_curve_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """curve_solve<N> built for the host with the Makefile's host flags, loaded with ctypes -> solve(R, v, α, β, γ)."""
    so = str(tmp_path_factory.mktemp("curve_host") / "curve_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3",
                    "-ffp-contract=off", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.curve_host_solve.argtypes = [ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp, dp, dp, dp,
                                     ctypes.POINTER(ctypes.c_int32)]

    def solve(R, v, alpha, beta, gamma):
        R, v = (np.ascontiguousarray(x, dtype=np.float64) for x in (R, v))
        alpha, beta, gamma = (np.ascontiguousarray(np.broadcast_to(x, R.shape[:1]), dtype=np.float64)
                              for x in (alpha, beta, gamma))
        m, n = R.shape
        D, L, ref = np.empty((m, n)), np.empty((m, n)), np.empty(m, dtype=np.int32)
        p = lambda a: a.ctypes.data_as(dp)
        assert lib.curve_host_solve(n, m, p(R), p(v), p(alpha), p(beta), p(gamma), p(D), p(L),
                                    ref.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
        return D, L, ref.astype(bool)

    return solve


def test_fixture_shape():
    assert os.path.getsize(P.PATH) <= 1 << 20
    assert sorted(C) == [f"c_{N}" for N in range(2, 9)]
    for name, c in C.items():
        N = int(name.split("_")[1])
        assert c["R"].shape[1] == N and len(c["v"]) >= 32
        assert set(np.unique(c["cls"])) == set(range(len(CLS))), name
        for k in range(len(CLS)):
            assert np.count_nonzero(c["cls"] == k) >= 16, (name, CLS[k])
        band = c["cls"] == CLS.index("band")
        assert np.all(c["D"][band] == 0) and np.all(c["L"][band] == 0)
        assert not np.any(np.signbit(c["D"])) and not np.any(np.signbit(c["L"]))
        trades = np.any(c["D"] > 0, axis=1) & np.any(c["L"] > 0, axis=1)
        assert np.count_nonzero(trades[~band]) >= 0.75 * np.count_nonzero(~band), name
        assert np.all(np.isfinite(c["cD"])) and np.all(np.isfinite(c["cL"]))
    assert "v2" in C["c_3"]
    c = C["c_2"]   # the range examples: α = 0 trades like Product at any β; α = 1 takes coin 1 in for the coin it drains
    rng_rows = np.flatnonzero(c["cls"] == CLS.index("range"))[:2]
    for i in rng_rows:
        assert c["D"][i, 0] > 1e9 and c["L"][i, 1] > 1e9


def _sample(rng, count):
    rows = [(name, i) for name, c in sorted(C.items()) for i in range(len(c["gamma"]))]
    return [rows[j] for j in rng.choice(len(rows), count, replace=False)]


def test_truth_rederived_at_80_digits_is_bit_equal():
    """Seeded rows: the stored float64 truth is the 80-digit value rounded once."""
    mp = pytest.importorskip("mpmath")
    gen = _generator()
    rng = np.random.default_rng(80)
    with mp.workdps(80):
        for name, i in _sample(rng, 64):
            c = C[name]
            D, L, _ = gen.curve_truth(c["R"][i], c["alpha"][i], c["beta"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
            assert [gen._f(x) for x in D] == list(c["D"][i]) and [gen._f(x) for x in L] == list(c["L"][i]), (name, i)


@pytest.mark.parametrize("name", sorted(C))
def test_reference_meets_the_bound(name):
    """curve_ref.solve within K_REF·u·scale, except on the pools where its float64 P₀/R_k leaves the range (predicted)."""
    c = C[name]
    with np.errstate(all="ignore"):
        D, L = cv.solve(c["R"], c["alpha"], c["beta"], c["gamma"], c["v"][c["Ai"] - 1])
    bD, bL = P.scale(c)
    r = P.ratios(D, L, c["D"], c["L"], bD, bL)
    pred = P.ref_out_of_range(c["R"], c["alpha"], c["beta"])
    print(f"\n[curve_ref] {name}: {P.class_max(np.where(pred, 0.0, r), c['cls'], CLS)}; {int(pred.sum())} predicted "
          f"out-of-range pools, {int(np.count_nonzero(r[pred] > 64))} of them off")
    kk = _k(K_REF, c["cls"])
    assert np.all(r[~pred] <= kk[~pred]), (np.flatnonzero(~pred & (r > kk))[:8], r[~pred & (r > kk)][:8])
    assert np.all(pred <= np.isin(c["cls"], [CLS.index("range"), CLS.index("alpha0")]))


@pytest.mark.parametrize("name", sorted(C))
def test_host_build_of_the_device_solve_meets_the_bound(name, host):
    """curve_solve<N> as the device runs it, on every row: the refused pools are exactly the predicted ones, every other
    pool within K_HOST·u·scale."""
    c = C[name]
    D, L, ref = host(c["R"], c["v"][c["Ai"] - 1], c["alpha"], c["beta"], c["gamma"])
    np.testing.assert_array_equal(ref, P.refused(c["R"], c["alpha"], c["beta"]))
    bD, bL = P.scale(c)
    r = np.where(ref, 0.0, P.ratios(D, L, c["D"], c["L"], bD, bL))
    print(f"\n[host] {name}: {P.class_max(r, c['cls'], CLS)}; {int(ref.sum())} refused")
    kk = _k(K_HOST, c["cls"])
    bad = r > kk
    assert not np.any(bad), (np.flatnonzero(bad)[:8], r[bad][:8], [CLS[k] for k in c["cls"][bad][:8]])
    band = c["cls"] == CLS.index("band")
    assert np.all(D[band] == 0) and not np.any(np.signbit(D[band])) and np.all(L[band] == 0)


def test_range_refusals_match_the_python_constructors():
    c = C["c_2"]
    ref = P.refused(c["R"], c["alpha"], c["beta"])
    assert np.any(ref)
    i = int(np.flatnonzero(ref)[0])
    with pytest.raises(cr.ArgumentError, match="log"):
        cr.Curve(c["R"][i], c["gamma"][i], c["Ai"][i], c["alpha"][i], c["beta"][i])
    with pytest.raises(cr.ArgumentError, match="log"):
        cr.Curve.batch(c["R"], c["gamma"], c["Ai"], c["alpha"], c["beta"])
    ok = ~ref
    b = cr.Curve.batch(c["R"][ok], c["gamma"][ok], c["Ai"][ok], c["alpha"][ok], c["beta"][ok])
    assert len(b) == np.count_nonzero(ok)


# ---- metamorphic relations, on the host build and on curve_ref ---------------------------------------------------

def _solvers(host):
    def ref(R, v, a, b, g):
        with np.errstate(all="ignore"):
            D, L = cv.solve(R, np.broadcast_to(a, R.shape[:1]), np.broadcast_to(b, R.shape[:1]),
                            np.broadcast_to(g, R.shape[:1]), v)
        return D, L
    return {"host": lambda *a: host(*a)[:2], "curve_ref": ref}


def _rows(c, which):
    """the rows a solver is held to: for curve_ref, those inside its range and outside the wide class (its bracket of
    12 doublings misses some wide pools once the coins are permuted); every row the upload accepts for the host build"""
    if which == "host":
        return np.flatnonzero(~P.refused(c["R"], c["alpha"], c["beta"]))
    keep = ~P.ref_out_of_range(c["R"], c["alpha"], c["beta"]) & (c["cls"] != CLS.index("wide"))
    return np.flatnonzero(keep)


@pytest.mark.parametrize("which", ["host", "curve_ref"])
def test_alpha_zero_trades_do_not_depend_on_beta(which, host):
    solve = _solvers(host)[which]
    for name, c in sorted(C.items()):
        rows = np.intersect1d(_rows(c, which), np.flatnonzero(c["alpha"] == 0))
        vl = c["v"][c["Ai"][rows] - 1]
        bD, bL = P.scale(c, rows)
        for f in (2.0 ** -300, 2.0 ** 200):
            b2 = c["beta"][rows] * f
            keep = ~P.ref_out_of_range(c["R"][rows], c["alpha"][rows], b2) if which == "curve_ref" else slice(None)
            D, L = solve(c["R"][rows], vl, c["alpha"][rows], b2, c["gamma"][rows])
            r = P.ratios(D, L, c["D"][rows], c["L"][rows], bD, bL)[keep]
            assert np.all(r <= 16), (name, f, np.max(r))


@pytest.mark.parametrize("which", ["host", "curve_ref"])
def test_scaling_all_prices_by_a_power_of_two_is_bit_identical(which, host):
    solve = _solvers(host)[which]
    for name, c in sorted(C.items()):
        rows = _rows(c, which)
        R, vl, a, b, g = c["R"][rows], c["v"][c["Ai"][rows] - 1], c["alpha"][rows], c["beta"][rows], c["gamma"][rows]
        D0, L0 = solve(R, vl, a, b, g)
        for j in (-37, 5, 60):
            D, L = solve(R, vl * 2.0 ** j, a, b, g)
            np.testing.assert_array_equal(D, D0, err_msg=f"{name} 2^{j}")
            np.testing.assert_array_equal(L, L0, err_msg=f"{name} 2^{j}")


@pytest.mark.parametrize("which", ["host", "curve_ref"])
def test_scaling_reserves_scales_the_trades(which, host):
    """R -> 2^j·R, β -> 2^{j(N+1)}·β: the same pool in other units, trades ×2^j within the bound."""
    solve = _solvers(host)[which]
    for name, c in sorted(C.items()):
        N = c["R"].shape[1]
        for j in (-8, 11):
            b2 = c["beta"] * 2.0 ** (j * (N + 1))
            rows = _rows(c, which)
            bD, bL = P.scale(c, rows)
            D, L = solve(c["R"][rows] * 2.0 ** j, c["v"][c["Ai"][rows] - 1], c["alpha"][rows], b2[rows], c["gamma"][rows])
            r = P.ratios(D * 2.0 ** -j, L * 2.0 ** -j, c["D"][rows], c["L"][rows], bD, bL)
            kk = _k(K_HOST if which == "host" else K_REF, c["cls"][rows])
            assert np.all(r <= kk), (name, j, np.flatnonzero(r > kk)[:8], r[r > kk][:8])


@pytest.mark.parametrize("which", ["host", "curve_ref"])
def test_permuting_the_coins_permutes_the_trades(which, host):
    solve = _solvers(host)[which]
    rng = np.random.default_rng(11)
    for name, c in sorted(C.items()):
        rows = _rows(c, which)
        N = c["R"].shape[1]
        p = rng.permutation(N)
        while N > 1 and np.all(p == np.arange(N)):
            p = rng.permutation(N)
        bD, bL = P.scale(c, rows)
        D, L = solve(c["R"][rows][:, p], c["v"][c["Ai"][rows] - 1][:, p], c["alpha"][rows], c["beta"][rows],
                     c["gamma"][rows])
        r = P.ratios(D, L, c["D"][rows][:, p], c["L"][rows][:, p], bD[:, p], bL[:, p])
        kk = _k(K_HOST if which == "host" else K_REF, c["cls"][rows])
        assert np.all(r <= kk), (name, np.flatnonzero(r > kk)[:8], r[r > kk][:8])
