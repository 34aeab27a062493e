"""cfmm_swap's per-kind forms on the CPU: csrc/swap_pool.h + quote_pool.h + univ3_pool.h built for the host
(tests/native/swap_host.cpp: the functions swap_kernel runs, applied in query order as the kernel and the host apply them)
held to the 80-digit sequences of tests/golden/swap_precise.npz within tests/swap_precise_ref.py's bounds; the exact
properties that need no tolerance; the wave numbering; and the same shim once as a stand-alone program under the address and
undefined-behaviour sanitizers.  The device is held to the same K in tests/test_gpu_swap_precise.py.

K table (swap_precise_ref.K_MEASURED, re-measured here): worst ratio of the host build -> K = next power of two >= 2x it:
    product    balanced 0.27, typical 0.30, lopsided 0.10, low_gamma 0.15 -> 1
    geomean    balanced 0.34, typical 0.28, lopsided 0.45, low_gamma 0.22 -> 1
    weighted   balanced 0.38, typical 0.33, lopsided 0.43, low_gamma 0.15 -> 1
    solidly    balanced 2.4, typical 2.5, lopsided 2.3 -> 8, low_gamma 1.8 -> 4
    curve      balanced 0.37, typical 0.40, lopsided 0.42, low_gamma 0.34 -> 1
    univ3      one_tick 0.13, two_ticks 0.082, tick_edge 0.045, crosses 0.18, empty_tick 0.041, exhausted 0.074, reversal 0.24 -> 1"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quote_precise_ref as Q
import swap_precise_ref as S
from test_quote_precise_cpu import host as quote_host  # noqa: F401  (the quote shim: `out` equals quote_* of the same state)
from test_quote_precise_cpu import host_pools, host_univ3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "swap_host.cpp")
D, I32, I64 = ctypes.c_double, ctypes.c_int32, ctypes.c_int64


@pytest.fixture(scope="module")
def fx():
    assert os.path.getsize(S.FIXTURE) <= 1 << 20
    return S.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("swap_host") / "swap_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp, ip, lp = ctypes.POINTER(D), ctypes.POINTER(I32), ctypes.POINTER(I64)
    lib.swap_host_pool.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, D, D, D, ctypes.c_int, ip, ip, dp, dp, dp, dp]
    lib.swap_host_univ3.argtypes = [D, D, I64, dp, dp, ctypes.c_int, ip, dp, dp, dp]
    lib.swap_host_waves.argtypes = [I64, lp, lp, lp, lp]
    lib.swap_host_waves.restype = I64
    return lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def swap_pool(lib, fam, R, gamma, cin, cout, a, w=None, alpha=0.0, beta=1.0):
    """-> (out [steps], R after every step [steps, n], refreshed constants [steps, 2])"""
    R = np.array(R, dtype=np.float64)
    n, steps = R.size, len(a)
    w = np.ones(n) if w is None else np.ascontiguousarray(w, dtype=np.float64)
    cin, cout = np.ascontiguousarray(cin, dtype=np.int32), np.ascontiguousarray(cout, dtype=np.int32)
    a = np.ascontiguousarray(a, dtype=np.float64)
    out, Rs, konst = np.empty(steps), np.empty((steps, n)), np.empty((steps, 2))
    rc = lib.swap_host_pool(S.KIND[fam], n, _p(R, D), _p(w, D), float(alpha), float(beta), float(gamma), steps, _p(cin, I32),
                            _p(cout, I32), _p(a, D), _p(out, D), _p(Rs, D), _p(konst, D))
    assert rc == 0
    return out, Rs, konst


def swap_univ3(lib, cp, gamma, lt, lq, cin, a):
    lt, lq = np.ascontiguousarray(lt, dtype=np.float64), np.ascontiguousarray(lq, dtype=np.float64)
    cin, a = np.ascontiguousarray(cin, dtype=np.int32), np.ascontiguousarray(a, dtype=np.float64)
    out, price = np.empty(a.size), np.empty(a.size)
    rc = lib.swap_host_univ3(float(cp), float(gamma), lt.size, _p(lt, D), _p(lq, D), a.size, _p(cin, I32), _p(a, D), _p(out, D), _p(price, D))
    assert rc == 0
    return out, price


def run_host(lib):
    def run(name, g, s):
        n = int(g["nsteps"][s])
        if name == "univ3":
            o, e = g["tick_off"][s], g["tick_off"][s + 1]
            out, price = swap_univ3(lib, g["cp"][s], g["gamma"][s], g["lower_ticks"][o:e], g["liquidity"][o:e], g["cin"][s, :n], g["a"][s, :n])
            return out, price[-1]
        out, Rs, _ = swap_pool(lib, Q.family(name), g["R0"][s], g["gamma"][s], g["cin"][s, :n], g["cout"][s, :n], g["a"][s, :n],
                               g["w"][s], g["alpha"][s], g["beta"][s])
        return out, Rs[-1]
    return run


def test_K_table_is_what_the_host_build_measures(fx, host):
    w = S.worst_by_class(fx, run_host(host))
    for key in sorted(w):
        print(f"    {key!r}: {w[key]:.3g},")
    assert set(w) == set(S.K_MEASURED)
    for key, worst in w.items():
        assert worst <= S.K_MEASURED[key] * 1.01 + 1e-300, (key, worst)
        S.K_of(*key)                                                     # within the cap


def test_fixture_covers_what_the_issue_names(fx):
    for name in S.RESERVE_GROUPS:
        g = S.group(fx, name)
        assert {"balanced", "typical", "lopsided", "low_gamma"} <= set(g["cls"]), name
        assert set(g["nsteps"]) == {1, 2, 3, 4}
    g = S.group(fx, "univ3")
    assert {"one_tick", "two_ticks", "tick_edge", "crosses", "empty_tick", "exhausted", "reversal"} <= set(g["cls"])
    assert {1, 2, 5} <= set(np.diff(g["tick_off"]))
    s = list(g["cls"]).index("tick_edge")
    assert g["price"][s, 0] == 1.0 and g["out"][s, 0] == 6.0            # the swap that ends exactly on a tick edge
    s = list(g["cls"]).index("exhausted")
    assert g["price"][s, 0] == g["lower_ticks"][g["tick_off"][s]] and g["out"][s, 1] == 0.0


# ---- exact properties ---------------------------------------------------------------------------------------------------------
def test_out_equals_the_quote_of_the_same_state(fx, host, quote_host):
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            out, Rs, _ = swap_pool(host, fam, g["R0"][s], g["gamma"][s], g["cin"][s, :n], g["cout"][s, :n], g["a"][s, :n], g["w"][s],
                                   g["alpha"][s], g["beta"][s])
            before = np.vstack([g["R0"][s][None, :], Rs[:-1]])
            rep = lambda x: np.repeat(np.atleast_1d(x), n)
            kw = {}
            if fam in ("geomean", "weighted"):
                kw["w"] = np.tile(g["w"][s], (n, 1))
            if fam == "curve":
                kw.update(alpha=rep(g["alpha"][s]), beta=rep(g["beta"][s]))
            q = host_pools(quote_host, fam, before, rep(g["gamma"][s]), g["cin"][s, :n], g["cout"][s, :n], g["a"][s, :n], **kw)
            np.testing.assert_array_equal(out.view(np.uint64), q.view(np.uint64), err_msg=f"{name} {s}")
    g = S.group(fx, "univ3")
    for s in range(len(g["cls"])):
        n = int(g["nsteps"][s])
        o, e = g["tick_off"][s], g["tick_off"][s + 1]
        out, price = swap_univ3(host, g["cp"][s], g["gamma"][s], g["lower_ticks"][o:e], g["liquidity"][o:e], g["cin"][s, :n], g["a"][s, :n])
        cps = np.concatenate([[g["cp"][s]], price[:-1]])
        for j in range(n):
            gg = {"current_price": cps[j:j + 1], "pool_gamma": g["gamma"][s:s + 1], "lower_ticks": g["lower_ticks"][o:e],
                  "liquidity": g["liquidity"][o:e], "tick_off": np.array([0, e - o]), "pool": np.zeros(1, dtype=np.int64),
                  "cin": g["cin"][s, j:j + 1], "a": g["a"][s, j:j + 1]}
            q = host_univ3(quote_host, gg)
            assert q.view(np.uint64)[0] == out.view(np.uint64)[j], (s, j)


def test_new_reserves_are_R_plus_gamma_a_and_R_minus_out(fx, host):
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            out, Rs, _ = swap_pool(host, fam, g["R0"][s], g["gamma"][s], g["cin"][s, :n], g["cout"][s, :n], g["a"][s, :n], g["w"][s],
                                   g["alpha"][s], g["beta"][s])
            R = np.array(g["R0"][s], copy=True)
            for j in range(n):
                ci, co = g["cin"][s, j], g["cout"][s, j]
                R[ci] = R[ci] + g["gamma"][s] * g["a"][s, j]           # each operation rounded on its own
                R[co] = R[co] - out[j]
                np.testing.assert_array_equal(Rs[j].view(np.uint64), R.view(np.uint64), err_msg=f"{name} {s} step {j}")


def test_zero_amount_leaves_every_bit_of_the_state(fx, host):
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            out, Rs, konst = swap_pool(host, fam, g["R0"][s], g["gamma"][s], g["cin"][s, :1], g["cout"][s, :1], [0.0], g["w"][s],
                                       g["alpha"][s], g["beta"][s])
            assert out.view(np.uint64)[0] == 0 and np.all(konst == 0.0)           # +0.0, and no constant was rewritten
            np.testing.assert_array_equal(Rs[0].view(np.uint64), np.asarray(g["R0"][s]).view(np.uint64))
    g = S.group(fx, "univ3")
    for s in range(len(g["cls"])):
        o, e = g["tick_off"][s], g["tick_off"][s + 1]
        for ci in (0, 1):
            out, price = swap_univ3(host, g["cp"][s], g["gamma"][s], g["lower_ticks"][o:e], g["liquidity"][o:e], [ci], [0.0])
            assert out.view(np.uint64)[0] == 0 and price.view(np.uint64)[0] == np.float64(g["cp"][s]).view(np.uint64)


def test_a_swap_that_would_empty_the_pool_is_refused(host):
    out, Rs, _ = swap_pool(host, "product", [100.0, 250.0], 0.997, [0, 0], [1, 1], [1e30, 1.0])
    assert np.isnan(out[0]) and out[1] > 0
    np.testing.assert_array_equal(Rs[0], [100.0, 250.0])                          # the pool stays; the next swap starts from it
    out, Rs, _ = swap_pool(host, "solidly", [2.0 ** -100, 1.0], 1.0, [1], [0], [2.0 ** 60])
    assert np.isnan(out[0]) or Rs[0, 0] >= 2.0 ** -150                            # a Solidly reserve never leaves the window


def waves_of(lib, rows):
    idx = np.ascontiguousarray(rows, dtype=np.int64)
    n = idx.size
    wave, perm, off = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64), np.zeros(n + 2, dtype=np.int64)
    nw = lib.swap_host_waves(n, _p(idx, I64), _p(wave, I64), _p(perm, I64), _p(off, I64))
    return nw, wave, perm, off[:nw + 1]


def test_wave_numbering(host):
    nw, wave, perm, off = waves_of(host, [5, 2, 5, 5, 2])
    assert nw == 3 and list(wave) == [0, 0, 1, 2, 1]
    assert list(off) == [0, 2, 4, 5] and list(perm) == [1, 0, 4, 2, 3]             # rows ascending within a wave
    nw, wave, perm, off = waves_of(host, [5, 2, 5, 7, 5, 2])
    assert list(wave) == [0, 0, 1, 0, 2, 1] and list(perm) == [1, 0, 3, 5, 2, 4] and list(off) == [0, 3, 5, 6]
    nw, wave, perm, off = waves_of(host, [9, 3, 4])                                # distinct rows: one launch
    assert nw == 1 and list(wave) == [0, 0, 0] and list(perm) == [1, 2, 0]
    n = np.int64(4)
    wave, perm, off = np.empty(4, dtype=np.int64), np.empty(4, dtype=np.int64), np.zeros(6, dtype=np.int64)
    assert host.swap_host_waves(n, None, _p(wave, I64), _p(perm, I64), _p(off, I64)) == 1      # idx == NULL: rows 0 .. count-1
    assert list(wave) == [0] * 4 and list(perm) == [0, 1, 2, 3]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "swap_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DSWAP_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SHIM, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "SWAP_HOST_OK" in r.stdout and r.stderr == ""
    assert "waves 3: 0 0 1 2 1" in r.stdout
