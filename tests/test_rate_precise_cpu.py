"""Marginal rates on the CPU: csrc/rate_pool.h built for the host (tests/native/rate_host.cpp, the functions the kernel runs)
held to the bounds of tests/rate_precise_ref.py on every row of the 80-digit fixture, at the K the numpy restatement of the
forms measured; its amounts out against the host build of quote_pool.h bit for bit; and the same shim once as a stand-alone
program under the address and undefined-behaviour sanitizers.  The device is held to the same K in
tests/test_gpu_rate_precise.py.

K table (python tests/rate_precise_ref.py; K = next power of two >= 2x the restatement's worst ratio, cap 16 / 64):
    family     class: worst -> K
    product    tiny 0.46 -> 1, typical 0.44 -> 1, huge 0.45 -> 1, lopsided 0.46 -> 1, low_gamma 0.45 -> 1
    geomean    tiny 0.32 -> 1, typical 0.52 -> 2, huge 0.51 -> 2, lopsided 0.48 -> 1, low_gamma 0.43 -> 1, w02_98 0.31 -> 1
    weighted   tiny 0.32 -> 1, typical 0.61 -> 2, huge 0.30 -> 1, lopsided 0.37 -> 1, low_gamma 0.96 -> 2, pairs 0.32 -> 1, w02_98 0.36 -> 1
    solidly    tiny 0.63 -> 2, typical 0.88 -> 2, huge 0.54 -> 2, lopsided 0.47 -> 1, low_gamma 1.3 -> 4, balanced 0.50 -> 1, t0_hi 0.60 -> 2, t0_lo 1.7 -> 4
    curve      tiny 0.72 -> 2, typical 0.74 -> 2, huge 0.55 -> 2, lopsided 0.42 -> 1, low_gamma 0.71 -> 2, stiff 1.0 -> 2, small_a 0.88 -> 2, alpha0 0.94 -> 2
    univ3      in_tick 0.63 -> 2, boundary_dn 0.37 -> 1, boundary_up 0.77 -> 2, depth1 0.56 -> 2, depth4 0.15 -> 1, depth5 0.092 -> 1,
               depth64 0.073 -> 1, empty_in_path 0.23 -> 1, empty_current 0.21 -> 1, last_tick 0.16 -> 1, exhausted 0 -> 1, spot 0.20 -> 1
(Curve with y′ formed as R_o − out measured 7.0e10 on `huge`, 8.8e8 on `lopsided` and 2.3e4 on `stiff`, far above the cap: the
finding that made y′ the root of the quote's quadratic in its difference-free form.)"""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import quote_precise_ref as P
import rate_precise_ref as RP
from test_quote_precise_cpu import KIND, _p, host as quote_host_lib, host_group as quote_host_group  # noqa: F401

ROOT = P.ROOT
SHIM = os.path.join(ROOT, "tests", "native", "rate_host.cpp")


@pytest.fixture(scope="module")
def fxs():
    assert os.path.getsize(RP.FIXTURE) <= 1 << 20
    return RP.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """rate_pool.h built for the host with the Makefile's host flags, loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("rate_host") / "rate_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.rate_host_pools.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp, dp, ip, ip, dp, dp, dp]
    lib.rate_host_univ3.argtypes = [ctypes.c_int64, dp, dp, lp, dp, dp, ctypes.c_int64, lp, ip, dp, dp, dp]
    return lib


def host_group(lib, fxs, gname, a=None):
    """(amount_out, rate, the group) of the host build over one group of the fixture"""
    g = RP.group(fxs, gname)
    f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    a = f(g["a"] if a is None else a)
    out, rate = np.empty(a.size), np.empty(a.size)
    D = ctypes.c_double
    if gname == "univ3":
        cp, gm, lt, lq = f(g["current_price"]), f(g["pool_gamma"]), f(g["lower_ticks"]), f(g["liquidity"])
        off = np.ascontiguousarray(g["tick_off"], dtype=np.int64)
        pool, cin = np.ascontiguousarray(g["pool"], dtype=np.int64), np.ascontiguousarray(g["cin"], dtype=np.int32)
        rc = lib.rate_host_univ3(cp.size, _p(cp, D), _p(gm, D), _p(off, ctypes.c_int64), _p(lt, D), _p(lq, D), a.size,
                                 _p(pool, ctypes.c_int64), _p(cin, ctypes.c_int32), _p(a, D), _p(out, D), _p(rate, D))
    else:
        R, gamma, w, alpha, beta = f(g["R"]), f(g["gamma"]), f(g.get("w")), f(g.get("alpha")), f(g.get("beta"))
        cin, cout = np.ascontiguousarray(g["cin"], dtype=np.int32), np.ascontiguousarray(g["cout"], dtype=np.int32)
        rc = lib.rate_host_pools(KIND[P.family(gname)], R.shape[1], a.size, _p(R, D), _p(w, D), _p(alpha, D), _p(beta, D),
                                 _p(gamma, D), _p(cin, ctypes.c_int32), _p(cout, ctypes.c_int32), _p(a, D), _p(out, D), _p(rate, D))
    assert rc == 0
    return out, rate, g


def assert_within(rate, g, gname, label):
    r = RP.ratios(rate, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K = RP.K_of(gname, str(c))
        worst = float(np.max(r[sel]))
        print(f"{label} {gname}/{c}: worst {worst:.3g} of K = {K}")
        assert np.all(np.isfinite(rate[sel])) and worst <= K, (gname, c, worst, K)


def test_K_table_is_what_the_restatement_measures(fxs):
    """K_MEASURED records the numpy restatement's worst ratios (to its three printed digits), and no class needs more than
    the cap"""
    w = RP.worst_by_class(fxs)
    assert set(w) == set(RP.K_MEASURED)
    for key, worst in w.items():
        assert worst <= RP.K_MEASURED[key] * 1.01 + 1e-300, (key, worst)
    for gname in RP.GROUPS:
        for c in np.unique(RP.group(fxs, gname)["cls"]):
            RP.K_of(gname, str(c))


def test_fixture_is_the_quote_fixture_twice(fxs):
    """every row of quote_precise.npz with its amount and again with a = 0, all ten groups; UniV3: its 64 rows and one a = 0
    row per pool and direction; the flagged rows are the 10 boundary rows and no others"""
    qfx, _ = fxs
    for gname in RP.GROUPS:
        q, g = P.group(qfx, gname), RP.group(fxs, gname)
        n = q["a"].size
        np.testing.assert_array_equal(g["a"][:n], q["a"])
        np.testing.assert_array_equal(g["out"][:n], q["out"])
        assert np.all(g["a"][n:] == 0.0) and np.all(g["out"][n:] == 0.0)
        assert np.all(np.isfinite(g["rate"])) and np.all(g["rate"] >= 0.0) and np.all(g["cond"] >= 0.0)
        if gname == "univ3":
            npools = q["current_price"].size
            assert g["a"].size == n + 2 * npools and set(g["cls"][n:]) == {"spot"}
            assert sorted(zip(g["pool"][n:], g["cin"][n:])) == [(p, c) for p in range(npools) for c in (0, 1)]
            assert np.all(g["rate"][n:] > 0.0)
            flagged = g["at_boundary"]
            assert flagged.sum() == 10 and set(g["cls"][flagged]) == {"boundary_dn", "boundary_up"}
            assert np.all(flagged[np.isin(g["cls"], ("boundary_dn", "boundary_up"))])
            np.testing.assert_array_equal(g["rate_left"][~flagged], g["rate"][~flagged])
            assert np.all(g["rate"][g["cls"] == "exhausted"] == 0.0) and np.all(g["cond"][g["cls"] == "exhausted"] == 0.0)
        else:
            assert g["a"].size == 2 * n
            np.testing.assert_array_equal(g["row"], np.tile(np.arange(n), 2))
            assert np.all(g["rate"][n:] > 0.0)


@pytest.mark.parametrize("gname", RP.GROUPS)
def test_host_build_within_the_bounds(fxs, host, gname):
    _, rate, g = host_group(host, fxs, gname)
    assert_within(rate, g, gname, "host")
    assert np.all(rate[g["cls"] == "exhausted"].view(np.uint64) == 0)


@pytest.mark.parametrize("gname", RP.GROUPS)
def test_amount_out_is_the_quote_builds_bit_for_bit(fxs, host, quote_host_lib, gname):
    """the amounts beside the rates against tests/native/quote_host.cpp, a separate build of quote_pool.h, on the quote
    fixture's own rows; and +0.0 on every a = 0 row"""
    out, _, g = host_group(host, fxs, gname)
    want, q = quote_host_group(quote_host_lib, fxs[0], gname)
    n = q["a"].size
    np.testing.assert_array_equal(out[:n].view(np.uint64), want.view(np.uint64))
    assert np.all(out[g["a"] == 0.0].view(np.uint64) == 0)


def test_rate_is_the_slope_of_the_host_quote(fxs, host):
    """a coarse, form-independent sanity check in doubles: (quote(a(1+e)) − quote(a(1−e)))/(2ae), e = 1e-6, agrees with the
    rate to 1e-4 relative on the `typical` rows of every reserve family (a finite difference in doubles loses half the
    digits: this only catches a wrong formula, the bounds catch a bad one)"""
    e = 1e-6
    for gname in RP.GROUPS[:-1]:
        g = RP.group(fxs, gname)
        sel = (g["cls"] == "typical") & (g["a"] > 0.0)
        up, _, _ = host_group(host, fxs, gname, a=g["a"] * (1 + e))
        dn, _, _ = host_group(host, fxs, gname, a=g["a"] * (1 - e))
        _, rate, _ = host_group(host, fxs, gname)
        fd = (up[sel] - dn[sel]) / (2 * e * g["a"][sel])
        np.testing.assert_allclose(fd, rate[sel], rtol=1e-4)


def write_blocks(path, fxs):
    """the fixture's queries as tests/native/rate_host.cpp's main reads them"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).tobytes()
    with open(path, "wb") as f:
        for gname in RP.GROUPS:
            g = RP.group(fxs, gname)
            if gname == "univ3":
                f.write(struct.pack("<4q", 2, g["current_price"].size, g["a"].size, g["lower_ticks"].size))
                f.write(f64(g["current_price"]) + f64(g["pool_gamma"]) + i64(g["tick_off"]) + f64(g["lower_ticks"]) +
                        f64(g["liquidity"]) + i64(g["pool"]) + i64(g["cin"]) + f64(g["a"]))
                continue
            kind = KIND[P.family(gname)]
            f.write(struct.pack("<4q", 1, kind, g["R"].shape[1], g["a"].size))
            f.write(f64(g["R"]))
            if kind in (1, 3):
                f.write(f64(g["w"]))
            if kind == 4:
                f.write(f64(g["alpha"]) + f64(g["beta"]))
            f.write(f64(g["gamma"]) + i64(g["cin"]) + i64(g["cout"]) + f64(g["a"]))


def test_stand_alone_program_under_the_sanitizers(fxs, tmp_path):
    """The same shim with its own main, built with -fsanitize=address,undefined, run as a program on the fixture: clean, and
    within the bounds (held to the bounds, not to the -O3 build's bits: see tests/test_quote_precise_cpu.py)."""
    exe, inp, outp = str(tmp_path / "rate_host"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DRATE_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SHIM,
                    "-o", exe], check=True)
    write_blocks(inp, fxs)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "RATE_HOST_OK" in r.stdout and r.stderr == ""
    res = np.fromfile(outp, dtype=np.float64)
    at = 0
    for gname in RP.GROUPS:
        g = RP.group(fxs, gname)
        n = g["a"].size
        assert_within(res[at + n:at + 2 * n], g, gname, "sanitized")
        at += 2 * n
    assert at == res.size
