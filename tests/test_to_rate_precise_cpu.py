"""The amount to a target rate on the CPU: csrc/to_rate_pool.h built for the host (tests/native/to_rate_host.cpp, the functions
the kernels run) held to BOTH bounds of tests/to_rate_precise_ref.py on every row of the 80-digit fixture -- the amount itself,
and the round trip in rate space -- at the K the numpy restatement of the forms measured; exactly +0.0 where the spot rate is
at or below the limit, exactly the capacity where a UniV3 direction is exhausted, monotone in the limit, the Curve search below
its cap on every row; and the same shim once as a stand-alone program under the address and undefined-behaviour sanitizers.
The device is held to the same K in tests/test_gpu_to_rate_precise.py.

K (python tests/to_rate_precise_ref.py; next power of two >= 2x the restatement's worst ratio, cap 16 / 64), amount | rate:
    product    at most 1.1 | 1.2 -> 4         geomean    at most 5.5 | 5.4 (w02_98) -> 16, typical 3.5 | 3.3 -> 8
    weighted   at most 5.6 | 5.8 (w02_98) -> 16, typical 2.4 | 2.3 -> 8
    solidly    at most 2.0 | 2.4 -> 4 / 8     curve      at most 1.3 | 1.1 -> 4      univ3      at most 0.70 | 0.46 -> 2
The Curve search (numpy's libm) made at most 101 evaluations of the rate on a fixture row (median 7, 90th percentile 20): the
cap is 128."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import quote_precise_ref as P
import rate_precise_ref as RP
import to_rate_precise_ref as TP
from test_quote_precise_cpu import KIND, _p

ROOT = P.ROOT
SHIM = os.path.join(ROOT, "tests", "native", "to_rate_host.cpp")


@pytest.fixture(scope="module")
def fxs():
    assert os.path.getsize(TP.FIXTURE) <= 1 << 20
    return TP.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """to_rate_pool.h built for the host with the Makefile's host flags, loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("to_rate_host") / "to_rate_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.to_rate_host_pools.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp, dp, ip, ip, dp, dp, dp, ip]
    lib.to_rate_host_univ3.argtypes = [ctypes.c_int64, dp, dp, lp, dp, dp, ctypes.c_int64, lp, ip, dp, dp, dp]
    return lib


def host_group(lib, fxs, gname):
    """(amount, rate at the amount, Curve evaluations, the group) of the host build over one group of the fixture"""
    g = TP.group(fxs, gname)
    f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)   # noqa: E731
    r = f(g["r"])
    amount, back, iters = np.empty(r.size), np.empty(r.size), np.zeros(r.size, dtype=np.int32)
    D = ctypes.c_double
    if gname == "univ3":
        cp, gm, lt, lq = f(g["current_price"]), f(g["pool_gamma"]), f(g["lower_ticks"]), f(g["liquidity"])
        off = np.ascontiguousarray(g["tick_off"], dtype=np.int64)
        pool, cin = np.ascontiguousarray(g["pool"], dtype=np.int64), np.ascontiguousarray(g["cin"], dtype=np.int32)
        rc = lib.to_rate_host_univ3(cp.size, _p(cp, D), _p(gm, D), _p(off, ctypes.c_int64), _p(lt, D), _p(lq, D), r.size,
                                    _p(pool, ctypes.c_int64), _p(cin, ctypes.c_int32), _p(r, D), _p(amount, D), _p(back, D))
    else:
        R, gamma, w, alpha, beta = f(g["R"]), f(g["gamma"]), f(g.get("w")), f(g.get("alpha")), f(g.get("beta"))
        cin, cout = np.ascontiguousarray(g["cin"], dtype=np.int32), np.ascontiguousarray(g["cout"], dtype=np.int32)
        rc = lib.to_rate_host_pools(KIND[P.family(gname)], R.shape[1], r.size, _p(R, D), _p(w, D), _p(alpha, D), _p(beta, D),
                                    _p(gamma, D), _p(cin, ctypes.c_int32), _p(cout, ctypes.c_int32), _p(r, D), _p(amount, D),
                                    _p(back, D), _p(iters, ctypes.c_int32))
    assert rc == 0
    return amount, back, iters, g


def assert_within(amount, back, g, gname, label):
    ra, rr = TP.ratios(amount, g), TP.rate_ratios(back, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K, Kr = TP.K_of(gname, str(c)), TP.K_rate_of(gname, str(c))
        worst, worst_r = float(np.max(ra[sel])), float(np.max(rr[sel]))
        print(f"{label} {gname}/{c}: amount worst {worst:.3g} of K = {K}, rate worst {worst_r:.3g} of K = {Kr}")
        assert not np.any(np.isnan(amount[sel])) and worst <= K, (gname, c, worst, K)
        assert worst_r <= Kr, (gname, c, worst_r, Kr)


def assert_exact_rows(amount, g, gname):
    zero = g["a"] == 0.0
    assert np.all(amount[zero].view(np.uint64) == 0)                       # exactly +0.0, the sign included
    if gname == "univ3":   # the capacity: the closing record's Σδmax over γ, as the upload prepares the records
        cap = np.flatnonzero(g["capacity"])
        assert cap.size > 0
        for j in cap:
            p, ci = int(g["pool"][j]), int(g["cin"][j])
            _, up, lo = P.univ3_prepare(*P.univ3_pool(g, p)[:3])
            want = np.float64((up if ci == 0 else lo)[-1][5]) / np.float64(g["pool_gamma"][p])
            assert amount[j].view(np.uint64) == want.view(np.uint64), (j, amount[j], want)


def assert_monotone(amount, g, gname):
    """r1 < r2 => a(r1) >= a(r2) over each pool's (and coin pair's) limits"""
    key = g["pool"] * 2 + g["cin"] if gname == "univ3" else g["row"]
    for k in np.unique(key):
        sel = np.flatnonzero(key == k)
        order = sel[np.argsort(g["r"][sel], kind="stable")]
        assert np.all(np.diff(amount[order]) <= 0.0), (gname, int(k), g["r"][order], amount[order])


def test_K_tables_are_what_the_restatement_measures(fxs):
    w, wr, most = TP.worst_by_class(fxs)
    assert set(w) == set(TP.K_MEASURED) == set(wr) == set(TP.K_MEASURED_RATE)
    for key in w:
        assert w[key] <= TP.K_MEASURED[key] * 1.01 + 1e-300, (key, w[key])
        assert wr[key] <= TP.K_MEASURED_RATE[key] * 1.01 + 1e-300, (key, wr[key])
    for gname in TP.GROUPS:
        for c in np.unique(TP.group(fxs, gname)["cls"]):
            TP.K_of(gname, str(c))
            TP.K_rate_of(gname, str(c))
    print("largest Curve evaluation count of the restatement:", most)
    assert most < TP.CURVE_ITERS


def test_fixture_covers_every_class_and_an_eighth_of_it_is_zero(fxs):
    """every (family, class) of the rate fixture's K table has rows; the ladder of limits per pool; at least one eighth of the
    rows have truth 0; the UniV3 rows the issue names are there; a few thousand rows"""
    qfx, _ = fxs
    total = zeros = 0
    have = set()
    for gname in TP.GROUPS:
        g = TP.group(fxs, gname)
        total += g["a"].size
        zeros += int(np.sum(g["a"] == 0.0))
        have |= {(P.family(gname), str(c)) for c in np.unique(g["cls"])}
        assert np.all(np.isfinite(g["r"])) and np.all(g["r"] > 0.0) and np.all(g["a"] >= 0.0) and np.all(g["cond"] >= 0.0)
        assert np.all(g["a"][g["interior"]] > 0.0) and np.all(np.isfinite(g["rcond"]))
        if gname != "univ3":
            n = P.group(qfx, gname)["a"].size
            assert set(g["row"]) == set(range(n))                          # every pool of the quote fixture
            assert np.all(g["interior"] == (g["a"] > 0.0))
            counts = np.bincount(g["row"], minlength=n)
            assert counts.min() >= 4 and counts.max() == 8                 # the ladder (less what would leave no valid pool) and r >= s twice
    assert have == set(RP.K_MEASURED), have ^ set(RP.K_MEASURED)
    assert 2000 <= total <= 5000 and 8 * zeros >= total, (total, zeros)
    u = TP.group(fxs, "univ3")
    assert u["zero"].sum() >= 2 * 5 and u["capacity"].any() and np.all(u["a"][u["zero"]] == 0.0)
    assert {"in_tick", "depth4", "depth64", "boundary_dn", "boundary_up", "empty_in_path", "exhausted", "empty_current"} <= set(u["cls"])


@pytest.mark.parametrize("gname", TP.GROUPS)
def test_restatement_exact_rows_and_monotone(fxs, gname):
    amount, _, _, g = TP.restatement(fxs, gname)
    assert_exact_rows(amount, g, gname)
    assert_monotone(amount, g, gname)


@pytest.mark.parametrize("gname", TP.GROUPS)
def test_host_build_within_both_bounds(fxs, host, gname):
    amount, back, iters, g = host_group(host, fxs, gname)
    assert_within(amount, back, g, gname, "host")
    assert_exact_rows(amount, g, gname)
    assert_monotone(amount, g, gname)
    if P.family(gname) == "curve":
        cap = host.to_rate_host_curve_cap()
        print(f"host {gname}: Curve evaluations: median {int(np.median(iters))}, largest {int(iters.max())} of the cap {cap}")
        assert cap == TP.CURVE_ITERS and 0 < iters.max() < cap


def write_blocks(path, fxs):
    """the fixture's queries as tests/native/to_rate_host.cpp's main reads them"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()   # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).tobytes()     # noqa: E731
    with open(path, "wb") as f:
        for gname in TP.GROUPS:
            g = TP.group(fxs, gname)
            if gname == "univ3":
                f.write(struct.pack("<4q", 2, g["current_price"].size, g["r"].size, g["lower_ticks"].size))
                f.write(f64(g["current_price"]) + f64(g["pool_gamma"]) + i64(g["tick_off"]) + f64(g["lower_ticks"]) +
                        f64(g["liquidity"]) + i64(g["pool"]) + i64(g["cin"]) + f64(g["r"]))
                continue
            kind = KIND[P.family(gname)]
            f.write(struct.pack("<4q", 1, kind, g["R"].shape[1], g["r"].size))
            f.write(f64(g["R"]))
            if kind in (1, 3):
                f.write(f64(g["w"]))
            if kind == 4:
                f.write(f64(g["alpha"]) + f64(g["beta"]))
            f.write(f64(g["gamma"]) + i64(g["cin"]) + i64(g["cout"]) + f64(g["r"]))


def test_stand_alone_program_under_the_sanitizers(fxs, tmp_path):
    """The same shim with its own main, built with -fsanitize=address,undefined, run as a program on the fixture: clean, and
    within both bounds."""
    exe, inp, outp = str(tmp_path / "to_rate_host"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DTO_RATE_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SHIM,
                    "-o", exe], check=True)
    write_blocks(inp, fxs)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "TO_RATE_HOST_OK" in r.stdout and r.stderr == ""
    res = np.fromfile(outp, dtype=np.float64)
    at = 0
    for gname in TP.GROUPS:
        g = TP.group(fxs, gname)
        n = g["r"].size
        assert_within(res[at:at + n], res[at + n:at + 2 * n], g, gname, "sanitized")
        at += 2 * n
    assert at == res.size
