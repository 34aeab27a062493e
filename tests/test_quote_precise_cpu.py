"""Exact-input swap quotes on the CPU: csrc/quote_pool.h built for the host (tests/native/quote_host.cpp, the functions the
kernel runs) held to the bounds of tests/quote_precise_ref.py on every row of the 60-digit fixture, at the K the numpy
restatement of the forms measured; relations the forms must keep; and the same shim once as a stand-alone program under
the address and undefined-behaviour sanitizers.  The device paths are held to the same K in tests/test_gpu_quote_precise.py.

K table (python tests/quote_precise_ref.py; K = next power of two >= 2x the restatement's worst ratio, cap 16 / 64):
    family     class: worst -> K
    product    tiny 1e-12 -> 1, typical 0.019 -> 1, huge 0 -> 1, lopsided 0.086 -> 1, low_gamma 0.18 -> 1
    geomean    tiny 2e-12 -> 1, typical 0.16 -> 1, huge 0 -> 1, lopsided 0.026 -> 1, low_gamma 0.18 -> 1, w02_98 0.042 -> 1
    weighted   tiny 4e-11 -> 1, typical 0.17 -> 1, huge 0 -> 1, lopsided 0.27 -> 1, low_gamma 0.17 -> 1, pairs 0.13 -> 1, w02_98 0.044 -> 1
    solidly    tiny 3.1 -> 8, typical 1.7 -> 4, huge 0 -> 1, lopsided 1.9 -> 4, low_gamma 1.1 -> 4, balanced 1.5 -> 4, t0_hi 1.2 -> 4, t0_lo 1.8 -> 4
    curve      tiny 3e-11 -> 1, typical 0.42 -> 1, huge 0.64 -> 2, lopsided 1.3 -> 4, low_gamma 0.60 -> 2, stiff 0.39 -> 1, small_a 0.13 -> 1, alpha0 0.13 -> 1
    univ3      in_tick 0.73 -> 2, boundary_dn 0.51 -> 2, boundary_up 0.18 -> 1, depth1 0.19 -> 1, depth4 0.20 -> 1, depth5 0.16 -> 1,
               depth64 0.033 -> 1, empty_in_path 0.20 -> 1, empty_current 0.18 -> 1, last_tick 0 -> 1, exhausted 0.49 -> 1
(Solidly with ONE Newton step after Cardano measured 77 on `lopsided`, above the cap: the finding that made it two.)
The oracle's own tick-by-tick walk against the same truth, in the same units: 0.73 (quote_precise_ref.ORACLE_UNIV3_WORST)."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import quote_precise_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "quote_host.cpp")
KIND = {"product": 0, "geomean": 1, "weighted": 3, "curve": 4, "solidly": 5}


@pytest.fixture(scope="module")
def fx():
    assert os.path.getsize(P.FIXTURE) <= 1 << 20
    return P.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """quote_pool.h built for the host with the Makefile's host flags, loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("quote_host") / "quote_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.quote_host_pools.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp, dp, ip, ip, dp, dp]
    lib.quote_host_univ3.argtypes = [ctypes.c_int64, dp, dp, lp, dp, dp, ctypes.c_int64, lp, ip, dp, dp]
    return lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def host_pools(lib, fam, R, gamma, cin, cout, a, w=None, alpha=None, beta=None):
    f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    R, gamma, a, w, alpha, beta = f(R), f(gamma), f(a), f(w), f(alpha), f(beta)
    cin, cout = np.ascontiguousarray(cin, dtype=np.int32), np.ascontiguousarray(cout, dtype=np.int32)
    out = np.empty(a.size)
    D = ctypes.c_double
    rc = lib.quote_host_pools(KIND[fam], R.shape[1], a.size, _p(R, D), _p(w, D), _p(alpha, D), _p(beta, D), _p(gamma, D),
                              _p(cin, ctypes.c_int32), _p(cout, ctypes.c_int32), _p(a, D), _p(out, D))
    assert rc == 0
    return out


def host_univ3(lib, g, pool=None, cin=None, a=None, liquidity=None):
    f = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    cp, gm, lt = f(g["current_price"]), f(g["pool_gamma"]), f(g["lower_ticks"])
    lq = f(g["liquidity"] if liquidity is None else liquidity)
    off = np.ascontiguousarray(g["tick_off"], dtype=np.int64)
    pool = np.ascontiguousarray(g["pool"] if pool is None else pool, dtype=np.int64)
    cin = np.ascontiguousarray(g["cin"] if cin is None else cin, dtype=np.int32)
    a = f(g["a"] if a is None else a)
    out = np.empty(a.size)
    D = ctypes.c_double
    rc = lib.quote_host_univ3(cp.size, _p(cp, D), _p(gm, D), _p(off, ctypes.c_int64), _p(lt, D), _p(lq, D), a.size,
                              _p(pool, ctypes.c_int64), _p(cin, ctypes.c_int32), _p(a, D), _p(out, D))
    assert rc == 0
    return out


def host_group(lib, fx, gname):
    g = P.group(fx, gname)
    if gname == "univ3":
        return host_univ3(lib, g), g
    return host_pools(lib, P.family(gname), g["R"], g["gamma"], g["cin"], g["cout"], g["a"], g.get("w"), g.get("alpha"),
                      g.get("beta")), g


def assert_within(out, g, gname, label):
    r = P.ratios(out, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K = P.K_of(gname, str(c))
        worst = float(np.max(r[sel]))
        print(f"{label} {gname}/{c}: worst {worst:.3g} of K = {K}")
        assert np.all(np.isfinite(out[sel])) and worst <= K, (gname, c, worst, K)


def test_K_table_is_what_the_restatement_measures(fx):
    """K_MEASURED records the numpy restatement's worst ratios (to its three printed digits), and no class needs more than
    the cap"""
    w = P.worst_by_class(fx)
    assert set(w) == set(P.K_MEASURED)
    for key, worst in w.items():
        assert worst <= P.K_MEASURED[key] * 1.01 + 1e-300, (key, worst)
    for gname in P.GROUPS:
        for c in np.unique(P.group(fx, gname)["cls"]):
            P.K_of(gname, str(c))


@pytest.mark.parametrize("gname", P.GROUPS)
def test_host_build_within_the_bounds(fx, host, gname):
    out, g = host_group(host, fx, gname)
    assert_within(out, g, gname, "host")


def test_fixture_covers_the_classes(fx):
    need = {"product": {"tiny", "typical", "huge", "lopsided", "low_gamma"},
            "solidly": {"tiny", "typical", "huge", "lopsided", "low_gamma", "balanced", "t0_hi", "t0_lo"},
            "curve3": {"tiny", "typical", "huge", "lopsided", "low_gamma", "stiff", "small_a", "alpha0"},
            "weighted3": {"tiny", "typical", "huge", "lopsided", "low_gamma", "pairs", "w02_98"},
            "weighted2": {"w02_98"}, "weighted8": {"typical", "w02_98"},
            "univ3": {"in_tick", "boundary_dn", "boundary_up", "depth1", "depth4", "depth5", "depth64", "empty_in_path",
                      "empty_current", "last_tick", "exhausted"}}
    for gname, classes in need.items():
        assert classes <= set(P.group(fx, gname)["cls"]), gname
    g = P.group(fx, "weighted3")
    pairs = {(int(i), int(o)) for i, o, c in zip(g["cin"], g["cout"], g["cls"]) if c == "pairs"}
    assert pairs == {(i, o) for i in range(3) for o in range(3) if i != o}


def test_curve_at_alpha_zero_is_the_product_quote(fx, host):
    """α = 0: the Curve form reduces to Product's, within the same bound (the fixture's alpha0 rows against THEIR truth, and
    against the Product function on the same reserves)"""
    for gname in P.CURVE:
        g = P.group(fx, gname)
        sel = g["cls"] == "alpha0"
        rows = np.arange(sel.sum())
        R2 = np.stack([g["R"][sel][rows, g["cin"][sel]], g["R"][sel][rows, g["cout"][sel]]], axis=1)
        prod = host_pools(host, "product", R2, g["gamma"][sel], np.zeros(rows.size), np.ones(rows.size), g["a"][sel])
        gs = {k: v[sel] for k, v in g.items() if isinstance(v, np.ndarray) and v.shape[:1] == sel.shape}
        assert np.max(P.ratios(prod, gs)) <= P.K_of(gname, "alpha0")


def test_zero_amount_is_plus_zero_bit_for_bit(fx, host):
    for gname in P.GROUPS:
        g = P.group(fx, gname)
        zero = np.zeros(g["a"].size)
        if gname == "univ3":
            out = host_univ3(host, g, a=zero)
        else:
            out = host_pools(host, P.family(gname), g["R"], g["gamma"], g["cin"], g["cout"], zero, g.get("w"), g.get("alpha"),
                             g.get("beta"))
        assert np.all(out.view(np.uint64) == 0), gname


@pytest.mark.parametrize("k", [-40, -3, 7, 60])
def test_scaling_by_a_power_of_two_is_exact(fx, host, k):
    """Product, Solidly: R and a by 2^k scales out by 2^k exactly.  UniV3: liquidity (k of x·y = k) by 4^k and a by 2^k."""
    s = 2.0 ** k
    for gname in ("product", "solidly"):
        g = P.group(fx, gname)
        base = host_pools(host, gname, g["R"], g["gamma"], g["cin"], g["cout"], g["a"])
        scaled = host_pools(host, gname, g["R"] * s, g["gamma"], g["cin"], g["cout"], g["a"] * s)
        np.testing.assert_array_equal(scaled, base * s)
    g = P.group(fx, "univ3")
    base = host_univ3(host, g)
    scaled = host_univ3(host, g, a=g["a"] * s, liquidity=g["liquidity"] * s * s)
    np.testing.assert_array_equal(scaled, base * s)


def test_swapping_the_coins_swaps_nothing_else(fx, host):
    """the pool with its coins (and weights) listed the other way round, queried at the swapped positions: same bits"""
    for gname in ("product", "solidly", "geomean", "curve2", "weighted2"):
        g = P.group(fx, gname)
        fam = P.family(gname)
        w = None if "w" not in g else g["w"][:, ::-1]
        a = host_pools(host, fam, g["R"], g["gamma"], g["cin"], g["cout"], g["a"], g.get("w"), g.get("alpha"), g.get("beta"))
        b = host_pools(host, fam, g["R"][:, ::-1], g["gamma"], 1 - g["cin"], 1 - g["cout"], g["a"], w, g.get("alpha"), g.get("beta"))
        np.testing.assert_array_equal(a, b)


def test_oracle_walk_against_the_truth(fx):
    """oracle.UniV3.forward_trade (the reference's sequential walk in doubles) against the 60-digit truth, in the units of
    the bound: the figure the GPU test adds to the device's K when it compares the two"""
    import oracle.cfmm_oracle as O
    g = P.group(fx, "univ3")
    out = np.empty(g["a"].size)
    for j, (p, ci, a) in enumerate(zip(g["pool"], g["cin"], g["a"])):
        cp, lt, lq, gamma = P.univ3_pool(g, int(p))
        D = np.zeros(2)
        D[ci] = a
        out[j] = O.UniV3(cp, lt, lq, gamma).forward_trade(D)
    worst = float(np.max(P.ratios(out, g)))
    print(f"oracle walk: worst {worst:.3g} units (recorded {P.ORACLE_UNIV3_WORST}, allowance K = {P.ORACLE_UNIV3_K})")
    assert worst <= P.ORACLE_UNIV3_WORST * 1.01 and P.ORACLE_UNIV3_K == P.next_pow2(2 * P.ORACLE_UNIV3_WORST)


def test_univ3_unit_in_doubles_is_the_fixtures(fx):
    """quote_precise_ref.univ3_unit (the per-row unit from the walk actually taken, in doubles: what the GPU comparison with the
    oracle's walk measures in) against the scale and conditioning the fixture stores from mpmath.  The boundary rows are left
    out: a rounding decides there which tick is the landing one, and the two choices have different (both valid) units."""
    g = P.group(fx, "univ3")
    preps = [P.univ3_prepare(*P.univ3_pool(g, p)[:3]) for p in range(g["current_price"].size)]
    for j, (p, ci, a, c) in enumerate(zip(g["pool"], g["cin"], g["a"], g["cls"])):
        if c.startswith("boundary"):
            continue
        scale, cond = P.univ3_unit(preps[p], float(g["pool_gamma"][p]), int(ci), float(a))
        assert abs(scale - g["scale"][j]) <= 1e-9 * g["scale"][j] and abs(cond - g["cond"][j]) <= 1e-9 * g["cond"][j], (j, c)


def write_blocks(path, fx):
    """the fixture's queries as tests/native/quote_host.cpp's main reads them"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).tobytes()
    with open(path, "wb") as f:
        for gname in P.GROUPS:
            g = P.group(fx, gname)
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


def test_stand_alone_program_under_the_sanitizers(fx, host, tmp_path):
    """The same shim with its own main, built with -fsanitize=address,undefined, run as a program on the fixture: clean, and
    within the bounds (the -O1 sanitized build need not round like the -O3 one bit for bit where libm is inlined differently,
    so it is held to the bounds, not to the other build's bits)."""
    exe, inp, outp = str(tmp_path / "quote_host"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DQUOTE_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SHIM,
                    "-o", exe], check=True)
    write_blocks(inp, fx)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "QUOTE_HOST_OK" in r.stdout and r.stderr == ""
    out = np.fromfile(outp, dtype=np.float64)
    at = 0
    for gname in P.GROUPS:
        g = P.group(fx, gname)
        n = g["a"].size
        assert_within(out[at:at + n], g, gname, "sanitized")
        at += n
    assert at == out.size
