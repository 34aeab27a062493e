"""Exact-output swap quotes on the CPU: the quote_out_* forms of csrc/quote_pool.h built for the host
(tests/native/quote_out_host.cpp, the functions quote_out_kernel runs) held to the bounds of tests/quote_out_precise_ref.py
on every row of the 80-digit fixture, at the K the numpy restatement of the forms measured; relations the forms must keep;
and the same shim once as a stand-alone program under the address and undefined-behaviour sanitizers.  The device paths are
held to the same K in tests/test_gpu_quote_out_precise.py.

K table (python tests/quote_out_precise_ref.py; K = next power of two >= 2x the restatement's worst ratio, cap 16 / 64):
    family     class: worst -> K
    product    tiny 2e-12 -> 1, typical 0.14 -> 1, huge 0 -> 1, lopsided 0.18 -> 1, low_gamma 0.039 -> 1, near_drain 0 -> 1
    geomean    tiny 1e-12 -> 1, typical 0.14 -> 1, huge 0.089 -> 1, lopsided 0.043 -> 1, low_gamma 0.12 -> 1, w02_98 0.26 -> 1,
               near_drain 0.22 -> 1
    weighted   tiny 2e-12 -> 1, typical 0.15 -> 1, huge 0.20 -> 1, lopsided 0.13 -> 1, low_gamma 0.32 -> 1, pairs 0.086 -> 1,
               w02_98 0.29 -> 1, near_drain 0.25 -> 1
    solidly    tiny 3e-12 -> 1, typical 0.27 -> 1, huge 0 -> 1, lopsided 0.0072 -> 1, low_gamma 0.39 -> 1, balanced 0.15 -> 1,
               t0_hi 0.049 -> 1, t0_lo 0.12 -> 1, near_drain 0.19 -> 1
    curve      tiny 2e-11 -> 1, typical 0.58 -> 2, huge 3e-10 -> 1, lopsided 0.14 -> 1, low_gamma 0.60 -> 2, stiff 0.38 -> 1,
               small_a 0.076 -> 1, alpha0 0.13 -> 1, near_drain 0.20 -> 1, o_gt_Ri 0.70 -> 2
    univ3      in_tick 0.014 -> 1, boundary_dn 0.25 -> 1, boundary_up 0.25 -> 1, depth1 0.15 -> 1, depth4 0.069 -> 1,
               depth5 0.097 -> 1, depth64 0.025 -> 1, empty_in_path 0.069 -> 1, empty_current 0.058 -> 1, last_tick 0.23 -> 1,
               exhausted 0.23 -> 1, on_boundary 0.68 -> 2, closing_exact 0.23 -> 1, beyond / asymptotic: +inf, compared for equality
(Solidly as first written, a = (u·y′ − R_i)/γ straight from the cubic's root, measured 5.5 on `typical` and `t0_hi` with numpy's
libm -- K = 16, AT the cap -- and the host build 3.1 on `balanced` where numpy's gave 0.79: noise of a difference of two
numbers of the size of R_i, which depends on the library.  Two Newton steps on the cubic in x itself took it to 0.27.)"""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import quote_out_precise_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "quote_out_host.cpp")
KIND = {"product": 0, "geomean": 1, "weighted": 3, "curve": 4, "solidly": 5}


@pytest.fixture(scope="module")
def fx():
    assert os.path.getsize(P.FIXTURE) <= 1 << 20
    return P.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """quote_pool.h built for the host with the Makefile's host flags, loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("quote_out_host") / "quote_out_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.quote_out_host_pools.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp, dp, ip, ip, dp, dp]
    lib.quote_out_host_univ3.argtypes = [ctypes.c_int64, dp, dp, lp, dp, dp, ctypes.c_int64, lp, ip, dp, dp]
    return lib


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def host_pools(lib, fam, R, gamma, cin, cout, a, w=None, alpha=None, beta=None):
    f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    R, gamma, a, w, alpha, beta = f(R), f(gamma), f(a), f(w), f(alpha), f(beta)
    cin, cout = np.ascontiguousarray(cin, dtype=np.int32), np.ascontiguousarray(cout, dtype=np.int32)
    out = np.empty(a.size)
    D = ctypes.c_double
    rc = lib.quote_out_host_pools(KIND[fam], R.shape[1], a.size, _p(R, D), _p(w, D), _p(alpha, D), _p(beta, D), _p(gamma, D),
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
    a = f(g["o"] if a is None else a)
    out = np.empty(a.size)
    D = ctypes.c_double
    rc = lib.quote_out_host_univ3(cp.size, _p(cp, D), _p(gm, D), _p(off, ctypes.c_int64), _p(lt, D), _p(lq, D), a.size,
                              _p(pool, ctypes.c_int64), _p(cin, ctypes.c_int32), _p(a, D), _p(out, D))
    assert rc == 0
    return out


def host_group(lib, fx, gname):
    g = P.group(fx, gname)
    if gname == "univ3":
        return host_univ3(lib, g), g
    return host_pools(lib, P.family(gname), g["R"], g["gamma"], g["cin"], g["cout"], g["o"], g.get("w"), g.get("alpha"),
                      g.get("beta")), g


def assert_within(out, g, gname, label):
    r = P.ratios(out, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K = P.K_of(gname, str(c))
        worst = float(np.max(r[sel]))
        print(f"{label} {gname}/{c}: worst {worst:.3g} of K = {K}")
        assert not np.any(np.isnan(out[sel])) and worst <= K, (gname, c, worst, K)      # (+inf rows: equal or the ratio is inf)


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
    """every row and class of the exact-input fixture carries over (same state, coins and class, o = its stored out), the
    inverse's own classes are there, and the +inf rows are few enough not to hollow out the accuracy classes"""
    import quote_precise_ref as F
    need = {"product": {"tiny", "typical", "huge", "lopsided", "low_gamma", "near_drain"},
            "solidly": {"tiny", "typical", "huge", "lopsided", "low_gamma", "balanced", "t0_hi", "t0_lo", "near_drain"},
            "geomean": {"near_drain"},
            "curve3": {"tiny", "typical", "huge", "lopsided", "low_gamma", "stiff", "small_a", "alpha0", "near_drain", "o_gt_Ri"},
            "curve2": {"o_gt_Ri"}, "curve4": {"o_gt_Ri"},
            "weighted3": {"tiny", "typical", "huge", "lopsided", "low_gamma", "pairs", "w02_98", "near_drain"},
            "weighted2": {"w02_98"}, "weighted8": {"typical", "w02_98"},
            "univ3": {"in_tick", "boundary_dn", "boundary_up", "depth1", "depth4", "depth5", "depth64", "empty_in_path",
                      "empty_current", "last_tick", "exhausted", "on_boundary", "closing_exact", "beyond", "asymptotic"}}
    for gname, classes in need.items():
        assert classes <= set(P.group(fx, gname)["cls"]), gname
    src = F.load()
    rows = infinite = 0
    for gname in P.GROUPS:
        g, f = P.group(fx, gname), F.group(src, gname)
        n = f["a"].size
        assert n >= 20 and list(g["cls"][:n]) == list(f["cls"]) and np.array_equal(g["cin"][:n], f["cin"])
        keep = g["cls"][:n] != "exhausted"          # (those take the device's own total: the ref module's docstring)
        np.testing.assert_array_equal(g["o"][:n][keep], f["out"][keep])
        if gname != "univ3":
            np.testing.assert_array_equal(g["R"][:n], f["R"])
        rows += g["o"].size
        infinite += int(np.sum(np.isinf(g["a"])))
    assert rows >= 380 + 60 and 0 < infinite <= P.MAX_INF_SHARE * rows, (rows, infinite)
    g = P.group(fx, "product")
    sel = g["cls"] == "near_drain"
    ro = g["R"][np.arange(sel.size), g["cout"]][sel]
    assert np.min(1.0 - g["o"][sel] / ro) <= 2.0 ** -40
    for gname in P.CURVE:   # o_gt_Ri is the E' < 0 branch
        g = P.group(fx, gname)
        sel = g["cls"] == "o_gt_Ri"
        rows_ = np.arange(sel.size)
        P0 = g["beta"] / np.prod(g["R"], axis=1)
        assert np.all((g["alpha"] * (g["R"][rows_, g["cin"]] - g["o"]) + P0)[sel] < 0)
    g = P.group(fx, "weighted3")
    pairs = {(int(i), int(o)) for i, o, c in zip(g["cin"], g["cout"], g["cls"]) if c == "pairs"}
    assert pairs == {(i, o) for i in range(3) for o in range(3) if i != o}


def test_curve_at_alpha_zero_is_the_product_quote(fx, host):
    """α = 0: the Curve form reduces to Product's, R_i·o/((R_o − o)·γ), within the same bound (the fixture's alpha0 rows against
    THEIR truth, and against the Product function on the same reserves)"""
    for gname in P.CURVE:
        g = P.group(fx, gname)
        sel = g["cls"] == "alpha0"
        rows = np.arange(sel.sum())
        R2 = np.stack([g["R"][sel][rows, g["cin"][sel]], g["R"][sel][rows, g["cout"][sel]]], axis=1)
        prod = host_pools(host, "product", R2, g["gamma"][sel], np.zeros(rows.size), np.ones(rows.size), g["o"][sel])
        gs = {k: v[sel] for k, v in g.items() if isinstance(v, np.ndarray) and v.shape[:1] == sel.shape}
        assert np.max(P.ratios(prod, gs)) <= P.K_of(gname, "alpha0")


def test_zero_amount_is_plus_zero_bit_for_bit(fx, host):
    for gname in P.GROUPS:
        g = P.group(fx, gname)
        zero = np.zeros(g["o"].size)
        if gname == "univ3":
            out = host_univ3(host, g, a=zero)
        else:
            out = host_pools(host, P.family(gname), g["R"], g["gamma"], g["cin"], g["cout"], zero, g.get("w"), g.get("alpha"),
                             g.get("beta"))
        assert np.all(out.view(np.uint64) == 0), gname


@pytest.mark.parametrize("k", [-40, -3, 7, 60])
def test_scaling_by_a_power_of_two_is_exact(fx, host, k):
    """Product, Solidly: R and o by 2^k scales a by 2^k exactly.  UniV3: liquidity (k of x·y = k) by 4^k and o by 2^k."""
    s = 2.0 ** k
    for gname in ("product", "solidly"):
        g = P.group(fx, gname)
        base = host_pools(host, gname, g["R"], g["gamma"], g["cin"], g["cout"], g["o"])
        scaled = host_pools(host, gname, g["R"] * s, g["gamma"], g["cin"], g["cout"], g["o"] * s)
        np.testing.assert_array_equal(scaled, base * s)
    g = P.group(fx, "univ3")
    base = host_univ3(host, g)
    scaled = host_univ3(host, g, a=g["o"] * s, liquidity=g["liquidity"] * s * s)
    np.testing.assert_array_equal(scaled, base * s)


def test_swapping_the_coins_swaps_nothing_else(fx, host):
    """the pool with its coins (and weights) listed the other way round, queried at the swapped positions: same bits"""
    for gname in ("product", "solidly", "geomean", "curve2", "weighted2"):
        g = P.group(fx, gname)
        fam = P.family(gname)
        w = None if "w" not in g else g["w"][:, ::-1]
        a = host_pools(host, fam, g["R"], g["gamma"], g["cin"], g["cout"], g["o"], g.get("w"), g.get("alpha"), g.get("beta"))
        b = host_pools(host, fam, g["R"][:, ::-1], g["gamma"], 1 - g["cin"], 1 - g["cout"], g["o"], w, g.get("alpha"), g.get("beta"))
        np.testing.assert_array_equal(a, b)


def test_inf_rows_are_inf_and_nothing_else_is(fx, host):
    """no finite input yields o: +inf exactly; every other row is finite.  Also o == R_o and o just above it on every reserve
    kind, and a NaN amount propagates"""
    for gname in P.GROUPS:
        out, g = host_group(host, fx, gname)
        np.testing.assert_array_equal(np.isinf(out) & (out > 0), np.isinf(g["a"]), err_msg=gname)
        assert not np.any(np.isnan(out))
        if gname == "univ3":
            assert np.all(np.isnan(host_univ3(host, g, a=np.full(g["o"].size, np.nan))))
            continue
        ro = g["R"][np.arange(g["o"].size), g["cout"]]
        for o in (ro, np.nextafter(ro, np.inf), 2.0 * ro, np.full(ro.size, np.nan)):
            a = host_pools(host, P.family(gname), g["R"], g["gamma"], g["cin"], g["cout"], o, g.get("w"), g.get("alpha"), g.get("beta"))
            assert np.all(np.isnan(a)) if np.isnan(o[0]) else np.all(a == np.inf), gname


def test_univ3_unit_in_doubles_is_the_fixtures(fx):
    """quote_out_precise_ref.univ3_unit (the per-row unit from the inverse walk actually taken, in doubles: what the GPU
    comparison with the restatement measures in) against the scale and conditioning the fixture stores from mpmath.  Rows AT a
    record's sum are left out: a rounding decides there which tick is the landing one, and the two choices have different
    (both valid) units."""
    import quote_precise_ref as F
    g = P.group(fx, "univ3")
    preps = [F.univ3_prepare(*F.univ3_pool(g, p)[:3]) for p in range(g["current_price"].size)]
    seen = 0
    for j, (p, ci, o, c) in enumerate(zip(g["pool"], g["cin"], g["o"], g["cls"])):
        if c.startswith("boundary") or c in ("on_boundary", "closing_exact", "exhausted") or not np.isfinite(g["a"][j]):
            continue
        scale, cond, _ = P.univ3_unit(preps[p], float(g["pool_gamma"][p]), int(ci), float(o))
        assert abs(scale - g["scale"][j]) <= 1e-9 * g["scale"][j] and abs(cond - g["cond"][j]) <= 1e-6 * g["cond"][j], (j, c)
        seen += 1
    assert seen >= 40


def write_blocks(path, fx):
    """the fixture's queries as tests/native/quote_out_host.cpp's main reads them"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).tobytes()
    with open(path, "wb") as f:
        for gname in P.GROUPS:
            g = P.group(fx, gname)
            if gname == "univ3":
                f.write(struct.pack("<4q", 2, g["current_price"].size, g["o"].size, g["lower_ticks"].size))
                f.write(f64(g["current_price"]) + f64(g["pool_gamma"]) + i64(g["tick_off"]) + f64(g["lower_ticks"]) +
                        f64(g["liquidity"]) + i64(g["pool"]) + i64(g["cin"]) + f64(g["o"]))
                continue
            kind = KIND[P.family(gname)]
            f.write(struct.pack("<4q", 1, kind, g["R"].shape[1], g["o"].size))
            f.write(f64(g["R"]))
            if kind in (1, 3):
                f.write(f64(g["w"]))
            if kind == 4:
                f.write(f64(g["alpha"]) + f64(g["beta"]))
            f.write(f64(g["gamma"]) + i64(g["cin"]) + i64(g["cout"]) + f64(g["o"]))


def test_stand_alone_program_under_the_sanitizers(fx, host, tmp_path):
    """The same shim with its own main, built with -fsanitize=address,undefined, run as a program on the fixture: clean,
    within the bounds, and bit-equal to the same program built without the sanitizers (same optimisation level: where libm
    calls are folded differently at another level the last bit may differ, which the bounds, not this comparison, judge)."""
    inp = str(tmp_path / "in.bin")
    write_blocks(inp, fx)
    outs = {}
    for name, flags in (("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ("plain", [])):
        exe, outp = str(tmp_path / f"quote_out_host_{name}"), str(tmp_path / f"out_{name}.bin")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off"] + flags +
                       ["-DQUOTE_OUT_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SHIM, "-o", exe], check=True)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        print(name, r.stdout, r.stderr[-2000:])
        assert r.returncode == 0 and "QUOTE_OUT_HOST_OK" in r.stdout and r.stderr == ""
        outs[name] = np.fromfile(outp, dtype=np.float64)
    out = outs["sanitized"]
    np.testing.assert_array_equal(out.view(np.uint64), outs["plain"].view(np.uint64))
    at = 0
    for gname in P.GROUPS:
        g = P.group(fx, gname)
        n = g["o"].size
        assert_within(out[at:at + n], g, gname, "sanitized")
        at += n
    assert at == out.size
