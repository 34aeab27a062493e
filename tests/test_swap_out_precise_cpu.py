"""cfmm_swap_out's per-kind forms on the CPU: csrc/swap_pool.h + quote_pool.h + univ3_pool.h built for the host
(tests/native/swap_out_host.cpp: the functions swap_out_kernel runs, applied in query order as the kernel and the host apply
them) held to the 80-digit sequences of tests/golden/swap_out_precise.npz within tests/swap_out_precise_ref.py's bounds; the
exact properties that need no tolerance; the status logic and the backward walk of a path as a numpy restatement; and the
same shim, with the HIP-free checks of the path entry, once as a stand-alone program under the address and
undefined-behaviour sanitizers.  The device is held to the same K in tests/test_gpu_swap_out_precise.py.

K table (swap_out_precise_ref.K_MEASURED, re-measured here): worst ratio of the host build -> K = next power of two >= 2x it:
    product    balanced 0.35, lopsided 0.18, low_gamma 0.45 -> 1, typical 0.62 -> 2
    geomean    balanced 0.26, typical 0.18, lopsided 0.23, low_gamma 0.29 -> 1
    weighted   typical 0.36, lopsided 0.42, low_gamma 0.13 -> 1, balanced 0.55 -> 2
    solidly    balanced 0.30, lopsided 0.38, low_gamma 0.022 -> 1, typical 0.74 -> 2
    curve      typical 0.27, low_gamma 0.47 -> 1, balanced 0.78, lopsided 0.60 -> 2
    univ3      one_tick 0.033, two_ticks 0.0035, tick_edge 0.0032, boundary 0.060, crosses 0.013, empty_tick 0.016,
               exhausted 0.092, reversal 0.12 -> 1"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quote_out_precise_ref as QO
import quote_precise_ref as Q
import swap_out_precise_ref as S
from test_quote_out_precise_cpu import host as quote_out_host  # noqa: F401  (the quote shim: `in` equals quote_out_* of the same state)
from test_quote_out_precise_cpu import host_pools, host_univ3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "swap_out_host.cpp")
D, I32, I64 = ctypes.c_double, ctypes.c_int32, ctypes.c_int64
APPLIED, OVER_LIMIT, REFUSED, UNOBTAINABLE = 0, 1, 2, 3               # CFMM_SWAP_*


def build_host(so):
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    dp, ip, lp = ctypes.POINTER(D), ctypes.POINTER(I32), ctypes.POINTER(I64)
    lib.swap_out_host_pool.argtypes = [ctypes.c_int, ctypes.c_int, dp, dp, D, D, D, ctypes.c_int, ip, ip, dp, dp, dp, ip, dp, dp]
    lib.swap_out_host_univ3.argtypes = [D, D, I64, dp, dp, ctypes.c_int, ip, dp, dp, dp, ip, dp]
    lib.swap_out_host_check.argtypes = [I64, ip, ip, lp, dp, ctypes.c_char_p, I64]
    return lib


@pytest.fixture(scope="module")
def fx():
    assert os.path.getsize(S.FIXTURE) <= 1 << 20
    return S.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("swap_out_host") / "swap_out_host.so"))


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def swap_out_pool(lib, fam, R, gamma, cin, cout, want, w=None, alpha=0.0, beta=1.0, max_in=None):
    """-> (amount_in [steps], status [steps], R after every step [steps, n], refreshed constants [steps, 2])"""
    R = np.array(R, dtype=np.float64)
    n, steps = R.size, len(want)
    w = np.ones(n) if w is None else np.ascontiguousarray(w, dtype=np.float64)
    cin, cout = np.ascontiguousarray(cin, dtype=np.int32), np.ascontiguousarray(cout, dtype=np.int32)
    want = np.ascontiguousarray(want, dtype=np.float64)
    lim = None if max_in is None else np.ascontiguousarray(max_in, dtype=np.float64)
    a, st, Rs, konst = np.empty(steps), np.empty(steps, dtype=np.int32), np.empty((steps, n)), np.empty((steps, 2))
    rc = lib.swap_out_host_pool(S.KIND[fam], n, _p(R, D), _p(w, D), float(alpha), float(beta), float(gamma), steps, _p(cin, I32),
                                _p(cout, I32), _p(want, D), _p(lim, D), _p(a, D), _p(st, I32), _p(Rs, D), _p(konst, D))
    assert rc == 0
    return a, st, Rs, konst


def swap_out_univ3(lib, cp, gamma, lt, lq, cin, want, max_in=None):
    lt, lq = np.ascontiguousarray(lt, dtype=np.float64), np.ascontiguousarray(lq, dtype=np.float64)
    cin, want = np.ascontiguousarray(cin, dtype=np.int32), np.ascontiguousarray(want, dtype=np.float64)
    lim = None if max_in is None else np.ascontiguousarray(max_in, dtype=np.float64)
    a, st, price = np.empty(want.size), np.empty(want.size, dtype=np.int32), np.empty(want.size)
    rc = lib.swap_out_host_univ3(float(cp), float(gamma), lt.size, _p(lt, D), _p(lq, D), want.size, _p(cin, I32), _p(want, D), _p(lim, D),
                                 _p(a, D), _p(st, I32), _p(price, D))
    assert rc == 0
    return a, st, price


def pool_args(g, s, fam):
    n = int(g["nsteps"][s])
    return (fam, g["R0"][s], g["gamma"][s], g["cin"][s, :n], g["cout"][s, :n], g["want"][s, :n], g["w"][s], g["alpha"][s], g["beta"][s])


def univ3_args(g, s):
    n = int(g["nsteps"][s])
    o, e = g["tick_off"][s], g["tick_off"][s + 1]
    return (g["cp"][s], g["gamma"][s], g["lower_ticks"][o:e], g["liquidity"][o:e], g["cin"][s, :n], g["want"][s, :n])


def run_host(lib):
    def run(name, g, s):
        if name == "univ3":
            a, st, price = swap_out_univ3(lib, *univ3_args(g, s))
            assert np.all(st == APPLIED)
            return a, price[-1]
        a, st, Rs, _ = swap_out_pool(lib, *pool_args(g, s, Q.family(name)))
        assert np.all(st == APPLIED)
        return a, Rs[-1]
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
    assert {"one_tick", "two_ticks", "tick_edge", "boundary", "crosses", "empty_tick", "exhausted", "reversal"} <= set(g["cls"])
    assert {1, 2, 5} <= set(np.diff(g["tick_off"]))
    s = list(g["cls"]).index("tick_edge")
    assert g["want"][s, 0] == 6.0 and g["a"][s, 0] == 4.0 and g["price"][s, 0] == 1.0   # the whole first tick: ends exactly on its edge
    for s in np.flatnonzero(g["cls"] == "boundary"):                     # want IS a running ΣR_out of the prepared records
        o, e = g["tick_off"][s], g["tick_off"][s + 1]
        prep = Q.univ3_prepare(float(g["cp"][s]), g["lower_ticks"][o:e], g["liquidity"][o:e])
        sums = [r[6] for r in (prep[1] if g["cin"][s, 0] == 0 else prep[2])[:-1]]
        assert g["want"][s, 0] in sums, s
    for s in np.flatnonzero(g["cls"] == "exhausted"):                    # ... or the closing record's, where a finite input exhausts
        o, e = g["tick_off"][s], g["tick_off"][s + 1]
        prep = Q.univ3_prepare(float(g["cp"][s]), g["lower_ticks"][o:e], g["liquidity"][o:e])
        sd, sr = QO.univ3_totals(prep, int(g["cin"][s, 0]))
        assert g["want"][s, 0] == sr and np.isfinite(sd) and g["price"][s, 0] == g["lower_ticks"][o]


# ---- exact properties ---------------------------------------------------------------------------------------------------------
def test_in_equals_quote_out_of_the_same_state(fx, host, quote_out_host):
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            a, st, Rs, _ = swap_out_pool(host, *pool_args(g, s, fam))
            before = np.vstack([g["R0"][s][None, :], Rs[:-1]])
            rep = lambda x: np.repeat(np.atleast_1d(x), n)
            kw = {}
            if fam in ("geomean", "weighted"):
                kw["w"] = np.tile(g["w"][s], (n, 1))
            if fam == "curve":
                kw.update(alpha=rep(g["alpha"][s]), beta=rep(g["beta"][s]))
            q = host_pools(quote_out_host, fam, before, rep(g["gamma"][s]), g["cin"][s, :n], g["cout"][s, :n], g["want"][s, :n], **kw)
            np.testing.assert_array_equal(a.view(np.uint64), q.view(np.uint64), err_msg=f"{name} {s}")
    g = S.group(fx, "univ3")
    for s in range(len(g["cls"])):
        n = int(g["nsteps"][s])
        o, e = g["tick_off"][s], g["tick_off"][s + 1]
        a, st, price = swap_out_univ3(host, *univ3_args(g, s))
        cps = np.concatenate([[g["cp"][s]], price[:-1]])
        for j in range(n):
            gg = {"current_price": cps[j:j + 1], "pool_gamma": g["gamma"][s:s + 1], "lower_ticks": g["lower_ticks"][o:e],
                  "liquidity": g["liquidity"][o:e], "tick_off": np.array([0, e - o]), "pool": np.zeros(1, dtype=np.int64),
                  "cin": g["cin"][s, j:j + 1], "o": g["want"][s, j:j + 1]}
            q = host_univ3(quote_out_host, gg)
            assert q.view(np.uint64)[0] == a.view(np.uint64)[j], (s, j)


def test_new_reserves_are_R_plus_gamma_in_and_R_minus_want(fx, host):
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            a, st, Rs, _ = swap_out_pool(host, *pool_args(g, s, fam))
            R = np.array(g["R0"][s], copy=True)
            for j in range(n):
                ci, co = g["cin"][s, j], g["cout"][s, j]
                R[ci] = R[ci] + g["gamma"][s] * a[j]                     # each operation rounded on its own
                R[co] = R[co] - g["want"][s, j]                          # the amount asked for
                np.testing.assert_array_equal(Rs[j].view(np.uint64), R.view(np.uint64), err_msg=f"{name} {s} step {j}")


def test_univ3_rests_where_the_swap_of_the_answer_rests(fx, host, tmp_path_factory):
    """the state equals the exact-input shim's (tests/native/swap_host.cpp) after swap(amount_in), bit for bit"""
    from test_swap_precise_cpu import SHIM as SWAP_SHIM
    so = str(tmp_path_factory.mktemp("swap_host") / "swap_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-mavx2", "-shared", "-fPIC", SWAP_SHIM, "-o", so], check=True)
    fwd = ctypes.CDLL(so)
    dp, ip = ctypes.POINTER(D), ctypes.POINTER(I32)
    fwd.swap_host_univ3.argtypes = [D, D, I64, dp, dp, ctypes.c_int, ip, dp, dp, dp]
    g = S.group(fx, "univ3")
    for s in range(len(g["cls"])):
        cp, gamma, lt, lq, cin, want = univ3_args(g, s)
        a, st, price = swap_out_univ3(host, cp, gamma, lt, lq, cin, want)
        lt, lq = np.ascontiguousarray(lt), np.ascontiguousarray(lq)
        cin = np.ascontiguousarray(cin, dtype=np.int32)
        out, p2 = np.empty(a.size), np.empty(a.size)
        assert fwd.swap_host_univ3(float(cp), float(gamma), lt.size, _p(lt, D), _p(lq, D), a.size, _p(cin, I32), _p(a, D), _p(out, D), _p(p2, D)) == 0
        np.testing.assert_array_equal(price.view(np.uint64), p2.view(np.uint64), err_msg=f"sequence {s}")


def test_refreshed_constants_are_swap_pool_h_expressions_of_the_new_reserves(fx, host):
    """the constants the swap refreshes (csrc/swap_pool.h swap_geomean_q, swap_weighted_q, swap_curve_q), restated with the
    same libm (math.log) in the same operation order, on the reserves the step left: bit for bit"""
    import math
    bits1 = lambda x: np.float64(x).view(np.uint64)
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            a, st, Rs, konst = swap_out_pool(host, *pool_args(g, s, fam))
            gm, w = float(g["gamma"][s]), [float(x) for x in g["w"][s]]
            for j in range(n):
                ci, co = int(g["cin"][s, j]), int(g["cout"][s, j])
                R = [float(x) for x in Rs[j]]
                if fam == "geomean":
                    e = w[0] / w[1]
                    lg, le, l1, l2 = math.log(gm), math.log(e), math.log(R[0]), math.log(R[1])
                    want = (((lg + le) + l2) + e * l1, e * ((lg + l1) - le) + l2)
                elif fam == "weighted":
                    ws = 0.0
                    for x in w:
                        ws += x
                    want = (math.log(R[ci] / (w[ci] / ws)), math.log(R[co] / (w[co] / ws)))
                elif fam == "curve":
                    want = (math.log(R[ci]), math.log(R[co]))
                else:
                    want = (0.0, 0.0)                                    # Product, Solidly: no constant depends on R
                assert (bits1(konst[j, 0]), bits1(konst[j, 1])) == (bits1(want[0]), bits1(want[1])), (name, s, j)
                assert fam in ("product", "solidly") or (konst[j, 0] != 0.0 and konst[j, 1] != 0.0)


def test_zero_wanted_leaves_every_bit_of_the_state(fx, host):
    for name in S.RESERVE_GROUPS:
        g, fam = S.group(fx, name), Q.family(name)
        for s in range(len(g["cls"])):
            a, st, Rs, konst = swap_out_pool(host, fam, g["R0"][s], g["gamma"][s], g["cin"][s, :1], g["cout"][s, :1], [0.0], g["w"][s],
                                             g["alpha"][s], g["beta"][s], max_in=[0.0])
            assert a.view(np.uint64)[0] == 0 and st[0] == APPLIED and np.all(konst == 0.0)   # +0.0, and no constant was rewritten
            np.testing.assert_array_equal(Rs[0].view(np.uint64), np.asarray(g["R0"][s]).view(np.uint64))
    g = S.group(fx, "univ3")
    for s in range(len(g["cls"])):
        o, e = g["tick_off"][s], g["tick_off"][s + 1]
        for ci in (0, 1):
            a, st, price = swap_out_univ3(host, g["cp"][s], g["gamma"][s], g["lower_ticks"][o:e], g["liquidity"][o:e], [ci], [0.0])
            assert a.view(np.uint64)[0] == 0 and st[0] == APPLIED and price.view(np.uint64)[0] == np.float64(g["cp"][s]).view(np.uint64)


# ---- statuses -----------------------------------------------------------------------------------------------------------------
def test_each_status_and_the_pool_it_leaves(host):
    R0 = [100.0, 250.0]
    q, _, Rq, _ = swap_out_pool(host, "product", R0, 0.997, [0], [1], [10.0])
    a, st, Rs, _ = swap_out_pool(host, "product", R0, 0.997, [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [250.0, 1e30, 10.0, 10.0, 10.0],
                                 max_in=[1e300, 1e300, np.nextafter(q[0], 0.0), q[0], 1e300])
    assert list(st) == [UNOBTAINABLE, UNOBTAINABLE, OVER_LIMIT, APPLIED, APPLIED]
    assert a[0] == a[1] == np.inf and a[2] == a[3] == q[0] and a[4] > a[3]
    for j in range(3):
        np.testing.assert_array_equal(Rs[j], R0)                          # the pool stays; the next swap starts from it
    np.testing.assert_array_equal(Rs[3], Rq[0])
    # the state tests are swap_pool.h's: a Solidly reserve may not leave [2^-150, 2^150]; a Curve log may not leave the solve's range
    a, st, Rs, _ = swap_out_pool(host, "solidly", [1.0, 2.0 ** -140], 0.997, [0, 0], [1, 1], [2.0 ** -140 * (1 - 2.0 ** -20), 2.0 ** -141])
    assert list(st) == [REFUSED, APPLIED] and np.isnan(a[0]) and a[1] == pytest.approx(0.26070316, rel=1e-6)
    np.testing.assert_array_equal(Rs[0], [1.0, 2.0 ** -140])
    a, st, Rs, _ = swap_out_pool(host, "curve", [1.0, 1.0], 0.9995, [0, 0], [1, 1], [0.9, 0.1], alpha=2.0, beta=float(np.exp(599.0)))
    assert list(st) == [REFUSED, APPLIED] and np.isnan(a[0]) and a[1] == pytest.approx(0.11116669, rel=1e-6)
    np.testing.assert_array_equal(Rs[0], [1.0, 1.0])
    # UniV3: beyond the ladder; over the limit; the pool keeps its price
    lt, lq = np.array([4.0, 1.0, 0.25]), np.full(3, 16.0)
    q, _, pq = swap_out_univ3(host, 0.6, 0.997, lt, lq, [1], [1.0])
    a, st, price = swap_out_univ3(host, 0.6, 0.997, lt, lq, [1, 1, 1], [1e9, 1.0, 1.0], max_in=[1e300, np.nextafter(q[0], 0.0), q[0]])
    assert list(st) == [UNOBTAINABLE, OVER_LIMIT, APPLIED] and a[0] == np.inf and a[1] == a[2] == q[0]
    assert price[0] == price[1] == 0.6 and price[2] == pq[0] > 0.6


def walk_path_out(pools, path, want, max_in=None):
    """cfmm_swap_path_out's two passes on one path, restated with numpy on Product pools {R_in, R_out, γ} (quote_out_precise_ref's
    qo_product; the state tests of csrc/swap_pool.h) -> (amount_in, status, hop_in [hops], the pools afterwards)"""
    nh = len(path)
    hop_in = np.full(nh, np.nan)
    y, status = np.float64(want), APPLIED
    k = nh - 1
    while k >= 0 and status == APPLIED:                                  # pass 1, the last hop first
        Ri, Ro, g = pools[path[k]]
        r = np.float64(QO.qo_product(Ri, Ro, g, y))
        if r == np.inf:
            y, status = np.inf, UNOBTAINABLE
        elif y != 0.0 and not (0 < Ri + g * r < np.inf and 0 < Ro - y < np.inf):
            y, status = np.nan, REFUSED
        else:
            y = r
        hop_in[k] = y
        k -= 1
    hop_in[:k + 1] = y                                                   # towards hop 0 of the hop that refused or cannot give
    if status == APPLIED and max_in is not None and not (y <= max_in):
        status = OVER_LIMIT
    after = dict(pools)
    if status == APPLIED:                                                # pass 2
        out = np.float64(want)
        for k in reversed(range(nh)):
            Ri, Ro, g = pools[path[k]]
            if out != 0.0:
                after[path[k]] = (Ri + g * hop_in[k], Ro - out, g)
            out = hop_in[k]
    return y, status, hop_in, after


def test_the_backward_walk_and_its_statuses_restated(host):
    """the restatement against chaining the host build's single swaps hop by hop, and each status's outputs"""
    pools = {"A": (100.0, 250.0, 0.997), "B": (4000.0, 90.0, 0.9995), "C": (7.0, 5000.0, 1.0), "tiny": (1e-25, 1e-25, 0.997)}
    path = ["A", "B", "C"]
    y, st, hops, after = walk_path_out(pools, path, 40.0)
    assert st == APPLIED and np.all(np.isfinite(hops)) and hops[0] == y
    out = 40.0
    for k in reversed(range(3)):                                         # the chain of cfmm_swap_out, last hop first
        Ri, Ro, g = pools[path[k]]
        a, s1, Rs, _ = swap_out_pool(host, "product", [Ri, Ro], g, [0], [1], [out])
        assert s1[0] == APPLIED and a.view(np.uint64)[0] == np.float64(hops[k]).view(np.uint64)
        np.testing.assert_array_equal(Rs[0], after[path[k]][:2])
        out = a[0]
    # over the limit: the would-be quote and the hop amounts, nothing moved; a limit equal to the quote is met
    y2, st2, hops2, after2 = walk_path_out(pools, path, 40.0, max_in=np.nextafter(y, 0.0))
    assert st2 == OVER_LIMIT and y2 == y and np.array_equal(hops2, hops) and after2 == pools
    assert walk_path_out(pools, path, 40.0, max_in=y)[1] == APPLIED
    # unobtainable in the middle: that hop, every earlier hop and the answer are +inf; the hop behind keeps its amount
    y3, st3, hops3, after3 = walk_path_out(pools, ["A", "tiny", "C"], 40.0)
    assert st3 == UNOBTAINABLE and y3 == np.inf and hops3[0] == hops3[1] == np.inf and hops3[2] == hops[2] and after3 == pools
    # wanted 0: +0.0 at every hop, nothing moved
    y4, st4, hops4, after4 = walk_path_out(pools, path, 0.0, max_in=0.0)
    assert st4 == APPLIED and y4 == 0.0 and np.all(hops4 == 0.0) and after4 == pools


def test_the_path_entrys_limit_check_names_the_first_hop(host):
    n_hops = np.array([2, 1], dtype=np.int32)
    seg = np.array([0, 1, 1, -77], dtype=np.int32)
    row = np.array([5, 5, 6, 1 << 40], dtype=np.int64)
    msg = ctypes.create_string_buffer(256)
    call = lambda lim: host.swap_out_host_check(2, _p(n_hops, I32), _p(seg, I32), _p(row, I64), _p(lim, D), msg, 256)
    assert call(None) == 0 and call(np.array([0.0, 1e300])) == 0
    for x in (-1.0, np.nan, np.inf):
        assert call(np.array([1.0, x])) == -1
        assert msg.value.decode() == "cfmm_swap_path_out: path 1, hop 0: max_amount_in must be finite and >= 0"
    seg[2], row[2] = 0, 5                                                # path 0 names pool (0, 5) twice
    assert call(None) == -1 and "cfmm_swap_path_out: path 0, hops 0 and 1: row 5 of segment 0 appears twice" in msg.value.decode()


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "swap_out_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DSWAP_OUT_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SHIM, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "SWAP_OUT_HOST_OK" in r.stdout and r.stderr == ""
    assert "cfmm_swap_path_out: path 1, hop 0: max_amount_in" in r.stdout
