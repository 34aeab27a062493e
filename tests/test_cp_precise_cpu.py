"""The 60-digit fixture tests/golden/cp_precise.npz on the CPU: its truth re-derived at 80 digits; the C oracle's
ProductTwoCoin and UniV3 (what the GPU suite compares bit for bit) held to the scale-aware bounds of
tests/cp_precise_ref.py; and the constants csrc/univ3_pool.h prepares at upload (current-tick record, walk lists, prefix
sums, bisection-found drain thresholds, closing records), fed through a plain NumPy restatement of find_arb_pos that jumps
over the drained ticks the way the device does, held to the same bounds.  The device paths: tests/test_gpu_cp_precise.py.

K per class: the next power of two >= 2x the largest ratio observed here (printed with -s:
profiles/cp_precise_cpu_tests.log), capped at 16 on well / inside / walk_head / walk_deep and at 64 elsewhere."""
import ast
import ctypes
import importlib.util
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import cfmmrouter_amd as cr
import cp_precise_ref as P
from helpers import oracle_sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC, UC, PCLS, UCLS = P.load()

K_PRODUCT, K_UNIV3 = P.K_PRODUCT, P.K_UNIV3


def _k(table, names, cls):
    return np.array([table[names[c]] for c in cls], dtype=np.float64)


def _generator():
    path = os.path.join(ROOT, "tests", "golden", "make_cp_precise_golden.py")
    spec = importlib.util.spec_from_file_location("make_cp_precise_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _univ3_batch(c):
    return cr.UniV3.batch(c["cp"], c["tick_off"], c["lower_ticks"], c["liquidity"], c["gamma"], c["Ai"])


def test_k_tables_respect_the_caps():
    for table in (K_PRODUCT, K_UNIV3):
        for name, k in table.items():
            assert k <= (16 if name in P.WELL else 64), name


def test_fixture_shape():
    assert os.path.getsize(P.PATH) <= 1 << 20
    assert sorted(PC) == ["p_main", "p_pxout", "p_resout"] and sorted(UC) == ["bounded", "u_main", "u_resout"]
    seen = set()
    for c in PC.values():
        m = len(c["gamma"])
        assert m <= 2200 and 16 <= len(c["v"]) <= 64 and c["zclear"].shape == (m, 2)
        seen |= set(np.unique(c["cls"]))
        trades = np.any(c["D"] > 0, axis=1) & np.any(c["L"] > 0, axis=1)
        assert np.count_nonzero(trades) >= 0.8 * m
    assert seen == set(range(len(PCLS)))
    both = PC["p_main"]["cls"] == PCLS.index("both_live")
    assert np.count_nonzero(np.all(PC["p_main"]["D"][both] > 0, axis=1)) >= 100     # most γ > 1 pools trade both ways
    seen = set()
    for name, c in UC.items():
        m = len(c["gamma"])
        assert m <= 2200 and 16 <= len(c["v"]) <= 64 and c["zclear"].shape == (m,) and c["tick_off"][-1] == len(c["liquidity"])
        seen |= set(np.unique(c["cls"]))
        band = c["cls"] == UCLS.index("band")
        trades = np.any(c["D"] > 0, axis=1) & np.any(c["L"] > 0, axis=1)
        assert np.count_nonzero(trades[~band]) >= 0.8 * np.count_nonzero(~band)
        if name != "u_resout":
            assert np.count_nonzero(c["zclear"][band]) >= 20 and np.count_nonzero(trades[band]) >= 20
        assert np.all(c["D"][c["zclear"]] == 0) and np.all(c["L"][c["zclear"]] == 0)
    assert seen == set(range(len(UCLS)))
    b = UC["bounded"]                                            # two ticks, the second empty: no walk list anywhere
    assert np.all(np.diff(b["tick_off"]) == 2) and np.all(b["liquidity"][1::2] == 0) and np.all(b["liquidity"][0::2] > 0)
    assert {UCLS[k] for k in np.unique(b["cls"])} == {"inside", "drained_all", "band", "cp_on_tick", "narrow"}
    u = UC["u_main"]
    nt, off = np.diff(u["tick_off"]), u["tick_off"][:-1]
    ct = np.array([np.count_nonzero(u["lower_ticks"][o:o + n] >= q) for o, n, q in zip(off, nt, u["cp"])])
    on = u["cls"] == UCLS.index("cp_on_tick")
    assert np.all(u["lower_ticks"][off[on] + ct[on] - 1] == u["cp"][on])            # cp is one of its own lower_ticks
    assert np.count_nonzero(ct[on] == 1) >= 20 and np.count_nonzero(ct[on] > 1) >= 20
    assert np.count_nonzero(u["liquidity"][off + ct - 1][u["cls"] == UCLS.index("empty_cur")] == 0) >= 50
    head = u["cls"] == UCLS.index("walk_head")
    falling = u["D"][:, 0] > 0
    assert {3, 4, 5} <= set((nt - ct)[head & falling]) and {3, 4, 5} <= set((ct - 1)[head & ~falling])   # list lengths
    assert "v2" in PC["p_main"] and "v2" in u


def _walks(c):
    """per pool, as the device forms them: falling, the target price P, the 0-based current tick and the tick that holds P
    (-1: P lies above the first tick), and the pool's ticks"""
    vp, g, cp = c["v"][c["Ai"] - 1], c["gamma"], c["cp"]
    pr = vp[:, 0] / vp[:, 1]
    falling = pr < g * cp
    Pt = np.where(falling, pr / g, g * pr)
    out = []
    for i in range(len(cp)):
        lt = c["lower_ticks"][c["tick_off"][i]:c["tick_off"][i + 1]]
        lq = c["liquidity"][c["tick_off"][i]:c["tick_off"][i + 1]]
        out.append((bool(falling[i]), Pt[i], np.count_nonzero(lt >= cp[i]) - 1, np.count_nonzero(lt >= Pt[i]) - 1, lt, lq))
    return out


def test_fixture_holds_every_mechanism_the_classes_name():
    """What a generator edit could silently drop: the list positions at which the four-at-a-time threshold scan wraps, the
    2^-k ladder of on_boundary with its exact and ulp-level rows, the narrow spacings, the runs of empty ticks, the fee set
    and the out-of-float-range thresholds of `wide`."""
    u = UC["u_main"]
    W = _walks(u)
    rows = lambda name: np.flatnonzero(u["cls"] == UCLS.index(name))
    for falling in (True, False):                                 # walk_deep (no empty ticks): the walk ends at list position |e − ct| − 1
        ends = {abs(W[i][3] - W[i][2]) - 1 for i in rows("walk_deep") if W[i][0] == falling and np.all(W[i][5] > 0)}
        assert {4, 7, 8, 9} <= ends and max(ends) >= 30 and min(ends) >= 4, (falling, sorted(ends))
    ks, ulps = set(), set()
    for i in rows("on_boundary"):                                 # P = boundary·(1 ± 2^-k), exactly on it, and 1..3 ulps beside it
        _, Pt, _, _, lt, _ = W[i]
        B = lt[np.argmin(np.abs(lt / Pt - 1.0))]
        d = int(np.float64(Pt).view(np.int64)) - int(np.float64(B).view(np.int64))
        if abs(d) <= 3:
            ulps.add(d)
        else:
            rel = abs(Pt / B - 1.0)
            k = int(round(-np.log2(rel)))
            assert abs(rel * 2.0 ** k - 1.0) <= max(1e-5, 2.0 ** (k - 49)), (i, rel)   # (the roundings of P, B and P/B: a few 2^-52)
            ks.add((k, Pt > B))
    assert {(k, s) for k in range(20, 50) for s in (True, False)} <= ks, sorted(ks)
    assert ulps == {-3, -2, -1, 0, 1, 2, 3}
    for name, c in (("u_main", u), ("bounded", UC["bounded"])):   # narrow: spacing 1 + 2^-k, k = 7..16
        nk = set()
        for i in np.flatnonzero(c["cls"] == UCLS.index("narrow")):
            lt = c["lower_ticks"][c["tick_off"][i]:c["tick_off"][i + 1]]
            if len(lt) > 1:
                k = -np.log2(lt[:-1] / lt[1:] - 1.0)
                assert np.all(np.abs(k - np.round(k)) < 1e-6), (name, i)
                nk |= set(np.round(k).astype(int))
        assert nk == set(range(7, 17)), (name, sorted(nk))
    runs, cur_empty = set(), 0
    for i in rows("empty_cur"):                                   # runs of 1-5 empty ticks inside the walk; empty current ticks
        falling, _, ct, e, _, lq = W[i]
        cur_empty += lq[ct] == 0
        path = lq[ct + 1:max(e, ct) + 1] if falling else lq[max(e, 0):ct][::-1]
        n = 0
        for z in list(path == 0) + [False]:
            if z:
                n += 1
            elif n:
                runs.add(n)
                n = 0
    assert {1, 2, 3, 4, 5} <= runs and cur_empty >= 50, (sorted(runs), cur_empty)
    assert set(u["gamma"][rows("gamma")]) == {1.0, 1.0 - 2.0 ** -52, 0.997, 0.3}
    wide = rows("wide")                                           # every boundary, hence every drain threshold, outside 2^±120
    for i in wide:
        lt, lq = W[i][4], W[i][5]
        assert np.all((lt > 2.0 ** 120) | (lt < 2.0 ** -120)) and np.all((lq == 0) | (lq > 2.0 ** 90) | (lq < 2.0 ** -80))
    assert sum(abs(W[i][3] - W[i][2]) >= 1 for i in wide) >= 50   # ... and most of them walk through list ticks
    drained = rows("drained_all")
    assert sum(W[i][3] == -1 for i in drained) >= 20              # rising past lower_ticks[0]
    assert sum(W[i][0] and W[i][3] == len(W[i][4]) - 1 and W[i][5][-1] > 0 for i in drained) >= 20    # into a last tick that reaches 0
    assert sum(W[i][0] and W[i][3] == len(W[i][4]) - 1 and W[i][5][-1] == 0 for i in drained) >= 20   # past an empty last tick
    p = PC["p_main"]
    assert set(p["gamma"][p["cls"] == PCLS.index("gamma1")]) == {1.0} and np.all(p["gamma"][p["cls"] == PCLS.index("both_live")] > 1)
    assert np.all(np.any(np.abs(np.log2(PC["p_resout"]["R"])) > 150, axis=1)) and np.max(PC["p_pxout"]["v"]) > 2.0 ** 150
    assert np.all(np.abs(np.log2(UC["u_resout"]["liquidity"][UC["u_resout"]["liquidity"] > 0])) > 150)


def test_k_tables_are_the_rule_applied_to_the_committed_logs():
    """K per class = the next power of two >= 2x the largest ratio in profiles/cp_precise_cpu_tests.log (oracle, prepared
    constants) and profiles/cp_precise_gpu_tests.log (every device path)."""
    worst = {}
    prof = os.path.join(ROOT, "profiles")
    for line in open(os.path.join(prof, "cp_precise_cpu_tests.log")):
        m = re.match(r"\[(oracle|prepared)\] (\w+): max ratio by class (\{.*\})", line)
        if m:
            fam = "product" if m.group(2) in PC else "univ3"
            for k, x in ast.literal_eval(m.group(3)).items():
                worst[(fam, k)] = max(worst.get((fam, k), 0.0), x)
    cpu = dict(worst)
    paths = set()
    for line in open(os.path.join(prof, "cp_precise_gpu_tests.log")):
        m = re.match(r"  (\w+)\s+(\w+)\s+((?:\w+=[\d.e+-]+\s*)+)$", line)
        if m:
            paths.add(m.group(2))
            fam = "product" if m.group(1) in PC else "univ3"
            for kv in m.group(3).split():
                k, x = kv.split("=")
                worst[(fam, k)] = max(worst.get((fam, k), 0.0), float(x))
    assert paths == {"host_fast", "host_full", "dev_auto", "dev_window", "direct", "pack0", "compact0", "heads0", "moved", "mixed"}
    assert set(cpu) == {("product", k) for k in PCLS} | {("univ3", k) for k in UCLS}
    for fam, table in (("product", K_PRODUCT), ("univ3", K_UNIV3)):
        assert {k: P.k_from(worst[(fam, k)]) for k in table} == table, fam


def _sample(cases, rng, count):
    rows = [(name, i) for name, c in sorted(cases.items()) for i in range(len(c["gamma"]))]
    return [rows[j] for j in rng.choice(len(rows), count, replace=False)]


def test_truth_rederived_at_80_digits_is_bit_equal():
    """256 seeded rows per family: the stored float64 truth is the 80-digit value rounded once."""
    gen = _generator()
    rng = np.random.default_rng(80)
    with mp.workdps(80):
        for name, i in _sample(PC, rng, 256):
            c = PC[name]
            d1, d2, l1, l2 = gen.prod_truth(c["R"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
            assert [gen._f(x) for x in (d1, d2, l1, l2)] == [c["D"][i, 0], c["D"][i, 1], c["L"][i, 0], c["L"][i, 1]], (name, i)
        for name, i in _sample(UC, rng, 256):
            c = UC[name]
            lt, lq = gen.pool_ticks(c, i)
            d1, d2, l1, l2 = gen.v3_truth(c["cp"][i], lt, lq, c["gamma"][i], c["v"][c["Ai"][i] - 1])
            assert [gen._f(x) for x in (d1, d2, l1, l2)] == [c["D"][i, 0], c["D"][i, 1], c["L"][i, 0], c["L"][i, 1]], (name, i)


def _check(tag, name, c, names, table, D, L, bD, bL):
    r = P.ratios(D, L, c["D"], c["L"], bD, bL)
    print(f"\n[{tag}] {name}: max ratio by class {P.class_max(r, c['cls'], names)}")
    kk = _k(table, names, c["cls"])
    assert np.all(r <= kk), (name, np.flatnonzero(r > kk)[:8], r[r > kk][:8])
    assert P.zero_rows_exact(D, L, c["zclear"]), name
    return r


@pytest.mark.parametrize("name", sorted(PC))
def test_oracle_meets_the_product_bound(name):
    c = PC[name]
    with np.errstate(all="ignore"):
        D, L, _, _ = oracle_sweep([cr.ProductTwoCoin.batch(c["R"], c["gamma"], c["Ai"])], len(c["v"]), c["v"])
    _check("oracle", name, c, PCLS, K_PRODUCT, D, L, *P.product_scale(c["R"], c["gamma"], c["D"], c["L"]))


@pytest.mark.parametrize("name", sorted(UC))
def test_oracle_meets_the_univ3_bound(name):
    """... the cp_on_tick noise trades included: a pool whose cp is its own tick's upper boundary returns, when the price
    rises, δmax = k/α − (R₂+β) of that tick -- rounding noise of either sign -- as the reference does (src/cfmms.jl:329-332;
    the current tick is exempt from the break of :383-385).  Its size is held to the bound; its sign is not."""
    c = UC[name]
    with np.errstate(all="ignore"):
        D, L, _, _ = oracle_sweep([_univ3_batch(c)], len(c["v"]), c["v"])
    _check("oracle", name, c, UCLS, K_UNIV3, D, L, *P.univ3_scale(c))
    if name == "u_main":
        on = c["cls"] == UCLS.index("cp_on_tick")
        noise = on & np.all(c["D"] == 0, axis=1) & np.any(D != 0, axis=1)
        print(f"[oracle] {name}: {int(noise.sum())} cp_on_tick pools trade rounding noise where the truth is zero, "
              f"{int(np.count_nonzero(D[noise] < 0))} of them a negative Δ (min {D[noise].min():.3g}, max {D[noise].max():.3g})")
        assert noise.any() and np.all(L[noise] == 0)


# ---- the constants the upload prepares (csrc/univ3_pool.h), through a NumPy restatement of find_arb_pos -------------

@pytest.fixture(scope="module")
def prepare_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("univ3_prepare") / "univ3_prepare_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"), "-O3", "-std=c++17", "-ffp-contract=off", "-mavx2", "-shared",
                    "-fPIC", os.path.join(ROOT, "tests", "native", "univ3_prepare_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.univ3_prepare_host.restype = ctypes.c_longlong
    lib.univ3_prepare_host.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 14
    return lib


def _prepare(lib, c):
    m, T = len(c["gamma"]), int(c["tick_off"][-1])
    out = dict(pg=np.empty((m, 2)), cur_a=np.empty((m, 2)), cur_b=np.empty((m, 2)), cur_c=np.empty(m), curR=np.empty((m, 2)),
               walk=np.empty((m, 4), dtype=np.int32), head=np.empty((m, 8), dtype=np.uint32))
    ticks, thr = np.empty((T + 2 * m, 8)), np.empty(T + 2 * m + 4)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ins = [np.ascontiguousarray(c[k]) for k in ("cp", "gamma", "tick_off", "lower_ticks", "liquidity")]
    n = lib.univ3_prepare_host(m, *(p(a) for a in ins), p(out["pg"]), p(out["cur_a"]), p(out["cur_b"]), p(out["cur_c"]),
                               p(out["curR"]), p(out["walk"]), p(ticks), p(thr), p(out["head"]))
    assert 2 * m <= n <= T + 2 * m
    out.update(ticks=ticks[:n], thr=thr[:n + 4])
    return out


def _pos(k, s_in, dmax, s_out, r_out, price):
    """find_arb_pos (src/cfmms.jl:321-337) on prepared constants"""
    dd = np.sqrt(k / price) - s_in
    if not dd > 0:
        return 0.0, 0.0
    if dd >= dmax:
        return dmax, r_out
    return dd, s_out - np.sqrt(price * k)


def _prepared_sweep(q, c, stop_after_jump=False):
    """find_arb! on the prepared constants alone: the current-tick record, then -- when it drains or is empty -- the
    thresholds say how many list ticks drain, the record reached carries their sums, and find_arb_pos goes on from it."""
    m = len(c["gamma"])
    D, L = np.zeros((m, 2)), np.zeros((m, 2))
    vp = c["v"][c["Ai"] - 1]
    T = q["ticks"]
    with np.errstate(all="ignore"):
        for i in range(m):
            cp, g = q["pg"][i]
            pr = vp[i, 0] / vp[i, 1]
            if g * cp <= pr <= cp / g:
                continue
            up = pr < g * cp
            price = pr / g if up else 1.0 / (g * pr)
            k0 = q["cur_a"][i, 0]
            sd = sl = 0.0
            partial = False
            if k0 != 0:
                s_in, s_out = (q["cur_a"][i, 1], q["cur_b"][i, 0]) if up else (q["cur_b"][i, 0], q["cur_a"][i, 1])
                dmax = q["cur_b"][i, 1] if up else q["cur_c"][i]
                sd, sl = _pos(k0, s_in, dmax, s_out, q["curR"][i, 1 if up else 0], price)
                dd = np.sqrt(k0 / price) - s_in
                partial = not (dd > 0 and dd >= dmax)
            begin, count = (q["walk"][i, 0], q["walk"][i, 1]) if up else (q["walk"][i, 2], q["walk"][i, 3])
            j = 0
            jumped = not partial and count > 0
            if jumped:
                while j < count and price <= q["thr"][begin + j]:
                    j += 1
                assert q["thr"][begin + count] == 0 and T[begin + count, 5] == 0      # the closing record: "never"
                sd, sl = T[begin + j, 6], T[begin + j, 7]
            while j < count:
                k, s_in, dmax, s_out, r_out = T[begin + j, :5]
                assert T[begin + j, 5] == q["thr"][begin + j]
                dj, lj = _pos(k, s_in, dmax, s_out, r_out, price)
                if dj == 0 or lj == 0:
                    break
                sd, sl = sd + dj, sl + lj
                j += 1
                if jumped and stop_after_jump:
                    break
            D[i, 0 if up else 1], L[i, 1 if up else 0] = sd / g, sl
    return D, L


@pytest.mark.parametrize("name", sorted(UC))
def test_prepared_constants_meet_the_univ3_bound(name, prepare_lib):
    c = UC[name]
    q = _prepare(prepare_lib, c)
    if name == "u_main":                      # wide: thresholds outside 2^±120 -> the head holds "ask thr[]" (NaN) or "never" (0)
        wide = c["cls"] == UCLS.index("wide")
        assert np.all(np.isin(q["head"][wide], [0, 0x7fc00000])) and np.count_nonzero(q["head"][wide] == 0x7fc00000) >= 100
        assert not np.any(q["head"][c["cls"] == UCLS.index("walk_head")] == 0x7fc00000)
    D, L = _prepared_sweep(q, c)
    _check("prepared", name, c, UCLS, K_UNIV3, D, L, *P.univ3_scale(c))
    with np.errstate(all="ignore"):
        Do, Lo, _, _ = oracle_sweep([_univ3_batch(c)], len(c["v"]), c["v"])
    np.testing.assert_array_equal(D, Do)      # ... and the thresholds and prefix sums decide as the tick-by-tick walk does
    np.testing.assert_array_equal(L, Lo)


def test_no_tick_is_entered_after_a_partial_one(prepare_lib):
    """The device leaves the walk after the first tick that does not drain unless the price is within 2^-40 of that tick's
    threshold (ops_univ3.h solve_dir).  On every row here -- targets exactly on a boundary and 1..3 ulps beside it
    included -- leaving ALWAYS gives the oracle's bits: the reference itself enters no tick after a partial one, so the
    band is a safety net that these fixtures do not exercise (a band of 0 passes them too)."""
    for name in ("u_main", "u_resout"):
        c = UC[name]
        D, L = _prepared_sweep(_prepare(prepare_lib, c), c, stop_after_jump=True)
        with np.errstate(all="ignore"):
            Do, Lo, _, _ = oracle_sweep([_univ3_batch(c)], len(c["v"]), c["v"])
        np.testing.assert_array_equal(D, Do)
        np.testing.assert_array_equal(L, Lo)
