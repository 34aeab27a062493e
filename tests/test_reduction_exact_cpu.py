"""The reduction reference (tests/reduction_ref.py) checked on the CPU: the oracle's own sums pass it, and every corruption
of Ψ that a reduction kernel could commit on a small token is rejected by it WHILE the suite's older measure,
rel_to_max(Ψ, Ψ_oracle) <= 1e-12, accepts it.  Plus the fold's block -> column-group map, the gather's rank-ordered sum and
its tag rule, restated in NumPy."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import reduction_ref as rr
from helpers import oracle_sweep, rel_to_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 96


@pytest.fixture(scope="module")
def market():
    deg = rr.default_degrees(N, seed=7)
    batches, v, e = rr.ill_scaled_market(N, deg, 400, seed=7)
    D, L, psi, acc = oracle_sweep(batches, N, v)
    Ai0 = rr.flat_tokens(batches)
    cnt = rr.assert_ill_scaled(D, L, Ai0, N, batches)
    for a in (D, L, psi, v):
        a.setflags(write=False)
    return dict(D=D, L=L, Ai0=Ai0, v=v, psi=psi, acc=acc, cnt=cnt, e=e)


def _small_token(mk, count):
    """A token with `count` nonzero flows (at least, for count >= 2) whose flows are 2^-60 of the market's largest."""
    fs, starts = rr.token_terms(mk["D"], mk["L"], mk["Ai0"], N)
    big = np.max(np.abs(mk["psi"]))
    for j in np.argsort(mk["e"], kind="stable"):
        ok = mk["cnt"][j] == count if count < 2 else mk["cnt"][j] >= count
        if ok and np.max(np.abs(fs[starts[j]:starts[j + 1]]), initial=0.0) <= 2.0 ** -60 * big:
            t = fs[starts[j]:starts[j + 1]]
            return int(j), t[t != 0.0]
    raise AssertionError("the market has no such token")


def _rejected_but_invisible(mk, psi):
    fails, _ = rr.reduction_report(mk["D"], mk["L"], mk["Ai0"], mk["v"], N, psi, mk["acc"])
    assert fails, "the exact reference must reject this Ψ"
    assert rel_to_max(psi, mk["psi"]) <= 1e-12, "... which max-error over max-|Ψ| accepts"
    with pytest.raises(AssertionError):
        rr.assert_reduction_exact(mk["D"], mk["L"], mk["Ai0"], mk["v"], N, psi, mk["acc"], geometry="cpu")
    print(f"rel_to_max = {rel_to_max(psi, mk['psi']):.3e} (passes 1e-12); exact reference: {fails[0]}")
    return fails


def test_the_oracles_own_sums_pass(market):
    worst = rr.assert_reduction_exact(market["D"], market["L"], market["Ai0"], market["v"], N, market["psi"], market["acc"])
    assert worst <= 1.0
    print(f"oracle: worst |error| / bound = {worst:.3f}")


def test_a_dropped_flow_on_a_small_token(market):
    j, t = _small_token(market, 3)
    psi = market["psi"].copy()
    psi[j] -= t[0]
    fails = _rejected_but_invisible(market, psi)
    assert f"token {j} " in fails[0]


def test_a_flow_booked_on_the_neighbouring_token(market):
    j, t = _small_token(market, 3)
    k = j + 1 if j + 1 < N else j - 1
    psi = market["psi"].copy()
    psi[j] -= t[-1]
    psi[k] += t[-1]
    fails = _rejected_but_invisible(market, psi)
    assert any(f"token {j} " in f for f in fails)


def test_a_flow_added_twice(market):
    j, t = _small_token(market, 2)
    psi = market["psi"].copy()
    psi[j] += t[0]
    _rejected_but_invisible(market, psi)


def test_minus_zero_on_an_untouched_token(market):
    j, _ = _small_token(market, 0)
    assert market["psi"][j] == 0.0 and not np.signbit(market["psi"][j])
    psi = market["psi"].copy()
    psi[j] = -0.0
    fails = _rejected_but_invisible(market, psi)
    assert "expected +0.0" in fails[0]


def test_one_ulp_on_a_token_with_one_flow(market):
    j, t = _small_token(market, 1)
    assert market["psi"][j] == t[0]
    for side in (np.inf, -np.inf):
        psi = market["psi"].copy()
        psi[j] = np.nextafter(psi[j], side)
        fails = _rejected_but_invisible(market, psi)
        assert "bit for bit" in fails[0]


def test_a_wrong_dual_value_is_rejected(market):
    with pytest.raises(AssertionError, match="acc"):
        rr.assert_reduction_exact(market["D"], market["L"], market["Ai0"], market["v"], N, market["psi"],
                                  market["acc"] * (1.0 + 1e-9))


def test_every_column_group_has_one_fold_block():
    """fold_colblock / fold_grid: every column group of n1 columns is owned by exactly one block of the grid, every other
    block is idle (its group lies past the last), and the two groups of one 128-byte line sit on the same XCD (b % 8)."""
    for n1 in range(1, 601):
        grid = rr.fold_grid(n1)
        groups = (n1 + 7) // 8
        owner = np.array([rr.fold_colblock(b) for b in range(grid)])
        assert grid % 16 == 0 and len(set(owner)) == grid
        live = owner[owner * 8 < n1]
        assert sorted(live) == list(range(groups))
        assert np.all(owner[owner >= groups] * 8 >= n1)
        where = {g: b for b, g in enumerate(owner)}
        for p in range(groups // 2):
            assert where[2 * p] % 8 == where[2 * p + 1] % 8 and where[2 * p + 1] - where[2 * p] == 8
    assert rr.fold_colblock(16) == 16 and rr.fold_grid(129) == 32   # 129 columns: the first group of the second deal


def test_the_gather_sum_is_rank_ordered():
    x = np.array([[1e30, 1.0, -0.0, np.inf], [1.0, 2.0 ** -60, -0.0, 1.0], [-1e30, -1.0, -0.0, -np.inf]])
    s = rr.gather_sum(x)
    assert s[0] == 0.0 and s[1] == 0.0                      # (1e30 + 1) − 1e30 = 0: the order is part of the result
    assert s[2] == 0.0 and not np.signbit(s[2])             # 0.0 + (−0.0) = +0.0
    assert np.isnan(s[3])
    assert rr.gather_sum(x[[0, 2, 1]])[0] == 1.0 and rr.gather_sum(x[[0, 2, 1]])[1] == 2.0 ** -60


def test_the_tag_rule_never_yields_zero_and_wraps_at_2_32_minus_1():
    for seq, tag in ((1, 2), (2, 3), (2 ** 32 - 3, 2 ** 32 - 2), (2 ** 32 - 2, 2 ** 32 - 1), (2 ** 32 - 1, 1), (2 ** 32, 2),
                     (2 ** 32 + 1, 3), (2 ** 40 + 2, (2 ** 40 + 2) % (2 ** 32 - 1) + 1)):
        assert rr.gather_tag(seq) == tag and 1 <= tag < 2 ** 32
    # consecutive launches of one parity (seq, seq + 2) never share a tag, across the wrap as well
    for seq in (2 ** 32 - 4, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1):
        assert rr.gather_tag(seq) != rr.gather_tag(seq + 2)
    g = rr.granules(np.array([1.5, -0.0]), 2 ** 32 - 1)
    assert g.dtype == np.uint64 and g.shape == (2, 2) and int(g[1, 1]) == (1 << 32) | 0x80000000 and int(g[1, 0]) == 1 << 32


@pytest.fixture(scope="module")
def plan_bin_copies(tmp_path_factory):
    """csrc/launch_plan.cpp's own bin_copies, built for the host behind tests/native/launch_plan_host.cpp (as
    tests/test_launch_plan_cpu.py builds the planner: it makes no HIP call)."""
    so = str(tmp_path_factory.mktemp("plan_bin_copies") / "launch_plan_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "launch_plan_host.cpp"),
                    os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "launch_plan.cpp"), "-o", so], check=True)
    f = ctypes.CDLL(so).launch_plan_bin_copies
    f.argtypes, f.restype = [ctypes.c_int] * 3, ctypes.c_int
    return f


def test_the_bin_copy_rule_is_the_plans_own(plan_bin_copies):
    """reduction_ref.planned_copies against launch_plan.cpp's bin_copies at EVERY n up to large-market mode, every option and
    both block sizes, and the auto thresholds the GPU tests straddle found by bisecting the C++ rule itself: if the plan's
    rule moves, this fails before a 'below' and an 'above' case can land on one side of it."""
    for block in (512, 1024):
        for option in (0, 1, 2):
            for n in range(1, 8500):
                assert rr.planned_copies(n, option, block) == plan_bin_copies(n, option, block), (n, option, block)
        lo, hi = 2, 8192
        assert plan_bin_copies(lo, 0, block) == block // 64 and plan_bin_copies(hi, 0, block) == 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if plan_bin_copies(mid, 0, block) > 1 else (lo, mid)
        assert rr.auto_threshold(block) == lo
        assert all(plan_bin_copies(n, 0, block) == block // 64 for n in range(2, lo + 1))      # one threshold only
        print(f"block {block}: private copies per wavefront up to n = {lo}, one shared copy from {lo + 1}")
    assert plan_bin_copies(8192, 2, 512) == 1 and plan_bin_copies(8193, 0, 512) == 1
