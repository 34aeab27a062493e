"""cfmm_size_path and cfmm_split_paths on the device against the 80-digit optima of tests/golden/optimum_precise.npz: the
inequalities of tests/test_optimum_precise_cpu.py (derived there and in tests/optimum_ref.py) on the device's own gain, total_out,
amount_in and shares, at rounds 5 and 16.  The bit-equality tests (tests/test_gpu_size_path.py, tests/test_gpu_split_paths.py)
prove that the device runs the contract's search; this proves that the search, over the device's quotes, reaches the optimum on
every pool family, on UniV3 tick boundaries and list ends, on Solidly cycles and on 8-hop paths.  The device's reported gain /
total is within e of the true one at its own amount_in / shares by the quote pins (tests/test_gpu_quote_precise.py): the `+ e`
of the bounds.  Run with -s for the worst case per class (profiles/optimum_precise.txt)."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import optimum_ref as O
from cfmmrouter_amd._lib import SIZED, SPLIT_OK, SPLIT_SATURATED

pytestmark = pytest.mark.gpu

N_TOKENS = 8
ROUNDS = (5, 16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def world():
    """the fixture's market on one context and the four calls, made once and left unchanged"""
    fx = O.load()
    ctx = cr.Context(N_TOKENS, 0)
    try:
        O.upload(ctx, fx)
        sized = {r: ctx.size_path(*O.hops_of(fx, "size"), fx["size_max_in"], fx["size_vi"], fx["size_vo"], r) for r in ROUNDS}
        split = {r: ctx.split_paths(fx["split_first"], fx["split_A"], *O.hops_of(fx, "split"), r) for r in ROUNDS}
        yield fx, ctx, sized, split
    finally:
        ctx.close()


@pytest.mark.parametrize("rounds", ROUNDS)
def test_sizing_reaches_the_optimum_within_resolution_and_noise(world, rounds):
    fx, ctx, sized, split = world
    x, y, g, st = sized[rounds]
    cls = O.names(fx, "size_classes", fx["size_cls"])
    short, bound = fx["size_g"] - g, O.size_bound(fx, rounds)
    for c in np.unique(cls):
        sel = cls == c
        print(f"size_path device rounds {rounds:2d} {c:14s}: worst (g* - g)/g* {np.max(short[sel] / fx['size_g'][sel]):.3g}, worst (g* - g)/bound "
              f"{np.max(short[sel] / bound[sel]):.3g}")
    assert np.all(st == SIZED)                                               # never SIZED_AT_LIMIT, NONE or NAN
    assert np.all(short <= bound)
    assert np.all((x > 0) & (x < fx["size_max_in"]))


@pytest.mark.parametrize("rounds", ROUNDS)
def test_amount_in_is_within_the_bracket_of_the_optimum(world, rounds):
    """`interior` and `plateau` without a Solidly hop: the final bracket plus the stretch noise cannot tell from x*
    (optimum_ref.size_x_bound)"""
    fx, ctx, sized, split = world
    x = sized[rounds][0]
    cls = O.names(fx, "size_classes", fx["size_cls"])
    used = np.arange(O.H)[None, :] < fx["size_n_hops"][:, None]
    solidly = np.array([np.any(fx["size_seg"][p, used[p]] == O.SEGMENTS.index("solidly")) for p in range(x.size)])
    bound = O.size_x_bound(fx, rounds)
    off = np.abs(x - fx["size_x"])
    for c in ("interior", "plateau"):
        sel = (cls == c) & ~solidly
        print(f"size_path device rounds {rounds:2d} {c:9s}: worst |amount_in - x*| / bound {np.max(off[sel] / bound[sel]):.3g}, / x* "
              f"{np.max(off[sel] / fx['size_x'][sel]):.3g}")
        assert sel.sum() >= 6 and np.all(off[sel] <= bound[sel])


@pytest.mark.parametrize("rounds", ROUNDS)
def test_splitting_reaches_the_optimum_within_resolution_and_noise(world, rounds):
    fx, ctx, sized, split = world
    path_in, path_out, total, st = split[rounds]
    kind = O.names(fx, "order_kinds", fx["split_kind"])
    short, bound = fx["split_T"] - total, O.split_bound(fx, rounds)
    for c in np.unique(kind):
        sel = kind == c
        print(f"split_paths device rounds {rounds:2d} {c:8s}: worst (T* - T)/T* {np.max(short[sel] / fx['split_T'][sel]):.3g}, worst (T* - T)/bound "
              f"{np.max(short[sel] / bound[sel]):.3g}")
    assert np.all((st == SPLIT_OK) | (st == SPLIT_SATURATED))
    assert np.all(short <= bound)


@pytest.mark.parametrize("rounds", ROUNDS)
def test_shares_sum_to_the_amount_and_lie_by_the_truth(world, rounds):
    fx, ctx, sized, split = world
    path_in = split[rounds][0]
    first, A = fx["split_first"], fx["split_A"]
    K = np.diff(first)
    order_of = np.repeat(np.arange(A.size), K)
    sums = np.array([np.sum(path_in[first[g]:first[g + 1]].astype(np.longdouble)) for g in range(A.size)])
    err = np.abs(sums - A.astype(np.longdouble)).astype(np.float64) / A
    kind = O.names(fx, "order_kinds", fx["split_kind"])
    empty = (fx["split_share"] == 0.0) & (kind[order_of] == "empty")
    sel = (O.s_ref_split(fx, rounds) < 1e-9 * fx["split_T"])[order_of] & (fx["split_curv"] > 0)
    bound = O.share_bound(fx, rounds)
    off = np.abs(path_in - fx["split_share"])
    print(f"split_paths device rounds {rounds:2d}: worst |sum of shares - A| / A {err.max():.3g}; {int(sel.sum())} of {sel.size} shares asserted, worst "
          f"|share - truth| / bound {np.max(off[sel] / bound[sel]):.3g}, / A {np.max(off[sel] / A[order_of][sel]):.3g}")
    assert np.all(err <= 3e-16)                                              # the header's 3e-16·A
    assert empty.sum() >= 2                                                  # the path the optimum leaves empty: +0.0 through 5 rounds,
    if rounds <= 5:                                                          # beyond them at most round 6's remainder (the CPU test says why)
        assert not np.any(bits(path_in[empty]))
    else:
        print(f"split_paths device rounds {rounds:2d}: the empty paths hold {path_in[empty]}")
        assert np.all(path_in[empty] <= (A * (K / 63.0) ** 5)[order_of][empty])
    assert np.all(off[sel] <= bound[sel])
    np.testing.assert_array_equal(bits(split[rounds][1]), bits(ctx.quote_path(*O.hops_of(fx, "split"), path_in)))    # the round trip
