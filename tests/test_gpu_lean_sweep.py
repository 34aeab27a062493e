"""The lean form of the sweep kernels (sweep_core.h sweep_body<..., LEAN>; launch_plan.cpp lean_launch; option
"lean_kernels", read-only option "lean_launches").

A launch in the default configuration takes a kernel in which the trade layout, the store policy, the price staging, the fee
table and the bin copies are compile-time facts, pool streams are addressed with 32-bit offsets and only the blocks of a
family that reads log v stage it.  It must return the general kernel's bits: every market below is swept by a context with
"lean_kernels" = 1 and by one with 0, and Δ, Λ, Ψ and the dual value are compared with np.array_equal; "lean_launches" says
which kernels ran.  Fused and materialising, in both tile directions (consecutive sweeps alternate); host pointers launch
the fast arithmetic, device pointers the kernels that carry both and pick per block from the prices they stage.

Markets: one block per family with two full tiles and a tail (1 500 pools under "max_grid" = 2) at 8 and 257 tokens; the
XCD-aware block map (2 x 70 000 pools under "max_grid" = 256); each family alone in 1024-thread blocks with several tiles per
lane (two blocks: a launch of ONE block is a direct launch, which stays on the general kernels -- see BIG_BLOCKS).  Into them go the pools of the rare paths: inside the no-arbitrage band (no trade), fees above 1 that trade both ways
(overflow rows), UniV3 pools on degenerate boundaries (negative zeros); and price vectors with a NaN and with a price outside
the window of the fast arithmetic.  Every configuration the predicate excludes launches the general kernels and counts 0."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from helpers import dev_sweep
from reduction_ref import assert_reduction_exact
from test_gpu_pool_update import batch_with
from test_gpu_select_trades import degenerate_univ3
from test_gpu_sweep_entry import backend

pytestmark = pytest.mark.gpu

EDGE = 40   # rows of every Product / GeometricMean batch rewritten by with_edge_pools


def prices(n):
    return synth.token_price_vector(n, 7) * synth.sweep_prices(n, seed=8, spread=0.05)


def with_edge_pools(b, v, seed):
    """rows 0 .. 39 of a Product / GeometricMean batch at the no-arbitrage point of v within 1e-3 (equal weights): with the
    0.997 fee they sit inside the band (rows 0 .. 19), with a fee of 1.01 they trade in both directions (rows 20 .. 39)"""
    R, g = b.R.copy(), b.γ.copy()
    S = 100.0 + 900.0 * synth.uniform(seed, 3, EDGE)
    R[:EDGE] = S[:, None] / v[b.Ai[:EDGE] - 1] * np.exp(1e-3 * (2.0 * synth.uniform(seed, 4, 2 * EDGE).reshape(EDGE, 2) - 1.0))
    g[:EDGE // 2], g[EDGE // 2:EDGE] = 0.997, 1.01
    if hasattr(b, "w"):
        w = b.w.copy()
        w[:EDGE] = 0.5
        return batch_with(b, R=R, γ=g, w=w)
    return batch_with(b, R=R, γ=g)


def P(m, n, v, seed=11):
    return with_edge_pools(synth.product_pools(m, n, seed=seed), v, seed)


def G(m, n, v, seed=12):
    return with_edge_pools(synth.geomean_pools(m, n, seed=seed), v, seed)


def U(m, n):
    """two-tick pools (one list tick beyond the current one: threshold heads) and 600 pools of the degenerate-boundary market,
    among them two (its rows 756 and 809) whose tick arithmetic leaves a negative zero or a tiny negative amount at V_U"""
    return cr.PoolBatch.concat([synth.univ3_ragged_pools(m - 600, n, min_ticks=2, max_ticks=2, seed=14),
                                degenerate_univ3(3000, n=n).slice(700, 1300)])


V_U = lambda n: synth.sweep_prices(n, seed=5, spread=0.05)


def swept(batches, n, v, lean, opts, dev):
    """[Ψ, acc, Δ, Λ] of four consecutive sweeps -- fused, materialising, materialising, fused: each in both tile directions --
    and the number of launches that took a lean kernel"""
    be = backend(batches, n, lean_kernels=lean, **opts)
    try:
        out = []
        for materialize in (False, True, True, False):
            if dev:
                psi, acc = dev_sweep(be, v, materialize)
            else:
                psi, acc = be.find_arb(v) if materialize else be.eval(v)
            out += [psi, np.float64(acc)]
            if materialize:
                out += list(be.trades())
        return out, be.ctx.get_option("lean_launches"), be.ctx.segments()
    finally:
        be.close()


def same_bits(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y, equal_nan=True), f"output {k}"
        assert np.array_equal(np.signbit(x), np.signbit(y)), f"output {k}: a zero's sign"


PSI = (0, 2, 6, 10)   # where swept() puts Ψ


def compare(batches, n, v, opts, dev, expect_lean=True, shared_bins=False):
    """shared_bins: the market is so wide that a block keeps ONE bin copy; its wavefronts' LDS adds arrive in any order, so Ψ
    is not reproducible bit for bit from one sweep to the next, with any kernel -- everything else is, and every Ψ must be the
    exact sum of the trade rows within the reduction's own bound (reduction_ref)"""
    lean, count, segs = swept(batches, n, v, 1, opts, dev)
    plain, zero, _ = swept(batches, n, v, 0, opts, dev)
    print(segs, "lean launches:", count)
    if shared_bins:
        Ai0 = np.concatenate([(b.Ai - 1).ravel() for b in batches])
        for out in (lean, plain):
            for k in PSI:
                assert_reduction_exact(out[4].ravel(), out[5].ravel(), Ai0, v, n, out[k], out[k + 1], geometry=segs)
        lean, plain = ([x for k, x in enumerate(out) if k not in PSI] for out in (lean, plain))
    same_bits(lean, plain)
    assert zero == 0
    assert count == (4 if expect_lean else 0)      # one sweep launch per evaluation in every market of this file
    return lean, segs


def check_edges(D, L, batches):
    """the rare paths ran: idle pools and pools trading both ways among the edge rows of every Product / GeometricMean batch"""
    first = 0
    for b in batches:
        if b.kind != cr._lib.KIND_UNIV3:
            d, l = D[first:first + EDGE], L[first:first + EDGE]
            assert np.count_nonzero(~d.any(axis=1) & ~l.any(axis=1)) > 0, "no pool inside the band"
            assert np.count_nonzero((d > 0).all(axis=1)) > 0, "no pool trading both ways"
        first += len(b)


@pytest.mark.parametrize("dev", [False, True], ids=["host_fast", "dev_auto"])
@pytest.mark.parametrize("n", [8, 257])
def test_fused_several_tiles_per_lane(n, dev):
    v = prices(n)
    batches = [P(1500, n, v), G(1500, n, v)]
    out, segs = compare(batches, n, v, {"max_grid": 2}, dev)
    assert [(s["block"], s["grid"]) for s in segs] == [(512, 1), (512, 1)]     # two full tiles and a tail of 476 per lane
    check_edges(out[4], out[5], batches)


@pytest.mark.parametrize("dev", [False, True], ids=["host_fast", "dev_auto"])
def test_fused_xcd_aware_block_map(dev):
    n = 256
    v = prices(n)
    batches = [P(70000, n, v), G(70000, n, v)]
    out, segs = compare(batches, n, v, {"max_grid": 256}, dev)
    assert sum(s["grid"] for s in segs) == 256 and all(s["block"] == 512 for s in segs)
    check_edges(out[4], out[5], batches)


SINGLE = {"product": lambda m, n, v: P(m, n, v), "geomean": lambda m, n, v: G(m, n, v), "univ3": lambda m, n, v: U(m, n)}
# 1024-thread blocks.  2 600 pools under "max_grid" = 1 are ONE block: two full tiles and a tail of 552 -- and a launch of one
# block is a direct launch (abi_sweep.cpp direct_launch: its row is the result, no fold), which the predicate leaves to the
# general kernels.  So the lean kernels run the same shape in two blocks: 5 200 pools under "max_grid" = 2, block 0 with three
# full tiles, block 1 with two and a tail of 80.
BIG_BLOCKS = {"two_blocks": (5200, 2, True), "one_block_direct": (2600, 1, False)}


@pytest.mark.parametrize("dev", [False, True], ids=["host_fast", "dev_auto"])
@pytest.mark.parametrize("geometry", list(BIG_BLOCKS))
@pytest.mark.parametrize("family", list(SINGLE))
def test_single_family_big_blocks(family, geometry, dev):
    n = 48
    m, grid, lean = BIG_BLOCKS[geometry]
    v = V_U(n) if family == "univ3" else prices(n)
    batches = [SINGLE[family](m, n, v)]
    out, segs = compare(batches, n, v, {"block": 1024, "max_grid": grid}, dev, expect_lean=lean)
    assert [(s["block"], s["grid"]) for s in segs] == [(1024, grid)]
    if family == "univ3":
        D, L = out[4], out[5]
        assert np.count_nonzero(np.signbit(D) | np.signbit(L)) > 0, "no negative zero or tiny negative amount"
    else:
        check_edges(out[4], out[5], batches)


@pytest.mark.parametrize("bad", ["nan", "outside"])
@pytest.mark.parametrize("market", ["fused"] + list(SINGLE))
def test_prices_the_fast_arithmetic_does_not_take(market, bad):
    """device pointers: the auto kernel stages such a vector and every block takes its full-range loop"""
    n = 48
    good = prices(n)
    v = good.copy()
    v[5] = np.nan if bad == "nan" else 2.0 ** 160
    if market == "fused":
        out, _ = compare([P(1500, n, good), G(1500, n, good)], n, v, {"max_grid": 2}, True)
    else:
        out, _ = compare([SINGLE[market](5200, n, good)], n, v, {"block": 1024, "max_grid": 2}, True)
    if bad == "nan":
        assert np.isnan(out[0]).any() and np.isnan(out[4]).any()       # the NaN reaches Ψ and the trade rows of its pools


def many_fee_tiers(b):
    """more distinct fees than a launch's fee table holds (256): the segment keeps its plain fee array"""
    g = b.γ.copy()
    g[:300] = 0.99 + 1e-5 * np.arange(300)
    return batch_with(b, γ=g)


def fallbacks():
    n = 48
    v = prices(n)
    fused = lambda: [P(1500, n, v), G(1500, n, v)]
    wide = 5200       # tokens: the {v, 1/v} pairs, log v and one bin copy no longer fit the LDS of a CU
    return {
        "compact_trades_0": (fused, n, v, {"max_grid": 2, "compact_trades": 0}, False),
        "stream_stores_2": (fused, n, v, {"max_grid": 2, "stream_stores": 2}, False),
        "fee_tiers": (lambda: [many_fee_tiers(P(1500, n, v)), G(1500, n, v)], n, v, {"max_grid": 2}, False),
        "prices_without_reciprocals": (lambda: [synth.product_pools(1500, wide, seed=11), synth.geomean_pools(1500, wide, seed=12)],
                                       wide, prices(wide), {"max_grid": 2}, True),
        "direct_small": (lambda: [P(2048, n, v)], n, v, {}, False),
        "ncoin": (lambda: [synth.weighted_pools(700, n, 3, seed=15)], n, v, {}, False),
    }


@pytest.mark.parametrize("name", list(fallbacks()))
def test_fallbacks_launch_the_general_kernels(name):
    make, n, v, opts, shared_bins = fallbacks()[name]
    _, segs = compare(make(), n, v, opts, True, expect_lean=False, shared_bins=shared_bins)
    if name == "direct_small":
        assert [s["grid"] for s in segs] == [1]
