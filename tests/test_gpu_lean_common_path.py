"""The straight-line common path of the lean two-coin kernels (sweep_core.h process_pool_lean; ProductOps / GeoMeanLogOps
lean_solve): a lane whose pool trades in one direction or not at all runs one epilogue without a decoded direction, and a
wavefront with a rare lane -- both directions live, ProductTwoCoin's predicate overlap, a NaN price -- leaves it for the general
solve and epilogue (finish_pool) behind one wave-uniform branch.  What can go wrong is the SPLIT: a rare lane taken for a common
one, a wavefront in which every lane or a single lane is rare, a record or a bin add dropped or doubled on either side, the
adds of a wavefront's lanes to one bin in another order than the general kernel's (which changes the last bit of Ψ: the first
form of the split, rare lanes alone behind the branch, failed here for that reason).  So the rare pools are not in rows
0 .. 39 as in test_gpu_lean_sweep.py but at chosen (tile, block, wavefront, lane) positions.

Every market is swept by a context with "lean_kernels" = 1 and by one with 0 (test_gpu_lean_sweep.compare: four sweeps, fused,
materialising, materialising, fused, so both tile directions), with host pointers and with device pointers; Δ, Λ, Ψ, the dual
value and the signs of zeros must be equal bit for bit, "lean_launches" > 0 in the first context and 0 in the second.

Geometry (launch_plan.cpp): pool i of a segment swept by B blocks of S threads is lane i % S of block (i // S) % B, in that
lane's tile (i // S) // B.
  fused      5 200 ProductTwoCoin + 5 200 GeometricMean under "max_grid" = 2: one 512-thread block per family (a launch of two
             blocks: not direct, so lean) with ten full tiles and a tail tile of 80 lanes;
  alone      each family alone, 5 200 pools in two 1024-thread blocks: block 0 with three full tiles, block 1 with two and a
             tail tile of 80 lanes.
Rare kinds: "band" (fee 0.997 at the no-arbitrage point: no trade), "both" (fee 1.01 there: both directions trade),
"overlap" (ProductTwoCoin with a fee within 1e-12 of 1 at the no-arbitrage point: both predicates hold; for GeometricMean,
which has no margin, a "both" pool)."""
import numpy as np
import pytest

from cfmmrouter_amd import synth
from reduction_ref import assert_reduction_exact
from test_gpu_lean_sweep import PSI, compare, prices
from test_gpu_pool_update import batch_with

pytestmark = pytest.mark.gpu

M = 5200
FEE = {"band": 0.997, "both": 1.01, "overlap": 1.0 - 5e-13}


def placements(S, B, m=M):
    """{row: kind} and the rows by purpose, for a segment of m pools swept by B blocks of S threads"""
    row = lambda tile, block, lane: (tile * B + block) * S + lane
    groups = -(-m // S)
    tail = m - (groups - 1) * S                       # lanes of the tail tile, which is the last tile of block (groups - 1) % B
    assert groups >= 3 * B and 64 < tail < 128        # tiles 0 and 1 are full in every block; the tail's last wavefront is partial
    tiles0 = len(range(0, groups, B))                 # tiles of block 0
    last0 = tiles0 - 2 if (groups - 1) % B == 0 else tiles0 - 1     # the last tile of block 0's lanes >= tail
    where = {
        "first_lane": {row(0, 0, 64): "both"},                                     # alone in its wavefront, as lane 0
        "last_lane": {row(1, B - 1, 191): "overlap"},                              # alone in its wavefront, as lane 63
        "tail_last_lane": {m - 1: "both"},                                         # the last lane of the tail tile
        "whole_wavefront": {row(1, 0, l): "both" for l in range(192, 256)},
        "whole_wavefront_overlap": {row(0, B - 1, l): "overlap" for l in range(320, 384)},
        "idle_wavefront": {row(0, 0, l): "band" for l in range(256, 320)},         # no lane trades
        "last_tile_only": {row(last0, 0, S - 3): "both", row(last0, 0, S - 40): "overlap"},   # the first tile walking back
    }
    rows = {}
    for part in where.values():
        assert not set(part) & set(rows) and max(part) < m
        rows.update(part)
    for r in where["last_tile_only"]:                 # nothing else rare in those lanes
        assert [q for q in rows if q % S == r % S and (q // S) % B == 0] == [r]
    return rows, where


def with_rare_pools(b, v, rows, seed):
    """the batch with the pools `rows` at the no-arbitrage point of v (equal weights) and their kind's fee; "band" pools lie
    within 1e-3 of it, the others exactly on it (up to the rounding of S / v)"""
    idx = np.array(sorted(rows))
    kinds = [rows[r] for r in idx]
    R, g = b.R.copy(), b.γ.copy()
    S = 100.0 + 900.0 * synth.uniform(seed, 3, len(idx))
    off = np.array([1e-3 if k == "band" else 0.0 for k in kinds])[:, None]
    R[idx] = S[:, None] / v[b.Ai[idx] - 1] * np.exp(off * (2.0 * synth.uniform(seed, 4, 2 * len(idx)).reshape(len(idx), 2) - 1.0))
    g[idx] = [FEE[k] for k in kinds]
    if hasattr(b, "w"):
        w = b.w.copy()
        w[idx] = 0.5
        g[idx] = [FEE["both" if k == "overlap" else k] for k in kinds]
        return batch_with(b, R=R, γ=g, w=w)
    return batch_with(b, R=R, γ=g)


def P(n, v, rows, seed=21):
    return with_rare_pools(synth.product_pools(M, n, seed=seed), v, rows, seed)


def G(n, v, rows, seed=22):
    return with_rare_pools(synth.geomean_pools(M, n, seed=seed), v, rows, seed)


def in_overlap(b, v, rows):
    """ProductOps' two predicates, restated: both hold on the "overlap" rows"""
    idx = np.array([r for r, k in rows.items() if k == "overlap"])
    a, c = v[b.Ai[idx, 0] - 1] * b.R[idx, 0], v[b.Ai[idx, 1] - 1] * b.R[idx, 1]
    margin = 1.0 + 1e-12
    return ((b.γ[idx] * c) * margin >= a) & ((b.γ[idx] * a) * margin >= c)


def check_rare_ran(D, L, first, where, product):
    """the trade rows of one segment (it starts at row `first`) show what each placement is for"""
    d = lambda part: D[first + np.array(sorted(where[part]))]
    l = lambda part: L[first + np.array(sorted(where[part]))]
    for part in ("first_lane", "tail_last_lane", "whole_wavefront"):
        assert (d(part) > 0).all() and (l(part) > 0).all(), f"{part}: a pool that does not trade both ways"
    assert not d("idle_wavefront").any() and not l("idle_wavefront").any(), "a pool of the idle wavefront trades"
    assert not np.signbit(d("idle_wavefront")).any() and not np.signbit(l("idle_wavefront")).any(), "-0.0 in an idle record"
    both_last = first + next(r for r, k in where["last_tile_only"].items() if k == "both")
    assert (D[both_last] > 0).all() and (L[both_last] > 0).all(), "last_tile_only: a pool that does not trade both ways"
    if not product:
        assert (d("whole_wavefront_overlap") > 0).all() and (d("last_lane") > 0).all()
    # the neighbours of a single rare lane are ordinary pools: some of them trade, none both ways
    for part in ("first_lane", "last_lane"):
        r = first + next(iter(where[part]))
        wave = np.arange(r - (r - first) % 64, r - (r - first) % 64 + 64)
        others = wave[wave != r]
        assert ((D[others] > 0).sum(axis=1) <= 1).all() and (D[others] > 0).any()


@pytest.mark.parametrize("dev", [False, True], ids=["host_fast", "dev_auto"])
@pytest.mark.parametrize("n", [8, 257])
def test_fused_rare_lanes_by_position(n, dev):
    v = prices(n)
    rows, where = placements(512, 1)
    batches = [P(n, v, rows), G(n, v, rows)]
    assert in_overlap(batches[0], v, rows).all()
    out, segs = compare(batches, n, v, {"max_grid": 2}, dev)
    assert [(s["block"], s["grid"]) for s in segs] == [(512, 1), (512, 1)]
    D, L = out[4], out[5]
    check_rare_ran(D, L, 0, where, True)
    check_rare_ran(D, L, M, where, False)
    if n == 257:
        # Ψ and the dual value of all four sweeps against the exact sums of the trade rows: a rare lane's bin add or dual
        # term dropped or doubled shows here whatever the general kernel does
        Ai0 = np.concatenate([(b.Ai - 1).ravel() for b in batches])
        for k in PSI:
            assert_reduction_exact(D.ravel(), L.ravel(), Ai0, v, n, out[k], out[k + 1], geometry=segs)


FAMILY = {"product": P, "geomean": G}


@pytest.mark.parametrize("dev", [False, True], ids=["host_fast", "dev_auto"])
@pytest.mark.parametrize("n", [8, 257])
@pytest.mark.parametrize("family", list(FAMILY))
def test_single_family_rare_lanes_by_position(family, n, dev):
    v = prices(n)
    rows, where = placements(1024, 2)
    batches = [FAMILY[family](n, v, rows)]
    if family == "product":
        assert in_overlap(batches[0], v, rows).all()
    out, segs = compare(batches, n, v, {"block": 1024, "max_grid": 2}, dev)
    assert [(s["block"], s["grid"]) for s in segs] == [(1024, 2)]
    check_rare_ran(out[4], out[5], 0, where, family == "product")


def bad_prices(n, bad):
    """token 5: few pools of a 257-token market hold it, so the NaN reaches some lanes of a wavefront and not the others"""
    v = prices(n)
    v[5] = np.nan if bad == "nan" else 2.0 ** 160
    return v


@pytest.mark.parametrize("bad", ["nan", "outside"])
@pytest.mark.parametrize("market", ["fused", "product", "geomean"])
def test_prices_outside_the_window_device_pointers(market, bad):
    """the auto kernels stage such a vector and every block takes its full-range loop: the same split on the compiler's
    arithmetic, and with a NaN price the lanes that hold token 5 are rare"""
    n = 257
    good, v = prices(n), bad_prices(n, bad)
    if market == "fused":
        rows, _ = placements(512, 1)
        batches, opts = [P(n, good, rows), G(n, good, rows)], {"max_grid": 2}
    else:
        rows, _ = placements(1024, 2)
        batches, opts = [FAMILY[market](n, good, rows)], {"block": 1024, "max_grid": 2}
    out, _ = compare(batches, n, v, opts, True)
    if bad == "nan":
        D = out[4]
        hit = np.concatenate([(b.Ai == 6).any(axis=1) for b in batches])
        assert hit.any() and not hit.all()
        assert np.isnan(D[hit]).any(axis=1).all() and not np.isnan(D[~hit]).any()
        waves = hit[:M - M % 64].reshape(-1, 64)
        assert (waves.any(axis=1) & ~waves.all(axis=1)).any(), "no wavefront with only some lanes on the NaN token"
        assert np.isnan(out[0]).any()


def test_price_outside_the_window_host_pointers():
    """host pointers: the library sees the prices and launches the general kernels on the full-range arithmetic (a NaN price
    it refuses: the reference's ArgumentError)"""
    n = 257
    rows, _ = placements(512, 1)
    good = prices(n)
    compare([P(n, good, rows), G(n, good, rows)], n, bad_prices(n, "outside"), {"max_grid": 2}, False, expect_lean=False)
