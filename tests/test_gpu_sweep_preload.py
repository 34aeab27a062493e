"""The sweep's entry with preloaded arguments and prices first (sweep.h SweepLaunch / SweepTail; sweep_core.h request_prices,
stage_prices; csrc/Makefile KFLAGS).

Every sweep kernel takes the descriptor, the prices, the direction and n as leading arguments, handed over in SGPRs, and each
lane requests its first two prices from them at the kernel's first instructions.  What can go wrong: an argument lands in
another parameter's place, a price is staged from the wrong index, or a pre-armed launch uses a price it requested before the
host had written it.  So, on small markets:
  - fused launches of two, three and four families -- with a segment of 3 pools, with idle blocks, and a 2 x 128-block launch
    under the XCD-aware map (65 025 pools: that launch needs 128 tiles of 512, there is no smaller market that has it) --, and
    one segment's own launch of 1, 513 and 2049 pools: fused and materialising, host and device pointers, both tile
    directions.  The trade rows equal, bit for bit, those of the same market swept one segment per launch ("fuse_segments" =
    0), Product and UniV3 rows are the CPU oracle's, and {Ψ, acc} are the sums of the rows within the bounds of reduction_ref;
  - markets of 2, 64, 513 and 1025 tokens at both block sizes: a lane stages no price, one, two (both requested at the
    kernel's first instructions) or three (the third loaded by stage_prices).  2 is the smallest market there is: the two
    coins of a pool are distinct tokens, and the library refuses a pool of a one-token market;
  - a pre-armed evaluation (cfmm_route) ends bit-identical to the unarmed one, at trades a per-segment sweep reproduces;
  - staleness: after cfmm_pools_set_ticks has swapped a UniV3 segment's arrays, after a call that allocates scratch
    (cfmm_select_trades), and after cfmm_set_stream, the next sweep equals a fresh context's."""
import numpy as np
import pytest
import torch

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import OBJ_LINEAR_NONNEGATIVE
from test_gpu_pool_ticks import changed, set_ticks, with_ladders
from test_gpu_pool_update import batch_with, rows_of
from test_gpu_sweep_entry import (B2, G, N, P, U, V, assert_equals_fresh, assert_same, backend, check_against_the_rows, outputs,
                                  outputs0, rows, swept)

pytestmark = pytest.mark.gpu


def prices(n):
    return V if n == N else synth.token_price_vector(n, 7) * synth.sweep_prices(n, seed=8, spread=0.05)


def check_market(n, batches, opts, grid=None):
    v = prices(n)
    be = backend(batches, n, **opts)
    per_seg = backend(batches, n, fuse_segments=0, **opts)
    try:
        segs = be.ctx.segments()
        print(segs)
        if grid is not None:
            assert sum(s["grid"] for s in segs) == grid and all(s["block"] == 512 for s in segs)
        k = 4 + 2 * len(batches)
        first = outputs(be, batches, v)           # fused / materialising, host / device pointers: sweeps 0 .. 3
        be.eval(v)                                # one more: the same four calls now run in the other tile direction
        second = outputs(be, batches, v)
        want = outputs(per_seg, batches, v)
        for out in (first, second):
            check_against_the_rows(be, batches, v, n, out[2], out[3], out[4:k])
            check_against_the_rows(be, batches, v, n, out[k + 2], out[k + 3], out[k + 4:])
            assert_same(out[4:k], want[4:k])      # trades: one launch of all families = one launch per family
            assert_same(out[k + 4:], want[k + 4:])
    finally:
        per_seg.close()
        be.close()


MARKETS = {
    # fused: a segment of 3 pools whose three blocks are idle but one; three families; four, two of them one family
    "fused_2_seg_of_3": (N, lambda: [P(1500), G(3)], {}, 6),
    "fused_3": (N, lambda: [P(700), G(1300), B2(513)], {}, 9),
    "fused_4": (N, lambda: [P(3), G(1100), U(900), P(513, seed=21)], {}, 12),
    # 128 tiles of 512 in the larger segment: "max_grid" = 256 gives 2 x 128 blocks, a multiple of 256 -- the XCD-aware map,
    # which leaves most of the small segment's blocks idle (the smallest market that has this launch)
    "fused_xcd_2x128": (N, lambda: [P(65025), G(1500)], {"max_grid": 256}, 256),
    # one segment's own launch: the single-block direct path (1024 threads), and 512-thread blocks with a fold
    "one_1": (N, lambda: [P(1)], {}, None),
    "one_513": (N, lambda: [U(513)], {}, None),
    "one_2049": (N, lambda: [G(2049)], {}, None),
}


@pytest.mark.parametrize("name", list(MARKETS))
def test_fused_equals_one_launch_per_segment(name):
    n, make, opts, grid = MARKETS[name]
    check_market(n, make(), opts, grid)


@pytest.mark.parametrize("n", [2, 64, 513, 1025])
@pytest.mark.parametrize("block", [512, 1024])
def test_token_counts_at_both_block_sizes(n, block):
    """lane t stages the prices t, t + block, ... < n: none, one or several"""
    check_market(n, [P(1500, n=n), G(700, n=n)], {"block": block})
    check_market(n, [P(513, n=n)], {"block": block} if block == 512 else {})   # (the single-block direct launch has 1024 threads)


def test_a_one_token_market_has_no_pools():
    """why the token counts above start at 2"""
    p = P(4, n=2)
    with pytest.raises(cr.ArgumentError):
        backend([batch_with(p, Ai=np.ones_like(p.Ai))], 1)


def test_route_armed_fused_three_families():
    n = 64
    batches = [P(700, n=n), G(300, n=n), B2(513, n=n)]
    c = synth.linear_prices(n, seed=3)
    got = []
    for armed in (1, 0):
        be = backend(batches, n, armed=armed)
        try:
            v, psi, info = be.ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(n))
            got.append([v, psi, np.int64(info["evaluations"])] + rows(be, batches))
        finally:
            be.close()
    assert got[0][2] >= 3
    assert_same(got[0], got[1])
    per_seg = backend(batches, n, fuse_segments=0)
    try:
        per_seg.find_arb(got[0][0])
        assert_same(got[0][3:], rows(per_seg, batches))
    finally:
        per_seg.close()


# ---- staleness: the descriptors are on the device, then something they name changes -------------------------------------------------

THREE = lambda: [P(700), G(300), U(1500)]


def test_sweep_after_set_ticks_swapped_the_univ3_arrays():
    old = THREE()
    be = swept(old)
    try:
        idx = rows_of(1500, 200, 6)
        states = [changed(old[2], int(i), "longer", k)[1:] for k, i in enumerate(idx)]
        set_ticks(be.ctx, 2, idx, states)
        assert be.ctx.get_option("pool_update_regrows") >= 1
        assert_equals_fresh(be, [old[0], old[1], with_ladders(old[2], idx, states)])
    finally:
        be.close()


def test_sweep_after_a_call_that_allocates_scratch():
    batches = THREE()
    be = swept(batches)
    try:
        idx, D, L, value = be.ctx.select_trades(0, 0.0)       # first call: allocates the selection's device scratch
        assert len(idx) > 0
        assert_equals_fresh(be, batches)
    finally:
        be.close()


def test_sweep_after_set_stream():
    batches = THREE()
    be = swept(batches)
    stream = torch.cuda.Stream()
    try:
        be.ctx.set_stream(stream.cuda_stream)
        assert_equals_fresh(be, batches)
        be.ctx.reset_stream()
        assert_equals_fresh(be, batches)
    finally:
        be.close()
