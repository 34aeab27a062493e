"""The sweep kernels' entry: per-launch arguments of one line + the launch-invariant descriptor in device memory (sweep.h
SweepLaunch / SweepDesc; csrc/launch_plan.cpp build_sweep_desc; abi_sweep.cpp ensure_desc).

Two things can go wrong and both are checked bit for bit.  (1) The block table: a block sweeps other pools than before, or
writes another row -- every shape below is swept fused and materialising, through host pointers (the fast kernels) and through
device pointers (the kernels that carry both arithmetics: what bench.py times), twice in a row so that both tile directions
run; Ψ and the dual value must be the exact sums of the trade rows (reduction_ref), Product and UniV3 rows must be the CPU
oracle's, and a second context must return the same bits.  (2) Staleness: a context that has swept once -- its descriptors are
on the device -- is changed, and its next sweep must equal that of a context built from the final state.

48 tokens: every wavefront owns its bins, so the sums are reproducible."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_PRODUCT, KIND_UNIV3, OBJ_LINEAR_NONNEGATIVE
from helpers import dev_sweep, oracle_sweep
from reduction_ref import assert_reduction_exact
from test_gpu_pool_ticks import changed, set_ticks, with_ladders
from test_gpu_pool_update import batch_with, new_state, rows_of

pytestmark = pytest.mark.gpu

N = 48
V = synth.token_price_vector(N, 7) * synth.sweep_prices(N, seed=8, spread=0.05)

P = lambda m, seed=11, n=N: synth.product_pools(m, n, seed=seed)
G = lambda m, seed=12, n=N: synth.geomean_pools(m, n, seed=seed)
B2 = lambda m, seed=13, n=N: synth.bounded_product_pools(m, n, seed=seed)
U = lambda m, seed=14, n=N: synth.univ3_ragged_pools(m, n, min_ticks=1, max_ticks=12, seed=seed)
W3 = lambda m, seed=15, n=N: synth.weighted_pools(m, n, 3, seed=seed)


def backend(batches, n=N, **opts):
    be = cr.DeviceBackend(n, batches)
    for k, x in opts.items():
        be.ctx.set_option(k, x)
    return be


def rows(be, batches):
    out = []
    for s, b in enumerate(batches):
        out += list(be.ctx.trades_range(s, 0, len(b), b.Ai.shape[1]))
    return out


def outputs(be, batches, v):
    """fused and materialising, host-pointer and device-pointer: [Ψ, acc, ...] and the trade rows of every segment"""
    psi_e, acc_e = be.eval(v)
    psi, acc = be.find_arb(v)
    out = [psi_e, np.float64(acc_e), psi, np.float64(acc)] + rows(be, batches)
    psi_d, acc_d = dev_sweep(be, v, False)
    psi_m, acc_m = dev_sweep(be, v, True)
    return out + [psi_d, np.float64(acc_d), psi_m, np.float64(acc_m)] + rows(be, batches)


def assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"output {k}")


def check_against_the_rows(be, batches, v, n, psi, acc, got):
    """Ψ / acc of a materialising sweep = the exact sums of its own rows `got`; Product and UniV3 rows = the oracle's"""
    D = np.concatenate([got[2 * s].ravel() for s in range(len(batches))])
    L = np.concatenate([got[2 * s + 1].ravel() for s in range(len(batches))])
    Ai0 = np.concatenate([(b.Ai - 1).ravel() for b in batches])
    assert_reduction_exact(D, L, Ai0, v, n, psi, acc, geometry=be.ctx.segments())
    for s, b in enumerate(batches):
        if b.kind in (KIND_PRODUCT, KIND_UNIV3):
            Do, Lo, _, _ = oracle_sweep([b], n, v)
            np.testing.assert_array_equal(got[2 * s], Do.reshape(-1, 2), err_msg=f"segment {s} Δ")
            np.testing.assert_array_equal(got[2 * s + 1], Lo.reshape(-1, 2), err_msg=f"segment {s} Λ")


SHAPES = {
    # one segment, the single-block direct path: one pool, a partial tile, one full tile + 1, two full tiles
    "one_1": (N, lambda: [P(1)], {}),
    "one_511": (N, lambda: [P(511)], {}),
    "one_513": (N, lambda: [U(513)], {}),
    "one_2048": (N, lambda: [P(2048)], {}),
    # 512-thread blocks, uneven tails
    "one_2049": (N, lambda: [G(2049)], {}),
    "one_70001": (N, lambda: [P(70001)], {}),
    # 1024-thread blocks: 137 of them, one tile per lane (the default geometry at this size), and -- "max_grid" = 32 -- several
    # tiles per lane, four or five
    "product_140000": (N, lambda: [P(140000)], {}),
    "product_140000_tiles": (N, lambda: [P(140000)], {"max_grid": 32}),
    # fused launches: the map without xcd_map, and the XCD-aware one
    "fused_1500": (N, lambda: [P(1500), G(1500)], {}),
    "fused_65600": (N, lambda: [P(65600), G(65600)], {"max_grid": 256}),
    "fused_three": (N, lambda: [P(5000), G(3), B2(1777)], {}),
    "fused_four": (N, lambda: [P(3), G(4099), U(2500), P(513, seed=21)], {}),
    "ncoin_between": (N, lambda: [P(3000), G(2000), W3(700), P(1000, seed=22), B2(900)], {}),
    # large-market mode
    "gbins_3000": (8200, lambda: [P(3000, n=8200)], {}),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_both_directions_both_variants(name):
    n, make, opts = SHAPES[name]
    batches = make()
    v = V if n == N else synth.token_price_vector(n, 7) * synth.sweep_prices(n, seed=8, spread=0.05)
    be = backend(batches, n, **opts)
    try:
        segs = be.ctx.segments()
        print(name, segs)
        if name.startswith("one_") and len(batches[0]) <= 2048:
            assert [s["grid"] for s in segs] == [1]
        if name.startswith("product_140000"):
            assert segs[0]["block"] == 1024 and segs[0]["grid"] == (32 if opts else 137)
        if name == "fused_65600":    # 129 tiles each in 128 blocks each: the XCD-aware map needs a multiple of 256 blocks
            assert sum(s["grid"] for s in segs) == 256 and all(s["block"] == 512 for s in segs)
        k = 4 + 2 * len(batches)
        first = outputs(be, batches, v)          # sweeps 0 .. 3
        be.eval(v)                               # one more: the same four calls now run in the other tile direction
        second = outputs(be, batches, v)
        for out in (first, second):
            check_against_the_rows(be, batches, v, n, out[2], out[3], out[4:k])                  # host pointers
            check_against_the_rows(be, batches, v, n, out[k + 2], out[k + 3], out[k + 4:])       # device pointers
        fresh = backend(batches, n, **opts)
        try:
            assert_same(first, outputs(fresh, batches, v))
            fresh.eval(v)
            assert_same(second, outputs(fresh, batches, v))
        finally:
            fresh.close()
        # the trade rows do not depend on the direction, nor on who asked
        assert_same(first[4:k], second[4:k])
        assert_same(first[4:k], first[k + 4:])
        if name == "fused_65600":
            # the XCD-aware map is ON for this launch: only that map divides a fused launch's blocks by cost (plan_xcd_map; the
            # map b % nseg gives every segment grid / nseg), so a fourfold GeometricMean cost must move the 128 + 128 split
            be.ctx.set_option("cost_geomean", 40)
            be.eval(v)
            grids = [s["grid"] for s in be.ctx.segments()]
            print(name, "cost_geomean = 40:", grids)
            assert sum(grids) == 256 and grids[0] % 8 == 0 and grids[0] < 128 < grids[1]
    finally:
        be.close()


# ---- staleness: the descriptors are on the device, then something they copy changes ------------------------------------------

def outputs0(be, batches, v=V):
    psi_e, acc_e = be.eval(v)
    psi, acc = be.find_arb(v)
    return [psi_e, np.float64(acc_e), psi, np.float64(acc)] + rows(be, batches)


def assert_equals_fresh(be, batches, n=N, **opts):
    """`be` against a context built from `batches` with the options set before its first sweep"""
    fresh = backend(batches, n, alternate=0, **opts)
    try:
        assert_same(outputs0(be, batches), outputs0(fresh, batches))
    finally:
        fresh.close()


def swept(batches, **opts):
    be = backend(batches, N, alternate=0, **opts)
    outputs0(be, batches)
    return be


def test_sparse_reserve_update():
    old = [P(1500), G(1500)]
    be = swept(old)
    try:
        idx = rows_of(1500, 37, 5)
        new = new_state(old[0], 101)
        be.ctx.set_reserves(0, idx, new.R[idx])
        R = old[0].R.copy()
        R[idx] = new.R[idx]
        assert_equals_fresh(be, [batch_with(old[0], R=R), old[1]])
    finally:
        be.close()


def test_fee_update():
    old = [P(1500), G(1500)]
    be = swept(old)
    try:
        g = old[0].γ.copy()
        g[::3] = 0.9925                                   # a fee tier the launch's table did not hold
        now = [batch_with(old[0], γ=g), old[1]]
        be.reload(now)
        assert_equals_fresh(be, now)
    finally:
        be.close()


def test_set_ticks_forcing_a_compaction():
    old = [P(1500), U(3000)]
    be = swept(old)
    try:
        idx = rows_of(3000, 400, 6)
        states = [changed(old[1], int(i), "longer", k)[1:] for k, i in enumerate(idx)]
        set_ticks(be.ctx, 1, idx, states)
        assert be.ctx.get_option("pool_update_regrows") >= 1
        assert_equals_fresh(be, [old[0], with_ladders(old[1], idx, states)])
    finally:
        be.close()


def test_added_pools_in_a_new_segment():
    p, g = P(1500), G(1500)
    be = swept([p])                                       # one block, direct
    try:
        be.ctx.add_geomean(g.R, g.w, g.γ, (g.Ai - 1).astype(np.int32))
        assert_equals_fresh(be, [p, g])                   # now a fused launch and a fold
    finally:
        be.close()


SMALL = lambda: [P(5000), G(3000), U(1777)]
BIG = lambda: [P(65600), G(65600)]
OPTION_FLIPS = [("pack", 0, SMALL, {}), ("compact_trades", 0, SMALL, {}), ("block", 1024, SMALL, {}), ("max_grid", 6, SMALL, {}),
                ("fuse_segments", 0, SMALL, {}), ("bin_copies", 1, SMALL, {}), ("stream_stores", 2, SMALL, {}),
                ("univ3_heads", 0, SMALL, {}), ("geomean_exact", 1, SMALL, {}),
                ("cost_geomean", 40, BIG, {"max_grid": 256}), ("cost_univ3", 40, lambda: [P(65600), B2(65600)], {"max_grid": 256})]


@pytest.mark.parametrize("option,value,make,opts", OPTION_FLIPS, ids=[o[0] for o in OPTION_FLIPS])
def test_an_option_flipped_after_the_first_sweep(option, value, make, opts):
    batches = make()
    be = swept(batches, **opts)
    try:
        assert be.ctx.get_option(option) != value
        be.ctx.set_option(option, value)
        if option == "bin_copies":
            # one shared copy: the LDS adds of a block's wavefronts arrive in any order, so Ψ is no longer reproducible bit for
            # bit -- the rows are, and Ψ / acc must still be the exact sums of the rows within the reduction's own bound
            fresh = backend(batches, N, alternate=0, **{option: value}, **opts)
            a = outputs0(be, batches)
            try:
                assert_same(a[4:], outputs0(fresh, batches)[4:])
            finally:
                fresh.close()
            check_against_the_rows(be, batches, V, N, a[2], a[3], a[4:])
        else:
            assert_equals_fresh(be, batches, **{option: value}, **opts)
    finally:
        be.close()


def test_set_peers_with_a_world_of_one():
    batches = [P(513)]
    be = swept(batches)                                   # one block, direct: no fold
    ptrs = []

    def shard(b):
        p, _ = b.ctx.peer_buffer_alloc()
        ptrs.append((b, p))
        b.ctx.set_peers([p], 1, 0, 0)

    try:
        shard(be)                                         # a sharded context folds
        fresh = backend(batches, N, alternate=0)
        try:
            shard(fresh)
            assert_same(outputs0(be, batches), outputs0(fresh, batches))
            be.ctx.set_peers([], 0, 0, 0)                 # and back
            fresh.ctx.set_peers([], 0, 0, 0)
            plain = backend(batches, N, alternate=0)
            try:
                assert_same(outputs0(be, batches), outputs0(plain, batches))
            finally:
                plain.close()
        finally:
            for b, p in ptrs:
                b.ctx.peer_buffer_free(p)
            fresh.close()
    finally:
        be.close()


def test_route_armed_and_unarmed_end_bit_identical():
    batches = [P(1500), G(1500)]
    c = synth.linear_prices(N, seed=3)
    got = []
    for armed in (1, 0):
        be = backend(batches, N, armed=armed)
        try:
            v, psi, info = be.ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N))
            got.append([v, psi, np.int64(info["evaluations"])] + rows(be, batches))
        finally:
            be.close()
    assert got[0][2] >= 3
    assert_same(got[0], got[1])
