"""Sparse pool-state updates on the device (cfmm_pools_set_reserves / _set_curve / _set_prices, update_pools_).

The rule throughout: context A is built with the old state and updated, context B is built fresh with the new state, and
every output of A equals B's BIT FOR BIT (the prepared constants come from the upload's own host code).  Tile order
alternates with the sweep count, so both contexts run with option "alternate" = 0; at 48 tokens every wavefront owns its
bins, so the sums are reproducible.  3 000 pools per segment: above 2 048, the two-launch path with a fold."""
import os
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_CURVE, KIND_SOLIDLY, KIND_UNIV3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 48, 3000
V = synth.sweep_prices(N, seed=7, spread=0.3)
V2 = synth.sweep_prices(N, seed=8, spread=0.3)


def ragged(m, seed, n=N):
    return synth.univ3_ragged_pools(m, n, min_ticks=2, max_ticks=12, seed=seed)


def batch_with(b, **fields):
    a = {f: getattr(b, f) for f in ("R", "w", "γ", "Ai", "α", "β", "current_price", "tick_off", "lower_ticks", "liquidity") if hasattr(b, f)}
    a.update(fields)
    return cr.PoolBatch(b.kind, **{k: np.array(x, copy=True) for k, x in a.items()})


def moved_prices(b, seed):
    """a new price per pool, anywhere inside its ladder (any tick, empty ones included), never above the first tick"""
    u, w = synth.uniform(seed, 1, len(b)), synth.uniform(seed, 2, len(b))
    nt = np.diff(b.tick_off)
    j = np.minimum((u * nt).astype(np.int64), nt - 1)
    hi = b.lower_ticks[b.tick_off[:-1] + j]
    lo = np.where(j + 1 < nt, b.lower_ticks[np.minimum(b.tick_off[:-1] + j + 1, b.lower_ticks.size - 1)], 0.5 * hi)
    return lo + (hi - lo) * (0.02 + 0.96 * w)


def new_state(b, seed):
    """-> the batch with every pool in a new state (same tokens, fees, weights, ladders)"""
    if b.kind == KIND_UNIV3:
        return batch_with(b, current_price=moved_prices(b, seed))
    if b.kind == KIND_CURVE:
        o = synth.curve_pools(len(b), N, b.n_coins, seed=seed)
        return batch_with(b, R=o.R, α=o.α, β=o.β)
    if b.kind == KIND_SOLIDLY:
        return batch_with(b, R=synth.solidly_pools(len(b), N, seed=seed).R)
    f = np.exp(synth.uniform(seed, 3, b.R.size).reshape(b.R.shape) - 0.5)
    return batch_with(b, R=b.R * f)


def rows_of(m, K, seed):
    return np.argsort(synth.uniform(seed, 4, m))[:K].astype(np.int64)     # K distinct rows, in no particular order


def apply(ctx, seg, old, new, rows):
    """rows of `new` into segment seg of ctx -> the batch the context now holds"""
    if old.kind == KIND_UNIV3:
        ctx.set_prices(seg, rows, new.current_price[rows])
        p = old.current_price.copy()
        p[rows] = new.current_price[rows]
        return batch_with(old, current_price=p)
    R = old.R.copy()
    R[rows] = new.R[rows]
    if old.kind == KIND_CURVE:
        ctx.set_curve(seg, rows, new.R[rows], new.α[rows], new.β[rows])
        al, be = old.α.copy(), old.β.copy()
        al[rows], be[rows] = new.α[rows], new.β[rows]
        return batch_with(old, R=R, α=al, β=be)
    ctx.set_reserves(seg, rows, new.R[rows])
    return batch_with(old, R=R)


def backend(batches, n=N, device=0):
    be = cr.DeviceBackend(n, batches, device=device)
    be.ctx.set_option("alternate", 0)
    return be


def outputs(be, batches, v=V):
    psi_e, acc_e = be.eval(v)
    psi, acc = be.find_arb(v)
    D, L = be.trades()
    state = [be.ctx.prices(s, len(b)) if b.kind == KIND_UNIV3 else be.ctx.reserves(s, len(b), b.Ai.shape[1])
             for s, b in enumerate(batches)]
    return [psi_e, np.float64(acc_e), psi, np.float64(acc), np.asarray(D), np.asarray(L)] + state


def assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"output {k}")


def assert_equals_fresh(be, batches, n=N, device=0, v=V):
    fresh = backend(batches, n, device)
    try:
        assert_same(outputs(be, batches, v), outputs(fresh, batches, v))
    finally:
        fresh.close()


KINDS = {
    "product": lambda m: synth.product_pools(m, N, seed=11),
    "geomean": lambda m: synth.geomean_pools(m, N, seed=12),
    "solidly": lambda m: synth.solidly_pools(m, N, seed=13),
    "weighted3": lambda m: synth.weighted_pools(m, N, 3, seed=14),
    "weighted8": lambda m: synth.weighted_pools(m, N, 8, seed=15),
    "curve2": lambda m: synth.curve_pools(m, N, 2, seed=16),
    "curve4": lambda m: synth.curve_pools(m, N, 4, seed=17),
    "univ3": lambda m: ragged(m, 18),
}


@pytest.mark.parametrize("K", [1, 37, M])
@pytest.mark.parametrize("kind", list(KINDS))
def test_updated_context_equals_fresh_per_kind(kind, K):
    old = KINDS[kind](M)
    new = new_state(old, 100 + K)
    if kind.startswith("curve"):
        assert (old.α == 0).any() and (new.α == 0).any()
    if kind == "univ3":
        assert np.diff(old.tick_off).min() == 2 and np.diff(old.tick_off).max() == 12 and (old.liquidity == 0).any()
    be = backend([old])
    try:
        be.find_arb(V)                                   # the update is enqueued behind an earlier sweep
        now = apply(be.ctx, 0, old, new, rows_of(M, K, 5))
        assert_equals_fresh(be, [now])
    finally:
        be.close()


def test_mixed_market_untouched_segments_keep_their_bits():
    olds = [synth.product_pools(M, N, seed=21), synth.geomean_pools(M, N, seed=22), ragged(M, 23),
            synth.solidly_pools(M, N, seed=24), synth.weighted_pools(M, N, 3, seed=25)]
    be = backend(olds)
    try:
        be.find_arb(V)
        before = [be.ctx.trades_range(s, 0, M, b.Ai.shape[1]) for s, b in enumerate(olds)]
        now = list(olds)
        now[1] = apply(be.ctx, 1, olds[1], new_state(olds[1], 31), rows_of(M, 500, 6))
        now[4] = apply(be.ctx, 4, olds[4], new_state(olds[4], 32), rows_of(M, 37, 7))
        be.find_arb(V)
        for s in (0, 2, 3):
            assert_same(be.ctx.trades_range(s, 0, M, olds[s].Ai.shape[1]), before[s])
        assert not np.array_equal(be.ctx.trades_range(1, 0, M)[0], before[1][0])
        assert_equals_fresh(be, now)
    finally:
        be.close()


def test_univ3_tick_crossings():
    lt, liq = [30.0, 20.0, 10.0, 5.0, 2.0], [1e6, 2e6, 0.0, 1.5e6, 1e6]       # tick 3, (5, 10], is empty
    m = 6
    pools = [cr.UniV3(15.0, lt, liq, 0.997, [1 + k, 2 + k]) for k in range(m - 1)] + [cr.UniV3(3.0, [8.0], [1e6], 1.0, [7, 8])]
    old = cr.PoolBatch.from_pools(KIND_UNIV3, pools)
    v = synth.sweep_prices(N, seed=41, spread=1.5)
    be = backend([old])
    try:
        # rows 0..4: another non-empty tick, into the empty tick, the exact first-tick bound, within the tick, the last tick; 5: single tick
        steps = [[25.0, 7.0, 30.0, 17.0, 1.0, 5.0],
                 [15.0, 3.0, 20.0, 17.5, 7.0, 8.0]]    # back, OUT of the empty tick, a tick boundary, same tick, into the empty tick, the bound
        now = old
        for p in steps:
            be.ctx.set_prices(0, np.arange(m), p)
            now = batch_with(now, current_price=np.array(p))
            np.testing.assert_array_equal(be.ctx.prices(0, m), p)
            assert_equals_fresh(be, [now], v=v)
    finally:
        be.close()


def test_univ3_tail_growth_and_compaction():
    old = ragged(M, 51)
    be = backend([old])
    try:
        assert be.ctx.get_option("pool_update_regrows") == 0
        now = old
        for r in range(5):
            now = apply(be.ctx, 0, now, new_state(now, 60 + r), rows_of(M, M // 2, 70 + r))
            be.eval(V)
        regrows = be.ctx.get_option("pool_update_regrows")
        print("pool_update_regrows after 5 rounds of m/2 price moves:", regrows)
        assert regrows >= 1
        assert_equals_fresh(be, [now])
    finally:
        be.close()


@pytest.mark.parametrize("kind", ["product", "univ3", "curve4"])
def test_small_market_on_the_single_block_path(kind):
    old = KINDS[kind](400)
    be = backend([old])
    try:
        if kind != "curve4":                           # (N-coin kinds are never single-block direct)
            assert be.ctx.segments()[0]["grid"] == 1
        now = apply(be.ctx, 0, old, new_state(old, 81), rows_of(400, 37, 8))
        assert_equals_fresh(be, [now])
    finally:
        be.close()


def test_large_market_mode_with_a_hub_token():
    n = 8193
    def hub(b):
        Ai = b.Ai.copy()
        Ai[::3, 0] = 1                                  # every third pool trades the hub token
        Ai[:, 1] = np.where(Ai[:, 1] == Ai[:, 0], 2, Ai[:, 1])
        return batch_with(b, Ai=Ai)
    olds = [hub(synth.product_pools(M, n, seed=91)), hub(synth.solidly_pools(M, n, seed=92))]
    v = synth.sweep_prices(n, seed=93, spread=0.3)
    be = backend(olds, n)
    try:
        be.find_arb(v)
        now = [apply(be.ctx, 0, olds[0], new_state(olds[0], 94), rows_of(M, 37, 9)),
               apply(be.ctx, 1, olds[1], batch_with(olds[1], R=synth.solidly_pools(M, n, seed=95).R), rows_of(M, 300, 10))]
        assert_equals_fresh(be, now, n, v=v)
    finally:
        be.close()


def test_multi_device_parent_rows_straddle_the_shards():
    olds = [synth.product_pools(M, N, seed=101), ragged(M, 102), synth.curve_pools(M, N, 4, seed=103)]
    be = backend(olds, device=[0, 0])
    try:
        rows = np.array([M // 2 + 1, 3, M // 2 - 1, M - 1, M // 2, 0], dtype=np.int64)    # shard boundary at M/2
        now = [apply(be.ctx, s, b, new_state(b, 110 + s), rows) for s, b in enumerate(olds)]
        assert_equals_fresh(be, now, device=[0, 0])
        single = backend(now)          # a single-device context: the same trades and state (its Ψ is summed in another order)
        try:
            assert_same(outputs(be, now)[4:], outputs(single, now)[4:])
        finally:
            single.close()
    finally:
        be.close()


def test_values_outside_the_fast_window():
    olds = [synth.product_pools(M, N, seed=121), ragged(M, 122)]
    be = backend(olds)
    try:
        R = olds[0].R.copy()
        R[1234, 0] = 2.0 ** 200
        p = olds[1].current_price.copy()
        p[77] = 2.0 ** -200                                                              # deep in the last tick (it reaches price 0)
        be.ctx.set_reserves(0, [1234], R[1234:1235])
        be.ctx.set_prices(1, [77], p[77:78])
        now = [batch_with(olds[0], R=R), batch_with(olds[1], current_price=p)]
        assert_equals_fresh(be, now)                                                     # (a fresh upload runs full-range too)
        # back inside the window: the segment stays on the full-range arithmetic, whose bits are the fast one's
        now = [apply(be.ctx, 0, now[0], olds[0], np.array([1234])), apply(be.ctx, 1, now[1], olds[1], np.array([77]))]
        assert_equals_fresh(be, now)
    finally:
        be.close()


def test_sequencing_route_update_reserves_and_stale_trades():
    olds = [synth.product_pools(M, N, seed=131), ragged(M, 132), synth.weighted_pools(M, N, 3, seed=133)]
    news = [new_state(b, 140 + k) for k, b in enumerate(olds)]
    picks = [rows_of(M, 200, 150 + k) for k in range(3)]
    offs = np.cumsum([0] + [len(b) for b in olds])
    changes, want = {}, []
    for k, (o, nw, rows) in enumerate(zip(olds, news, picks)):
        if o.kind == KIND_UNIV3:
            p = o.current_price.copy()
            p[rows] = nw.current_price[rows]
            want.append(batch_with(o, current_price=p))
            changes.update({int(offs[k] + i): float(nw.current_price[i]) for i in rows})
        else:
            R = o.R.copy()
            R[rows] = nw.R[rows]
            want.append(batch_with(o, R=R))
            changes.update({int(offs[k] + i): nw.R[i] for i in rows})
    obj = cr.LinearNonnegative(synth.linear_prices(N, seed=134))
    ra = cr.Router(obj, [batch_with(b) for b in olds], N)
    rb = cr.Router(obj, want, N)
    try:
        cr.find_arb_(ra, V)
        cr.update_pools_(ra, changes)
        for a, b in zip(ra._batches, want):                                             # the host mirror followed
            np.testing.assert_array_equal(a.current_price if a.kind == KIND_UNIV3 else a.R, b.current_price if b.kind == KIND_UNIV3 else b.R)
        with pytest.raises(RuntimeError, match="no materialised trades"):
            ra._backend.ctx.trades()
        assert not np.any(np.concatenate([np.ravel(d) for d in ra.Δs]))
        cr.find_arb_(rb, V)                                                             # (the same number of sweeps on both)
        cr.route_(ra, v=np.ones(N), solver="native")
        cr.route_(rb, v=np.ones(N), solver="native")
        np.testing.assert_array_equal(ra.v, rb.v)
        np.testing.assert_array_equal(cr.netflows(ra), cr.netflows(rb))
        for a, b in zip(ra.Δs, rb.Δs):
            np.testing.assert_array_equal(a, b)
        # set_prices -> find_arb -> update_reserves!: the UniV3 host copies moved with the update
        for r in (ra, rb):
            cr.find_arb_(r, V2)
            cr.update_reserves_(r)
        for a, b in zip(ra._batches, rb._batches):
            np.testing.assert_array_equal(a.current_price if a.kind == KIND_UNIV3 else a.R, b.current_price if b.kind == KIND_UNIV3 else b.R)
        assert_same(ra._backend.eval(V), rb._backend.eval(V))
    finally:
        ra.close()
        rb.close()


@pytest.mark.parametrize("device", [0, [0, 0]])
def test_refusals_are_atomic(device):
    olds = [synth.product_pools(M, N, seed=161), synth.solidly_pools(M, N, seed=162), synth.curve_pools(M, N, 3, seed=163, regime="stableswap"),
            ragged(M, 164)]
    be = backend(olds, device=device)
    bad = M - 5                                                                          # (second shard of the parent)
    rows = np.array([3, bad, 7], dtype=np.int64)
    try:
        before = be.eval(V)

        def refused(match, call, *args):
            with pytest.raises(cr.ArgumentError, match=match):
                call(*args)
            assert_same(be.eval(V), before)

        R = olds[0].R[rows] * 1.5
        for poison in (0.0, -1.0, np.inf, np.nan):
            Rb = R.copy()
            Rb[1, 1] = poison
            refused(rf"pool {bad}: reserves must be finite and > 0", be.ctx.set_reserves, 0, rows, Rb)
        Rb = olds[1].R[rows].copy()
        Rb[1, 0] = 2.0 ** 151
        refused(rf"pool {bad}: reserves of a Solidly stable pair must lie within \[2\^-150, 2\^150\]", be.ctx.set_reserves, 1, rows, Rb)
        c = olds[2]
        Rb = c.R[rows].copy()
        Rb[1] = [1e-300, 1e-300, 1e-300]                                                    # log(P0/R_k) far outside the solve's range
        refused(rf"pool {bad}: log\(P0/R_k\) = log\(beta\) - sum log R - log R_k must lie within", be.ctx.set_curve, 2, rows, Rb, c.α[rows], c.β[rows])
        al = c.α[rows].copy()
        al[1] = -1.0
        refused(rf"pool {bad}: alpha must be finite and >= 0", be.ctx.set_curve, 2, rows, c.R[rows], al, c.β[rows])
        bt = c.β[rows].copy()
        bt[1] = 0.0
        refused(rf"pool {bad}: beta must be finite and > 0", be.ctx.set_curve, 2, rows, c.R[rows], c.α[rows], bt)
        u = olds[3]
        p = u.current_price[rows].copy()
        p[1] = u.lower_ticks[u.tick_off[bad]] * 1.0001
        refused(rf"pool {bad}: current_price above the first tick", be.ctx.set_prices, 3, rows, p)
        p[1] = 0.0
        refused(rf"pool {bad}: current_price must be finite and > 0", be.ctx.set_prices, 3, rows, p)
        # the wrong entry for the kind names the right one; rows and segments out of range
        refused("cfmm_pools_set_prices", be.ctx.set_reserves, 3, rows, R)
        refused("cfmm_pools_set_curve", be.ctx.set_reserves, 2, rows, c.R[rows])
        refused("cfmm_pools_set_reserves", be.ctx.set_prices, 0, rows, p)
        refused("cfmm_pools_set_reserves", be.ctx.set_curve, 1, rows, R, al, bt)
        refused("out of range", be.ctx.set_reserves, 0, np.array([3, M, 7]), R)
        refused("out of range", be.ctx.set_reserves, 0, np.array([3, -1, 7]), R)
        refused("segment out of range", be.ctx.set_reserves, 4, rows, R)
        be.ctx.set_reserves(0, np.zeros(0, dtype=np.int64), np.zeros((0, 2)))            # count == 0: a no-op
        assert_same(be.eval(V), before)
        assert_equals_fresh(be, olds, device=device)
    finally:
        be.close()


@pytest.mark.parametrize("device", [0, [0, 0]])
def test_duplicate_rows_the_last_value_wins(device):
    olds = [synth.product_pools(M, N, seed=171), ragged(M, 172)]
    be = backend(olds, device=device)
    try:
        R = olds[0].R.copy()
        vals = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
        be.ctx.set_reserves(0, [5, 9, 5], vals)
        R[5], R[9] = vals[2], vals[1]
        top = olds[1].lower_ticks[olds[1].tick_off[5]]
        be.ctx.set_prices(1, [5, 9, 5], [0.5 * top, olds[1].current_price[9], 0.9 * top])
        p = olds[1].current_price.copy()
        p[5] = 0.9 * top
        np.testing.assert_array_equal(be.ctx.reserves(0, M), R)
        assert_equals_fresh(be, [batch_with(olds[0], R=R), batch_with(olds[1], current_price=p)], device=device)
    finally:
        be.close()


def test_plain_c_client(tmp_path):
    exe = str(tmp_path / "abi_update")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_update.c"), "-o", exe, "-L", libdir, "-lcfmm_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ABI_UPDATE_OK" in r.stdout
    assert "reserves must be finite and > 0" in r.stdout


def test_the_example_routes_updates_and_routes_again():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pool_update_example", os.path.join(ROOT, "examples", "pool_update.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after, changes = mod.main()
    assert len(changes) == 2 and before > 0 and after > 0 and before != after
