"""UniV3 mints and burns on the device (cfmm_pools_set_ticks, update_pools_ with a ladder state) and the device-side compaction
of the tick records (compact_walks).

The rule of tests/test_gpu_pool_update.py: context A is built with the old state and updated, context B is built fresh with
the new state, and every output of A equals B's BIT FOR BIT.  Both run with option "alternate" = 0 (tile order alternates
with the sweep count).  Markets come from synth.univ3_ragged_pools; prices are the market's own token prices, a few per cent
off, so most pools trade inside their tick and a sizeable minority walks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import ERR_INVALID_ARG, KIND_UNIV3, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
SHAPES = ("longer", "shorter", "single", "from_single", "liquidity", "boundaries", "empty_tick", "on_boundary")


def prices(seed, n=N, off=0.03):
    return synth.token_price_vector(n, seed) * synth.sweep_prices(n, seed=seed + 1, spread=off)


def ragged(m, seed, lo=1, hi=64, n=N):
    return synth.univ3_ragged_pools(m, n, min_ticks=lo, max_ticks=hi, seed=seed)


def ladder(b, i):
    o, e = b.tick_off[i], b.tick_off[i + 1]
    return b.lower_ticks[o:e].copy(), b.liquidity[o:e].copy()


def changed(b, i, shape, salt=0):
    """-> (shape applied, price, lower_ticks, liquidity): pool i of batch b after a mint / burn of the given shape"""
    lt, lq = ladder(b, i)
    p, nt, f = float(b.current_price[i]), lt.size, 1.0 + 0.001 * (1 + salt % 7)
    if nt == 1 and shape in ("shorter", "single", "empty_tick"):
        shape = "from_single"
    if shape == "longer":                  # a mint above the first tick and two below the last
        return shape, p, np.concatenate([[lt[0] * 1.05 * f], lt, [lt[-1] * 0.9, lt[-1] * 0.8]]), np.concatenate([[2e5 * f], lq, [3e5, 0.0]])
    if shape == "shorter":                 # a burn of the lower half (the last tick left reaches price 0)
        k = max(1, nt // 2)
        return shape, min(p, float(lt[0])), lt[:k], lq[:k]
    if shape == "single":                  # down to one tick: no walk lists
        return shape, p, lt[:1], np.array([max(lq[0], 1e5) * f])
    if shape == "from_single":             # one tick (or any ladder) to twelve, the price somewhere inside
        top = max(lt[0], p) * 1.2
        new = top * 0.93 ** np.arange(12)
        return shape, p, new, 1e6 * (0.05 + 0.07 * np.arange(12)) * f
    if shape == "liquidity":               # liquidity only; an empty tick filled, a full one emptied
        new = lq * 1.5 * f
        new[new == 0] = 4e5
        if nt > 2:
            new[nt // 2] = 0.0
        return shape, p, lt, new
    if shape == "boundaries":              # every boundary moves up a little, the price stays
        return shape, p, lt * (1.0 + 0.002 * f), lq
    if shape == "empty_tick":              # the price moves into the last tick, which is emptied
        new = lq.copy()
        new[-1] = 0.0
        return shape, 0.5 * float(lt[-1]), lt, new
    assert shape == "on_boundary"          # the price exactly on a tick boundary
    return shape, float(lt[nt // 2]), lt, lq


def with_ladders(b, rows, states):
    """the batch with pools `rows` in their new states (price, lower_ticks, liquidity): a host-side rebuild, pool by pool"""
    new = dict(zip((int(r) for r in rows), states))
    lts, lqs, p = [], [], b.current_price.copy()
    for i in range(len(b)):
        if i in new:
            p[i], lt, lq = new[i]
        else:
            lt, lq = ladder(b, i)
        lts.append(np.asarray(lt, dtype=np.float64))
        lqs.append(np.asarray(lq, dtype=np.float64))
    off = np.zeros(len(b) + 1, dtype=np.int64)
    np.cumsum([a.size for a in lts], out=off[1:])
    return cr.PoolBatch(KIND_UNIV3, current_price=p, tick_off=off, lower_ticks=np.concatenate(lts), liquidity=np.concatenate(lqs),
                        γ=b.γ.copy(), Ai=b.Ai.copy())


def set_ticks(ctx, seg, rows, states):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(s[1]) for s in states], out=off[1:])
    ctx.set_ticks(seg, rows, [s[0] for s in states], off, np.concatenate([s[1] for s in states]) if len(rows) else [],
                  np.concatenate([s[2] for s in states]) if len(rows) else [])


def rows_of(m, K, seed):
    return np.argsort(synth.uniform(seed, 4, m))[:K].astype(np.int64)


def backend(batches, n=N, device=0, **opts):
    be = cr.DeviceBackend(n, batches, device=device)
    be.ctx.set_option("alternate", 0)
    for k, x in opts.items():
        be.ctx.set_option(k, x)
    return be


def outputs(be, batches, v, eval_only=False):
    psi_e, acc_e = be.eval(v)
    out = [psi_e, np.float64(acc_e)]
    if not eval_only:
        psi, acc = be.find_arb(v)
        D, L = be.trades()
        out += [psi, np.float64(acc), np.asarray(D), np.asarray(L)]
    return out + [be.ctx.prices(s, len(b)) for s, b in enumerate(batches) if b.kind == KIND_UNIV3]


def assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"output {k}")


def assert_equals_fresh(be, batches, v, n=N, device=0, eval_only=False, **opts):
    fresh = backend(batches, n, device, **opts)
    try:
        assert_same(outputs(be, batches, v, eval_only), outputs(fresh, batches, v, eval_only))
    finally:
        fresh.close()


def every_shape(b, rows):
    states, seen = [], set()
    for k, i in enumerate(rows):
        shape, p, lt, lq = changed(b, int(i), SHAPES[k % len(SHAPES)], k)
        seen.add(shape)
        states.append((p, lt, lq))
    return states, seen


# ---- 1. updated equals fresh -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fold", "eval_only", "plain_trades", "single_block"])
def test_updated_context_equals_fresh(mode):
    m, mp, K = (1500, 0, 150) if mode == "single_block" else (3000, 1000, 300)
    old = ragged(m, 11)
    nt = np.diff(old.tick_off)
    assert nt.min() == 1 and nt.max() == 64 and (old.liquidity == 0).any()
    prod = [synth.product_pools(mp, N, seed=12)] if mp else []
    opts = {"compact_trades": 0} if mode == "plain_trades" else {}
    v = prices(11)
    be = backend([old] + prod, **opts)
    try:
        if mode == "single_block":
            assert be.ctx.segments()[0]["grid"] == 1
        be.find_arb(v)                                   # the update is enqueued behind an earlier sweep
        before = be.ctx.trades_range(1, 0, mp) if mp else None
        rows = rows_of(m, K, 5)
        states, seen = every_shape(old, rows)
        assert seen == set(SHAPES)
        set_ticks(be.ctx, 0, rows, states)
        with pytest.raises(RuntimeError, match="no materialised trades"):
            be.ctx.trades()
        now = with_ladders(old, rows, states)
        assert not np.array_equal(np.diff(now.tick_off), nt)
        assert_equals_fresh(be, [now] + prod, v, eval_only=mode == "eval_only", **opts)
        if mp and mode != "eval_only":                   # the Product rows keep their bits
            assert_same(be.ctx.trades_range(1, 0, mp), before)
    finally:
        be.close()


# ---- 2. the two plan inputs a ladder update can move ---------------------------------------------------------------------------
def test_first_walk_list_of_a_single_tick_segment():
    old, prod = ragged(3000, 21, 1, 1), synth.product_pools(3000, N, seed=22)
    assert np.diff(old.tick_off).max() == 1              # has_walk == 0: uploaded without heads
    v = prices(21)
    be = backend([prod, old])
    try:
        be.eval(v)
        rows = np.array([1234], dtype=np.int64)
        states = [changed(old, 1234, "from_single")[1:]]
        set_ticks(be.ctx, 1, rows, states)
        assert_equals_fresh(be, [prod, with_ladders(old, rows, states)], v)
    finally:
        be.close()


def test_mean_ticks_per_pool_crosses_two_in_both_directions():
    m = 3000
    old, prod = ragged(m, 31, 2, 2), synth.product_pools(m, N, seed=32)
    assert old.tick_off[-1] == 2 * m                     # T / m == 2: not "multi-tick" for the plan
    v = prices(31)
    be = backend([prod, old])
    try:
        be.eval(v)
        rows = rows_of(m, 60, 6)
        up = []
        for i in rows:                                   # 60 rows of 52 ticks: T = 3m, T / m > 2
            lt, lq = ladder(old, int(i))
            up.append((float(old.current_price[i]), np.concatenate([lt, lt[-1] * 0.97 ** np.arange(1, 51)]), np.concatenate([lq, np.full(50, 2e5)])))
        set_ticks(be.ctx, 1, rows, up)
        now = with_ladders(old, rows, up)
        assert now.tick_off[-1] == 3 * m
        assert_equals_fresh(be, [prod, now], v)
        down = [(float(old.current_price[i]),) + ladder(old, int(i)) for i in rows]
        set_ticks(be.ctx, 1, rows, down)                 # and back
        assert_equals_fresh(be, [prod, old], v)
    finally:
        be.close()


# ---- 3. refusals are atomic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, [0, 0]])
def test_refusals_are_atomic(device):
    m = 3000
    olds = [synth.product_pools(m, N, seed=41), ragged(m, 42, 2, 12)]
    v = prices(42)
    be = backend(olds, device=device)
    bad = m - 5                                          # (second shard of the parent)
    rows = np.array([3, bad, 7], dtype=np.int64)
    u = olds[1]
    good = [changed(u, int(i), "longer")[1:] for i in rows]
    try:
        before = be.eval(v)

        def refused(match, states, r=rows, seg=1, error=cr.ArgumentError):
            with pytest.raises(error, match=match):
                set_ticks(be.ctx, seg, r, states)
            assert_same(be.eval(v), before)
            np.testing.assert_array_equal(be.ctx.prices(1, m), u.current_price)

        def poisoned(fn):
            s = [tuple(np.array(a, dtype=np.float64, copy=True) for a in g) for g in good]
            s[1] = fn(*s[1])
            return [(float(p), lt, lq) for p, lt, lq in s]

        refused(rf"pool {bad}: needs at least one tick", poisoned(lambda p, lt, lq: (p, lt[:0], lq[:0])))
        refused(rf"pool {bad}: lower_ticks must be strictly descending", poisoned(lambda p, lt, lq: (p, lt[::-1].copy(), lq)))
        refused(rf"pool {bad}: lower_ticks must be strictly descending", poisoned(lambda p, lt, lq: (p, np.concatenate([lt[:1], lt]), np.concatenate([lq[:1], lq]))))
        refused(rf"pool {bad} tick 0: price must be finite and > 0", poisoned(lambda p, lt, lq: (p, np.concatenate([[np.inf], lt[1:]]), lq)))
        for poison in (-1.0, np.inf, np.nan):
            refused(rf"pool {bad} tick 1: liquidity must be finite and >= 0", poisoned(lambda p, lt, lq: (p, lt, np.concatenate([lq[:1], [poison], lq[2:]]))))
        refused(rf"pool {bad}: current_price above the first tick", poisoned(lambda p, lt, lq: (lt[0] * 1.0001, lt, lq)))
        refused(rf"pool {bad}: current_price must be finite and > 0", poisoned(lambda p, lt, lq: (0.0, lt, lq)))
        refused("out of range", good, r=np.array([3, m, 7]))
        refused("out of range", good, r=np.array([3, -1, 7]))
        refused("segment out of range", good, seg=2)
        refused("cfmm_pools_set_ticks: segment of ProductTwoCoin pools: cfmm_pools_set_reserves", good, seg=0)   # the wrong kind names this entry
        # null arrays (through the raw binding)
        L, h, idx = be.ctx._L, be.ctx._h, np.array([3], dtype=np.int64)
        p, off, lt, lq = np.array([good[0][0]]), np.array([0, good[0][1].size], dtype=np.int64), good[0][1], good[0][2]
        for args in ((None, ptr(p), ptr(off), ptr(lt), ptr(lq)), (ptr(idx), None, ptr(off), ptr(lt), ptr(lq)), (ptr(idx), ptr(p), None, ptr(lt), ptr(lq)),
                     (ptr(idx), ptr(p), ptr(off), None, ptr(lq)), (ptr(idx), ptr(p), ptr(off), ptr(lt), None)):
            assert L.cfmm_pools_set_ticks(h, 1, 1, *args) == ERR_INVALID_ARG
            assert "null pool array" in L.cfmm_last_error(h).decode()
        off[0] = 1
        assert L.cfmm_pools_set_ticks(h, 1, 1, ptr(idx), ptr(p), ptr(off), ptr(lt), ptr(lq)) == ERR_INVALID_ARG
        assert "tick_off[0] must be 0" in L.cfmm_last_error(h).decode()
        set_ticks(be.ctx, 1, np.zeros(0, dtype=np.int64), [])                              # count == 0: a no-op
        assert_same(be.eval(v), before)
        assert_equals_fresh(be, olds, v, device=device)
        set_ticks(be.ctx, 1, rows, good)                                                 # and the good rows are accepted afterwards
        assert_equals_fresh(be, [olds[0], with_ladders(u, rows, good)], v, device=device)
    finally:
        be.close()


# ---- 4. duplicates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, [0, 0]])
def test_duplicate_rows_the_last_ladder_wins(device):
    m = 3000
    old = ragged(m, 51, 2, 12)
    v = prices(51)
    be = backend([old], device=device)
    try:
        a, b, c = changed(old, 5, "longer")[1:], changed(old, 9, "single")[1:], changed(old, 5, "from_single")[1:]
        set_ticks(be.ctx, 0, np.array([5, 9, 5], dtype=np.int64), [a, b, c])
        assert_equals_fresh(be, [with_ladders(old, [5, 9], [c, b])], v, device=device)
    finally:
        be.close()


# ---- 5. compaction on the device -----------------------------------------------------------------------------------------------
def compaction_rounds(be, old, v, with_ticks, live=None):
    """rounds of updates on half the pools until the tick records have been compacted twice; after every round the sweep
    equals a fresh upload's -> the batch at the end"""
    m, now = len(old), old
    assert be.ctx.get_option("pool_update_regrows") == 0
    for r in range(12):
        rows = rows_of(m, m // 2, 70 + r)
        if with_ticks:
            states = [changed(now, int(i), ("liquidity", "boundaries", "on_boundary", "shorter", "longer")[(k + r) % 5], k + r)[1:] for k, i in enumerate(rows)]
            states = [(p, lt[:64], lq[:64]) for p, lt, lq in states]
            set_ticks(be.ctx, 0, rows, states)
            now = with_ladders(now, rows, states)
        else:
            p = now.current_price.copy()
            p[rows] = now.lower_ticks[now.tick_off[rows] + (r % 3)] * (1.0 - 0.001 * (r + 1))
            be.ctx.set_prices(0, rows, p[rows])
            now = cr.PoolBatch(KIND_UNIV3, current_price=p, tick_off=now.tick_off, lower_ticks=now.lower_ticks, liquidity=now.liquidity, γ=now.γ, Ai=now.Ai)
        assert_equals_fresh(be, [now], v)
        if be.ctx.get_option("pool_update_regrows") >= 2:
            break
    print("rounds:", r + 1, "pool_update_regrows:", be.ctx.get_option("pool_update_regrows"))
    assert 2 <= be.ctx.get_option("pool_update_regrows") and r >= 1     # (the first update compacts: an upload has no spare records)
    return now


@pytest.mark.parametrize("with_ticks", [True, False], ids=["set_ticks", "set_prices"])
def test_compaction_on_the_device(with_ticks):
    old = ragged(200, 61, 64, 64)
    be = backend([old])
    try:
        compaction_rounds(be, old, prices(61), with_ticks)
    finally:
        be.close()


def compaction_body():
    """(child process, hooks build) the compactions release exactly what they replace"""
    probe = cr.Context(4)
    live = lambda: probe.get_option("debug_live_allocs")
    old = ragged(200, 61, 64, 64)
    v = prices(61)
    be = backend([old])
    try:
        be.find_arb(v)
        be.trades()
        steady = live()
        be.ctx.set_option("time_kernels", 1)
        compaction_rounds(be, old, v, True)
        assert be.ctx.get_option("compact_walks_ns") > 0
        assert live() == steady
        be.ctx.clear()
        cleared = live()
        be.reload([old])
        be.find_arb(v)
        be.trades()
        assert live() == steady                          # the same market costs the same allocations after the rounds
        be.ctx.clear()
        assert live() == cleared
    finally:
        be.close()
    probe.close()


def test_compaction_releases_what_it_replaces():
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_pool_ticks as t\n"
            "t.compaction_body()\n"
            "print('compaction-ok')\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "compaction-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


# ---- 6. sequencing -------------------------------------------------------------------------------------------------------------
def test_sequencing_route_update_reserves_and_later_prices():
    m = 3000
    olds = [synth.product_pools(m, N, seed=81), ragged(m, 82, 1, 24)]
    rows = rows_of(m, 200, 7)
    states, _ = every_shape(olds[1], rows)
    want = [olds[0], with_ladders(olds[1], rows, states)]
    changes = {int(m + i): s for i, s in zip(rows, states)}
    bare = next(i for i in range(m) if i not in set(int(r) for r in rows))
    changes[m + bare] = float(olds[1].current_price[bare]) * 0.999                         # a bare price next to ladder states
    p = want[1].current_price.copy()
    p[bare] = changes[m + bare]
    want[1] = cr.PoolBatch(KIND_UNIV3, current_price=p, tick_off=want[1].tick_off, lower_ticks=want[1].lower_ticks, liquidity=want[1].liquidity,
                           γ=want[1].γ, Ai=want[1].Ai)
    obj = cr.LinearNonnegative(synth.linear_prices(N, seed=83))
    v = prices(82)
    copy = lambda b: b.slice(0, len(b))
    ra, rb = cr.Router(obj, [copy(b) for b in olds], N), cr.Router(obj, [copy(b) for b in want], N)
    try:
        for r in (ra, rb):
            r._backend.ctx.set_option("alternate", 0)
        cr.find_arb_(ra, v)
        cr.update_pools_(ra, changes)
        for f in ("current_price", "tick_off", "lower_ticks", "liquidity"):                # the host mirror followed
            np.testing.assert_array_equal(getattr(ra._batches[1], f), getattr(want[1], f), err_msg=f)
        with pytest.raises(RuntimeError, match="no materialised trades"):
            ra._backend.ctx.trades()
        np.testing.assert_array_equal(ra._backend.ctx.prices(1, m), want[1].current_price)   # cfmm_get_prices: the new prices
        cr.find_arb_(rb, v)                                                                # (the same number of sweeps on both)
        cr.route_(ra, v=np.ones(N), solver="native")
        cr.route_(rb, v=np.ones(N), solver="native")
        np.testing.assert_array_equal(ra.v, rb.v)
        np.testing.assert_array_equal(cr.netflows(ra), cr.netflows(rb))
        # set_ticks -> route! -> update_reserves! -> find_arb at the same prices: no trade, and the bits of the fresh context
        va, routed = ra.v.copy(), np.abs(ra.Δs[m:]).max()
        for r in (ra, rb):
            cr.update_reserves_(r)
        np.testing.assert_array_equal(ra._batches[1].current_price, rb._batches[1].current_price)
        for r in (ra, rb):
            cr.find_arb_(r, va)
        np.testing.assert_array_equal(ra.Δs, rb.Δs)
        np.testing.assert_array_equal(ra.Λs, rb.Λs)
        # no trade is left: a moved pool rests at fl(p/γ) or fl(γ·p), one rounding from the band's edge, so what a UniV3 pool
        # still trades is a rounding of its reserves (2^-53 relative, a few operations), not a trade: 2^-40 of the largest
        # routed trade bounds it with room to spare
        left = max(np.abs(ra.Δs[m:]).max(), np.abs(ra.Λs[m:]).max())
        print("largest UniV3 trade of the route:", routed, "left at the same prices:", left)
        assert routed > 0 and left <= routed * 2.0 ** -40
        assert_same(ra._backend.eval(v), rb._backend.eval(v))
        # set_prices after set_ticks validates against the NEW ladder
        i = int(rows[0])                                                                 # shape "longer": a new first tick above the old one
        top_new = want[1].lower_ticks[want[1].tick_off[i]]
        assert top_new > olds[1].lower_ticks[olds[1].tick_off[i]]
        ra._backend.ctx.set_prices(1, [i], [top_new])
        with pytest.raises(cr.ArgumentError, match=rf"pool {i}: current_price above the first tick"):
            ra._backend.ctx.set_prices(1, [i], [top_new * 1.0001])
        assert ra._backend.ctx.prices(1, m)[i] == top_new
    finally:
        ra.close()
        rb.close()


# ---- 7. large-market mode ------------------------------------------------------------------------------------------------------
def test_large_market_mode_with_a_hub_token():
    n, m = 8193, 3000
    def hub(b):
        Ai = b.Ai.copy()
        Ai[::3, 0] = 1                                  # every third pool trades the hub token
        Ai[:, 1] = np.where(Ai[:, 1] == Ai[:, 0], 2, Ai[:, 1])
        return Ai
    u = ragged(m, 91, 1, 24, n)
    u = cr.PoolBatch(KIND_UNIV3, current_price=u.current_price, tick_off=u.tick_off, lower_ticks=u.lower_ticks, liquidity=u.liquidity, γ=u.γ, Ai=hub(u))
    prod = synth.product_pools(m, n, seed=92)
    v = prices(91, n)
    be = backend([prod, u], n)
    try:
        be.find_arb(v)
        rows = rows_of(m, 100, 9)
        states, _ = every_shape(u, rows)
        set_ticks(be.ctx, 1, rows, states)
        assert_equals_fresh(be, [prod, with_ladders(u, rows, states)], v, n)
    finally:
        be.close()


# ---- 8. multi-device parent ----------------------------------------------------------------------------------------------------
def test_multi_device_parent_rows_straddle_the_shards():
    m = 3000
    olds = [synth.product_pools(m, N, seed=101), ragged(m, 102, 1, 24)]
    v = prices(102)
    be = backend(olds, device=[0, 0])
    try:
        rows = np.array([m // 2 + 1, 3, m // 2 - 1, m - 1, m // 2, 0], dtype=np.int64)    # shard boundary at m/2
        states, _ = every_shape(olds[1], rows)
        set_ticks(be.ctx, 1, rows, states)
        now = [olds[0], with_ladders(olds[1], rows, states)]
        assert_equals_fresh(be, now, v, device=[0, 0])
        single = backend(now)          # a single-device context: the same trades and state (its Ψ is summed in another order)
        try:
            assert_same(outputs(be, now, v)[4:], outputs(single, now, v)[4:])
        finally:
            single.close()
    finally:
        be.close()


# ---- 9. plain C client, the example --------------------------------------------------------------------------------------------
def test_plain_c_client(tmp_path):
    exe = str(tmp_path / "abi_ticks")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_ticks.c"), "-o", exe, "-L", libdir, "-lcfmm_amd",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ABI_TICKS_OK" in r.stdout
    assert "lower_ticks must be strictly descending" in r.stdout


def test_the_example_follows_a_mint_a_burn_and_a_swap():
    import importlib.util
    spec = importlib.util.spec_from_file_location("follow_chain_mints", os.path.join(ROOT, "examples", "follow_chain_mints.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    before, after, changes = mod.main()
    kinds = sorted(type(s).__name__ for s in changes.values())
    assert kinds.count("tuple") == 2 and len(changes) == 3 and before != after
