"""cfmm_select_trades: the rows of a segment that trade and are worth at least min_value, compacted on the device.

The expected answer in every case is numpy over the FULL download of the same sweep (ctx.trades_range):
    value = Σ_k (Λ_k − Δ_k)·v[A_k]   summed in coin order from +0.0, every operation rounded on its own
    mask  = ((Δ != 0) | (Λ != 0)).any(1) & ~(value < τ)
and idx == flatnonzero(mask), the rows, value and the count are compared with assert_array_equal: no tolerances.
The sizes come from the implementation's own geometry (read-only options "select_block_pools", "select_scan_chunk")."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import ptr

pytestmark = pytest.mark.gpu

N = 48
V = synth.sweep_prices(N, seed=7, spread=0.3)
V2 = synth.sweep_prices(N, seed=8, spread=0.3)
INF = float("inf")
SENTINEL = -12345.5


def backend(batches, n=N, device=0, compact=1):
    be = cr.DeviceBackend(n, [], device=device)
    be.ctx.set_option("compact_trades", compact)
    be.reload(batches)
    return be


def expected(D, L, Ai, v, tau):
    """numpy over the downloaded rows D, L [m, coins] with 1-based tokens Ai -> (idx, value of every pool)"""
    value = np.zeros(D.shape[0])
    for k in range(D.shape[1]):
        value = value + (L[:, k] - D[:, k]) * v[Ai[:, k] - 1]
    with np.errstate(invalid="ignore"):
        mask = ((D != 0) | (L != 0)).any(axis=1) & ~(value < tau)
    return np.flatnonzero(mask), value


def check_segment(ctx, seg, batch, v, tau, v_arg="same"):
    """select_trades of one segment against numpy over its full download; v_arg: "same" passes None (the sweep's prices)"""
    m, coins = len(batch), batch.Ai.shape[1]
    D, L = ctx.trades_range(seg, 0, m, coins)
    want, value = expected(D, L, batch.Ai, v, tau)
    idx, Ds, Ls, val = ctx.select_trades(seg, tau, v=None if v_arg == "same" else v, n_coins=coins)
    assert ctx.select_count(seg, tau, v=None if v_arg == "same" else v) == want.size
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(Ds, D[want])
    np.testing.assert_array_equal(Ls, L[want])
    np.testing.assert_array_equal(val, value[want])
    assert not np.any(np.signbit(Ds) != np.signbit(D[want])) and not np.any(np.signbit(Ls) != np.signbit(L[want]))
    return want, value


def raw_select(ctx, seg, v, tau, cap, coins=2, room=None, use=(True, True, True, True)):
    """the C entry itself on sentinel-filled buffers of `room` rows -> rc, count, idx, Δ, Λ, value"""
    room = max(cap, 1) if room is None else room
    idx, val = np.full(room, -7, dtype=np.int64), np.full(room, SENTINEL)
    D, L = np.full((room, coins), SENTINEL), np.full((room, coins), SENTINEL)
    count = C.c_int64(-1)
    vv = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    rc = ctx._L.cfmm_select_trades(ctx._h, seg, ptr(vv), float(tau), cap, C.byref(count), ptr(idx) if use[0] else None,
                                   ptr(D) if use[1] else None, ptr(L) if use[2] else None, ptr(val) if use[3] else None)
    return rc, count.value, idx, D, L, val


def middle(value, mask_trading):
    return float(np.median(value[mask_trading])) if mask_trading.any() else 0.0


# ---- geometry ---------------------------------------------------------------------------------------------------------------
GEOMETRY = {"one": lambda P, S: 1, "63": lambda P, S: 63, "64": lambda P, S: 64, "65": lambda P, S: 65,
            "block-1": lambda P, S: P - 1, "block": lambda P, S: P, "block+1": lambda P, S: P + 1,
            "three-blocks+37": lambda P, S: 3 * P + 37, "scan-carry": lambda P, S: P * S + 1}


@pytest.mark.parametrize("size", list(GEOMETRY))
def test_geometry(size):
    probe = cr.Context(4)
    P, S = probe.get_option("select_block_pools"), probe.get_option("select_scan_chunk")
    probe.close()
    assert P % 64 == 0 and S >= 64 and P * S + 1 <= 1 << 20
    m = GEOMETRY[size](P, S)
    b = synth.product_pools(m, N, seed=21)
    be = backend([b])
    try:
        be.find_arb(V)
        want, value = check_segment(be.ctx, 0, b, V, -INF)
        assert want.size > 0.9 * m or m < 64
        trading = np.zeros(m, dtype=bool)
        trading[want] = True
        got, _ = check_segment(be.ctx, 0, b, V, middle(value, trading))
        assert m < 4 or 0 < got.size < want.size
    finally:
        be.close()


# ---- selectivity --------------------------------------------------------------------------------------------------------------
def idle_pools(m, seed=5):
    """Product pools that sit exactly on the prices V: R_k = S / V[token k], fee 0.3 % -> inside every fee band"""
    Ai = synth.token_pairs(seed, 1, m, N)
    S = 100.0 + 900.0 * synth.uniform(seed, 3, m)
    R = S[:, None] / V[Ai - 1]
    return cr.ProductTwoCoin.batch(R, np.full(m, 0.997), Ai)


def test_selectivity():
    m = 1000
    b = synth.product_pools(m, N, seed=22)
    be = backend([b])
    try:
        be.find_arb(V)
        want, value = check_segment(be.ctx, 0, b, V, -INF)
        D, L = be.ctx.trades_range(0, 0, m)
        assert want.size == np.count_nonzero(((D != 0) | (L != 0)).any(axis=1)) > 0.9 * m
        trading = np.zeros(m, dtype=bool)
        trading[want] = True
        got, _ = check_segment(be.ctx, 0, b, V, middle(value, trading))
        assert 0.3 * want.size < got.size < 0.7 * want.size
        none, _ = check_segment(be.ctx, 0, b, V, INF)          # +inf selects only NaN-valued rows: none here
        assert none.size == 0
    finally:
        be.close()
    idle = idle_pools(m)
    be = backend([idle])
    try:
        be.find_arb(V)
        D, L = be.ctx.trades_range(0, 0, m)
        assert not D.any() and not L.any()
        rc, count, idx, Ds, Ls, val = raw_select(be.ctx, 0, None, -INF, 16)
        assert rc == 0 and count == 0
        assert np.all(idx == -7) and np.all(Ds == SENTINEL) and np.all(Ls == SENTINEL) and np.all(val == SENTINEL)
    finally:
        be.close()


# ---- capacity -----------------------------------------------------------------------------------------------------------------
def test_capacity_and_optional_outputs():
    m = 700
    b = synth.product_pools(m, N, seed=23)
    be = backend([b])
    try:
        be.find_arb(V)
        D, L = be.ctx.trades_range(0, 0, m)
        want, value = expected(D, L, b.Ai, V, 0.0)
        n = want.size
        assert n > 10
        rc, count, idx, Ds, Ls, val = raw_select(be.ctx, 0, None, 0.0, 0, room=4)                  # counts only
        assert rc == 0 and count == n and np.all(idx == -7) and np.all(Ds == SENTINEL) and np.all(val == SENTINEL)
        rc, count, idx, Ds, Ls, val = raw_select(be.ctx, 0, None, 0.0, n - 1, room=n)              # the first n - 1 rows, no more
        assert rc == 0 and count == n
        np.testing.assert_array_equal(idx[:n - 1], want[:n - 1])
        np.testing.assert_array_equal(Ds[:n - 1], D[want[:n - 1]])
        np.testing.assert_array_equal(Ls[:n - 1], L[want[:n - 1]])
        np.testing.assert_array_equal(val[:n - 1], value[want[:n - 1]])
        assert idx[n - 1] == -7 and np.all(Ds[n - 1] == SENTINEL) and np.all(Ls[n - 1] == SENTINEL) and val[n - 1] == SENTINEL
        for cap in (n, n + 5, 10 * m):                                                              # >= count
            rc, count, idx, Ds, Ls, val = raw_select(be.ctx, 0, None, 0.0, cap, room=max(cap, n) + 1)
            assert rc == 0 and count == n
            np.testing.assert_array_equal(idx[:n], want)
            np.testing.assert_array_equal(Ds[:n], D[want])
            np.testing.assert_array_equal(val[:n], value[want])
            assert idx[n] == -7 and val[n] == SENTINEL and np.all(Ls[n] == SENTINEL)
        for skip in range(4):                                                                       # each optional output NULL in turn
            use = tuple(k != skip for k in range(4))
            rc, count, idx, Ds, Ls, val = raw_select(be.ctx, 0, None, 0.0, n, use=use)
            assert rc == 0 and count == n
            for k, (got, ref) in enumerate(((idx, want), (Ds, D[want]), (Ls, L[want]), (val, value[want]))):
                if use[k]:
                    np.testing.assert_array_equal(got[:n], ref)
                else:
                    assert np.all(got == (-7 if k == 0 else SENTINEL))
        rc, count, *_ = raw_select(be.ctx, 0, None, 0.0, -1, room=1)
        assert rc == -1 and "capacity" in be.ctx._L.cfmm_last_error(be.ctx._h).decode()
        for seg in (-1, 1):
            rc, *_ = raw_select(be.ctx, seg, None, 0.0, 4)
            assert rc == -1
        with pytest.raises(cr.ArgumentError):
            be.ctx.select_trades(0, capacity=-1)
        # the wrapper: too small a first capacity is repeated once with the count
        idx, Ds, Ls, val = be.ctx.select_trades(0, 0.0, capacity=None)
        np.testing.assert_array_equal(idx, want)
        idx, Ds, Ls, val = be.ctx.select_trades(0, 0.0, capacity=7)
        np.testing.assert_array_equal(idx, want[:7])
    finally:
        be.close()


# ---- layouts and kinds --------------------------------------------------------------------------------------------------------
def both_directions(m, seed=31):
    """Product pools with γ > 1: near their marginal price they trade in BOTH directions (the overflow rows {0, −1})"""
    Ai = synth.token_pairs(seed, 1, m, N)
    S = 100.0 + 900.0 * synth.uniform(seed, 3, m)
    R = S[:, None] / V[Ai - 1] * np.exp(0.002 * (2.0 * synth.uniform(seed, 4, 2 * m).reshape(m, 2) - 1.0))
    return cr.ProductTwoCoin.batch(R, np.full(m, 1.01), Ai)


def degenerate_univ3(m, n=16, seed=7):
    """ragged ladders of 1..40 ticks, empty current ticks, prices ON tick boundaries, γ = 1 and tiny: the pools whose
    tick arithmetic yields tiny negatives and −0.0 (tests/test_gpu_parity.py's market, smaller)"""
    rng = np.random.default_rng(seed)
    nt = rng.integers(1, 41, m)
    off = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(nt, out=off[1:])
    ticks, liq, cp = np.empty(off[-1]), np.empty(off[-1]), np.empty(m)
    for i in range(m):
        t = np.sort(10.0 ** rng.uniform(-3, 3, nt[i]))[::-1]
        t *= 1.0 + np.arange(nt[i])[::-1] * 1e-9
        ticks[off[i]:off[i + 1]] = t
        lq = 10.0 ** rng.uniform(-2, 6, nt[i])
        lq[rng.random(nt[i]) < 0.3] = 0.0
        liq[off[i]:off[i + 1]] = lq
        k = rng.integers(0, nt[i])
        cp[i] = t[k] if rng.random() < 0.3 else t[k] * rng.uniform(0.5, 1.0)
    return cr.UniV3.batch(cp, off, ticks, liq, rng.choice([1.0, 0.997, 0.3], m), synth.token_pairs(5, 1, m, n))


KINDS = {
    "product-both-directions": (lambda: both_directions(777), N, V),
    "geomean": (lambda: synth.geomean_pools(777, N, seed=32), N, V),
    "solidly": (lambda: synth.solidly_pools(777, N, seed=33), N, V),
    "univ3-ragged": (lambda: synth.univ3_ragged_pools(777, N, min_ticks=2, max_ticks=12, seed=34), N, None),
    "univ3-degenerate": (lambda: degenerate_univ3(3000), 16, synth.sweep_prices(16, seed=5, spread=0.05)),
    "weighted3": (lambda: synth.weighted_pools(777, N, 3, seed=35), N, V),
    "weighted8": (lambda: synth.weighted_pools(777, N, 8, seed=36), N, V),
    "curve3": (lambda: synth.curve_pools(777, N, 3, seed=37), N, V),
    "curve8": (lambda: synth.curve_pools(777, N, 8, seed=38), N, V),
}


@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("kind", list(KINDS))
def test_layouts_and_kinds(kind, compact):
    make, n, v = KINDS[kind]
    b = make()
    if v is None:   # a few per cent off the token prices behind the ragged ladders: most pools trade, some walk
        v = synth.token_price_vector(n, 34) * np.exp(0.03 * (2.0 * synth.uniform(9, 1, n) - 1.0))
    be = backend([b], n=n, compact=compact)
    try:
        be.find_arb(v)
        m, coins = len(b), b.Ai.shape[1]
        D, L = be.ctx.trades_range(0, 0, m, coins)
        want, value = check_segment(be.ctx, 0, b, v, -INF)
        assert 0 < want.size
        trading = np.zeros(m, dtype=bool)
        trading[want] = True
        got, _ = check_segment(be.ctx, 0, b, v, middle(value, trading))
        assert 0 < got.size < want.size
        check_segment(be.ctx, 0, b, v, 0.0)
        if kind == "product-both-directions":
            both = (D[:, 0] != 0) & (D[:, 1] != 0) & (L[:, 0] != 0) & (L[:, 1] != 0)
            assert both.sum() > 50 and np.all(trading[both])        # the overflow rows are there, and selected
        if kind == "univ3-degenerate":
            assert np.count_nonzero(((D < 0) | (L < 0)).any(axis=1)) >= 1      # the tiny negatives of the tick arithmetic
            zero_only = ~((D != 0) | (L != 0)).any(axis=1)
            assert zero_only.any() and not np.any(trading[zero_only])          # ±0.0 alone never selects a pool
    finally:
        be.close()


def test_mixed_market_segment_by_segment_and_router():
    batches = [synth.product_pools(500, N, seed=41), synth.geomean_pools(301, N, seed=42),
               synth.univ3_ragged_pools(257, N, min_ticks=2, max_ticks=12, seed=43), synth.weighted_pools(130, N, 3, seed=44)]
    r = cr.Router(cr.LinearNonnegative(np.ones(N)), batches, N)
    try:
        cr.find_arb_(r, V)
        ctx = r._backend.ctx
        assert len(ctx.segments()) == 4
        first, all_idx, all_val, rows_D = 0, [], [], []
        for seg, b in enumerate(batches):
            want, value = check_segment(ctx, seg, b, V, 0.0)
            D, _ = ctx.trades_range(seg, 0, len(b), b.Ai.shape[1])
            all_idx.append(want + first)
            all_val.append(value[want])
            rows_D += [D[i] for i in want]
            first += len(b)
        idx, Ds, Ls, val = cr.active_trades(r, 0.0)
        np.testing.assert_array_equal(idx, np.concatenate(all_idx))
        np.testing.assert_array_equal(val, np.concatenate(all_val))
        assert len(Ds) == len(rows_D) == len(Ls)
        for a, b_ in zip(Ds, rows_D):
            np.testing.assert_array_equal(a, b_)
        full = r.Δs                                        # and the rows are r.Δs's
        for i, a in zip(idx, Ds):
            np.testing.assert_array_equal(a, full[int(i)])
    finally:
        r.close()


def test_large_market_mode_with_a_hub_token():
    n, m = 8200, 3000
    Ai = synth.token_pairs(51, 1, m, n)
    Ai[::3, 0] = 1                                        # a hub: every third pool trades token 1 ...
    Ai[::3, 1] = np.where(Ai[::3, 1] == 1, 2, Ai[::3, 1])
    Ai[1, :] = (n, n - 1)                                 # ... and the last tokens are used
    p = synth.product_pools(m, n, seed=52)
    b = cr.ProductTwoCoin.batch(p.R, p.γ, Ai)
    v = synth.sweep_prices(n, seed=53, spread=0.3)
    be = backend([b], n=n)
    try:
        be.find_arb(v)
        want, value = check_segment(be.ctx, 0, b, v, -INF)
        trading = np.zeros(m, dtype=bool)
        trading[want] = True
        got, _ = check_segment(be.ctx, 0, b, v, middle(value, trading))
        assert 0 < got.size < want.size and trading[1] and np.any(trading[::3])
    finally:
        be.close()


# ---- prices -------------------------------------------------------------------------------------------------------------------
def test_prices_null_and_explicit():
    m = 900
    b = synth.product_pools(m, N, seed=61)
    be = backend([b])
    try:
        be.find_arb(V)
        want, value = check_segment(be.ctx, 0, b, V, 0.0)                      # v = NULL after cfmm_find_arb
        D, L = be.ctx.trades_range(0, 0, m)
        want2, value2 = check_segment(be.ctx, 0, b, V2, -INF, v_arg="explicit")   # other prices: other values, the same rows
        assert np.any(value2 != value)
        idx, Ds, Ls, val = be.ctx.select_trades(0, -INF, v=V2)
        np.testing.assert_array_equal(Ds, D[want2])
        vout, psi, info = be.ctx.route(0, np.ones(N))                          # v = NULL after cfmm_route: its final prices
        check_segment(be.ctx, 0, b, vout, 0.0)
    finally:
        be.close()


def test_prices_after_a_device_pointer_sweep():
    from helpers import dev_sweep
    m = 900
    b = synth.product_pools(m, N, seed=62)
    be = backend([b])
    try:
        dev_sweep(be, V)
        rc, count, *_ = raw_select(be.ctx, 0, None, 0.0, 4)
        assert rc == -3 and "cfmm_sweep_dev" in be.ctx._L.cfmm_last_error(be.ctx._h).decode()
        with pytest.raises(RuntimeError, match="cfmm_sweep_dev"):
            be.ctx.select_trades(0)
        check_segment(be.ctx, 0, b, V, 0.0, v_arg="explicit")
        # one NaN price: the pools on that token are selected at any τ, their NaNs intact
        vn = V.copy()
        vn[3] = np.nan
        dev_sweep(be, vn)
        D, L = be.ctx.trades_range(0, 0, m)
        on3 = np.flatnonzero((b.Ai == 4).any(axis=1))
        assert on3.size > 5 and np.isnan(D[on3]).any()
        for tau in (-INF, 0.0, 1e300, INF):
            want, value = check_segment(be.ctx, 0, b, vn, tau, v_arg="explicit")
            assert np.all(np.isin(on3, want)) and np.all(np.isnan(value[on3]))
        only_nan, _ = check_segment(be.ctx, 0, b, vn, INF, v_arg="explicit")
        np.testing.assert_array_equal(only_nan, on3)
    finally:
        be.close()


# ---- state --------------------------------------------------------------------------------------------------------------------
def test_state():
    m = 600
    b = synth.product_pools(m, N, seed=63)
    be = backend([b])
    try:
        with pytest.raises(RuntimeError, match="no materialised trades"):
            be.ctx.select_trades(0)
        be.eval(V)
        with pytest.raises(RuntimeError, match="no materialised trades"):
            be.ctx.select_trades(0)
        be.find_arb(V)
        D0, L0 = be.trades()
        a = be.ctx.select_trades(0, 0.0)
        a2 = be.ctx.select_trades(0, 0.0)                                       # two selections in a row are identical
        for x, y in zip(a, a2):
            np.testing.assert_array_equal(x, y)
        D1, L1 = be.trades()                                                   # the download is what it was
        np.testing.assert_array_equal(D0, D1)
        np.testing.assert_array_equal(L0, L1)
        be.ctx.select_trades(0, 0.0)
        R0 = be.ctx.reserves(0, m)
        be.ctx.update_reserves()                                               # still works, and consumes the trades
        np.testing.assert_array_equal(be.ctx.reserves(0, m), (R0 + b.γ[:, None] * D0) - L0)
        with pytest.raises(RuntimeError, match="no materialised trades"):
            be.ctx.select_trades(0)
        be.find_arb(V)
        be.ctx.set_reserves(0, [5], b.R[5:6] * 1.5)
        with pytest.raises(RuntimeError, match="no materialised trades"):
            be.ctx.select_trades(0)
    finally:
        be.close()


# ---- the loop it is for ---------------------------------------------------------------------------------------------------------
LOOP_SEED, LOOP_MOVED = 71, 50


def loop_market(seed=LOOP_SEED):
    """20 000 mixed pools (ProductTwoCoin and GeometricMeanTwoCoin, fee 0.3 %) whose marginal prices scatter by ±0.32 % around
    one token price vector π: a market close to no-arbitrage, as real pools are -- a few per cent of it sits outside its
    fee band.  -> batches, π"""
    pi = synth.token_price_vector(N, seed)
    mp, mg = 12_000, 8_000
    noise = lambda m, stream: np.exp(0.0032 * (2.0 * synth.uniform(seed, stream, m) - 1.0))
    Ap = synth.token_pairs(seed, 1, mp, N)
    Sp = 100.0 + 900.0 * synth.uniform(seed, 3, mp)
    Rp = Sp[:, None] / pi[Ap - 1]
    Rp[:, 0] *= noise(mp, 4)
    Ag = synth.token_pairs(seed, 5, mg, N)
    w1 = np.clip(synth.uniform(seed, 7, mg), 0.1, 0.9)
    w = np.stack([w1, 1.0 - w1], axis=1)
    Rg = (100.0 + 900.0 * synth.uniform(seed, 8, mg))[:, None] * w / pi[Ag - 1]
    Rg[:, 0] *= noise(mg, 9)
    return [cr.ProductTwoCoin.batch(Rp, np.full(mp, 0.997), Ap), cr.GeometricMeanTwoCoin.batch(Rg, w, np.full(mg, 0.997), Ag)], pi


def run_loop(r, batches):
    """route!, update_reserves!, move LOOP_MOVED pools, find_arb! at the same prices -> those prices"""
    cr.route_(r, solver="native")
    v = r.v.copy()
    cr.update_reserves_(r)
    rows = np.argsort(synth.uniform(LOOP_SEED, 10, len(batches[0])))[:LOOP_MOVED]
    f = np.exp(0.05 * (2.0 * synth.uniform(LOOP_SEED, 11, 2 * LOOP_MOVED).reshape(-1, 2) - 1.0))
    cr.update_pools_(r, {int(i): batches[0].R[i] * f[k] for k, i in enumerate(rows)})
    cr.find_arb_(r, v)
    return v


def test_the_loop_it_is_for():
    """(The same loop on the CPU oracle: tests/test_select_trades_cpu.py -- the bound holds for the reference arithmetic.)"""
    batches, pi = loop_market()
    m_all = sum(len(b) for b in batches)
    r = cr.Router(cr.LinearNonnegative(pi), batches, N)
    try:
        v = run_loop(r, batches)
        ctx = r._backend.ctx
        first, want_all = 0, []
        for seg, b in enumerate(batches):
            want, _ = check_segment(ctx, seg, b, v, 0.0)
            want_all.append(want + first)
            first += len(b)
        want_all = np.concatenate(want_all)
        idx, Ds, Ls, val = cr.active_trades(r, 0.0)
        np.testing.assert_array_equal(idx, want_all)
        print("selected", idx.size, "of", m_all)
        assert 0 < idx.size < 0.05 * m_all
    finally:
        r.close()


def test_the_example_ends_with_the_short_list():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("active_trades_example", os.path.join(root, "examples", "active_trades.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    idx, D, L, value, rows = mod.main(m=2000, moved=10)
    assert 10 <= idx.size < 200 and np.all(np.isin(rows, idx)) and np.all(value >= 1e-6) and D.shape == L.shape == (idx.size, 2)


# ---- multi-device parents -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_device_parent(devices):
    batches = [synth.product_pools(1001, N, seed=81), synth.weighted_pools(334, N, 3, seed=82), synth.geomean_pools(5, N, seed=83)]
    be = backend(batches, device=devices)
    single = backend(batches)
    try:
        be.find_arb(V)
        single.find_arb(V)
        for seg, b in enumerate(batches):
            want, value = check_segment(be.ctx, seg, b, V, 0.0)
            one = single.ctx.select_trades(seg, 0.0, n_coins=b.Ai.shape[1])
            many = be.ctx.select_trades(seg, 0.0, n_coins=b.Ai.shape[1])
            for x, y in zip(one, many):
                np.testing.assert_array_equal(x, y)
        # a capacity that runs out inside the second shard
        b, nd = batches[0], len(devices)
        D, L = be.ctx.trades_range(0, 0, len(b))
        want, value = expected(D, L, b.Ai, V, 0.0)
        bound = -(-len(b) // nd)                           # rows of shard 0
        in_first = int(np.count_nonzero(want < bound))
        in_second = int(np.count_nonzero((want >= bound) & (want < 2 * bound)))
        assert in_first > 3 and in_second > 3
        cap = in_first + in_second // 2
        rc, count, idx, Ds, Ls, val = raw_select(be.ctx, 0, None, 0.0, cap, room=cap + 1)
        assert rc == 0 and count == want.size
        np.testing.assert_array_equal(idx[:cap], want[:cap])
        np.testing.assert_array_equal(Ds[:cap], D[want[:cap]])
        np.testing.assert_array_equal(val[:cap], value[want[:cap]])
        assert idx[cap] == -7 and val[cap] == SENTINEL
    finally:
        be.close()
        single.close()


# ---- ownership ------------------------------------------------------------------------------------------------------------------
def ownership_body():
    probe = cr.Context(4)
    live = lambda: probe.get_option("debug_live_allocs")
    before = live()
    batches = [synth.product_pools(1500, N, seed=91), synth.curve_pools(300, N, 4, seed=92)]
    be = backend(batches)
    try:
        be.find_arb(V)
        be.trades()
        steady = live()
        first = [be.ctx.select_trades(s, 0.0, n_coins=b.Ai.shape[1]) for s, b in enumerate(batches)]
        grown = live()
        assert grown > steady                                  # the scratch and the output rows are context-owned DevBufs
        for _ in range(3):                                     # repeated selections at one size allocate nothing new
            again = [be.ctx.select_trades(s, 0.0, n_coins=b.Ai.shape[1]) for s, b in enumerate(batches)]
            assert live() == grown
            for a, c in zip(first, again):
                for x, y in zip(a, c):
                    np.testing.assert_array_equal(x, y)
        be.ctx.select_count(0, 0.0)
        assert live() == grown
    finally:
        be.close()
    assert live() == before
    probe.close()


def test_ownership():
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_select_trades as t\n"
            "t.ownership_body()\n"
            "print('ownership-ok')\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "ownership-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])
