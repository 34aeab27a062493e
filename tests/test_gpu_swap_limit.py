"""cfmm_swap_limit on the device, every family: the pools of tests/golden/quote_precise.npz, one pool per row.  A TWIN context
runs the three calls the entry replaces -- cfmm_quote_to_rate, min, cfmm_swap -- and everything is compared bit for bit: the
amounts used and out, the statuses and the whole segment's state afterwards.  Then the order of a batch that names one row
several times, the limit 0.0, the amount +inf, a refused state, UniV3 across a tick boundary and into an empty tick's range,
and the rows a batch does not name.  Shapes: the fixture's groups (28 .. 46 pools, UniV3 5) and counts 1, 64 and 65."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
import to_rate_precise_ref as TP
from test_gpu_quote_precise import N_TOKENS, upload

pytestmark = pytest.mark.gpu
INF = np.inf


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fx():
    return P.load()


def fresh(fx, gname):
    ctx = cr.Context(N_TOKENS, 0)
    upload(ctx, gname, P.group(fx, gname))
    return ctx


def one_per_pool(gname, g, flip=False):
    """(idx, coin_in, coin_out or None, a fallback amount) -- every pool once, so a batch is one wave"""
    if gname == "univ3":
        m = g["current_price"].size
        ci = (np.arange(m) + int(flip)) % 2
        return np.arange(m, dtype=np.int64), ci.astype(np.int32), None, np.ones(m)
    m = g["a"].size
    two = g["R"].shape[1] == 2 and P.family(gname) not in ("weighted", "curve")
    ci, co = (g["cout"], g["cin"]) if flip else (g["cin"], g["cout"])
    fallback = np.where(g["a"] > 0.0, g["a"], 1e-3 * g["R"][np.arange(m), ci])
    return np.arange(m, dtype=np.int64), ci.astype(np.int32), None if two else co.astype(np.int32), fallback


def state(ctx, gname, g):
    if gname == "univ3":
        return (bits(ctx.prices(0, g["current_price"].size)),)
    return (bits(ctx.reserves(0, *g["R"].shape)),)


def probes(ctx, gname, g):
    """quotes of both directions of every pool: the prepared state behind the reserves / prices, as the kernels read it"""
    out = []
    for flip in (False, True):
        idx, ci, co, amt = one_per_pool(gname, g, flip)
        out.append(bits(ctx.quote(0, amt, ci, co, idx)))
    return out


def reference(twin, amount, lim, ci, co, idx):
    """cfmm_quote_to_rate -> min -> cfmm_swap on the twin: (used, out, status)"""
    a_lim = np.full(amount.size, INF)
    has = lim > 0.0
    if has.any():
        a_lim[has] = twin.quote_to_rate(0, lim[has], ci[has], None if co is None else co[has], idx[has], want_out=False)[0]
    used = np.minimum(amount, a_lim)
    out = twin.swap(0, used, ci, co, idx)
    status = np.where(used == 0.0, cr.LIMIT_NONE, np.where(used == amount, cr.LIMIT_FILLED, cr.LIMIT_PARTIAL)).astype(np.int32)
    refused = np.isnan(out)
    status[refused] = cr.LIMIT_REFUSED
    return np.where(refused, np.nan, used), out, status, a_lim


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("gname", P.GROUPS)
def test_twin_quote_to_rate_min_swap_bit_for_bit(fx, gname, flip):
    g = P.group(fx, gname)
    ctx, twin = fresh(fx, gname), fresh(fx, gname)
    try:
        idx, ci, co, fallback = one_per_pool(gname, g, flip)
        n = idx.size
        spot = ctx.quote_rate(0, None, ci, co, idx, want_out=False)[1]
        assert np.all(spot > 0.0)
        lim = spot * np.resize([0.999, 0.9, 0.5, 2.0, 0.0, 0.9, 0.5, 0.999], n)
        a_lim = twin.quote_to_rate(0, np.where(lim > 0.0, lim, spot), ci, co, idx, want_out=False)[0]
        # below the limit's amount (FILLED), above it (PARTIAL), +inf (PARTIAL), 0 (NONE), by a period coprime to the ladder's
        pattern = np.resize([0.5, 2.0, INF, 0.0, 0.5, INF, 2.0], n)
        with np.errstate(invalid="ignore"):
            amount = np.where((lim > 0.0) & (a_lim > 0.0), pattern * a_lim, np.where(pattern == 0.0, 0.0, fallback))
        amount = np.where(np.isfinite(amount) | (lim > 0.0), amount, fallback)
        assert not np.any(np.isnan(amount))
        used, out, status = ctx.swap_limit(0, amount, lim, ci, co, idx)
        r_used, r_out, r_status, r_lim = reference(twin, amount, lim, ci, co, idx)
        np.testing.assert_array_equal(bits(used), bits(r_used))
        np.testing.assert_array_equal(bits(out), bits(r_out))
        np.testing.assert_array_equal(status, r_status)
        for a, b in zip(state(ctx, gname, g) + tuple(probes(ctx, gname, g)), state(twin, gname, g) + tuple(probes(twin, gname, g))):
            np.testing.assert_array_equal(a, b)
        # the contracts by name
        inf_in = np.isinf(amount)
        assert inf_in.any() and np.all(bits(used[inf_in]) == bits(r_lim[inf_in]))            # +inf: the full amount to the limit
        none = status == cr.LIMIT_NONE
        assert none.any() and np.all(bits(used[none]) == 0) and np.all(bits(out[none]) == 0)
        filled = status == cr.LIMIT_FILLED
        assert filled.any() and np.all(bits(used[filled]) == bits(amount[filled]))
        partial = status == cr.LIMIT_PARTIAL
        assert partial.any() and np.all((used[partial] > 0.0) & (used[partial] < amount[partial]))
        assert ctx.get_option("swap_refused") == int(np.sum(status == cr.LIMIT_REFUSED))
    finally:
        ctx.close()
        twin.close()


@pytest.mark.parametrize("gname", P.GROUPS)
def test_limit_zero_is_cfmm_swap(fx, gname):
    g = P.group(fx, gname)
    ctx, twin = fresh(fx, gname), fresh(fx, gname)
    try:
        idx, ci, co, amount = one_per_pool(gname, g)
        used, out, status = ctx.swap_limit(0, amount, 0.0, ci, co, idx)
        want = twin.swap(0, amount, ci, co, idx)
        np.testing.assert_array_equal(bits(out), bits(want))
        ok = ~np.isnan(want)
        assert ok.any() and np.all(bits(used[ok]) == bits(amount[ok])) and np.all(status[ok] == cr.LIMIT_FILLED)
        assert np.all(np.isnan(used[~ok])) and np.all(status[~ok] == cr.LIMIT_REFUSED)
        for a, b in zip(state(ctx, gname, g), state(twin, gname, g)):
            np.testing.assert_array_equal(a, b)
    finally:
        ctx.close()
        twin.close()


def typical_row(gname, g):
    if gname == "univ3":
        return 0, 0, None
    r = int(np.flatnonzero(g["cls"] == "typical")[0])
    two = g["R"].shape[1] == 2 and P.family(gname) not in ("weighted", "curve")
    return r, int(g["cin"][r]), None if two else int(g["cout"][r])


@pytest.mark.parametrize("gname", P.GROUPS)
def test_one_row_named_repeatedly_is_swapped_in_order(fx, gname):
    """Four swaps of one row, four waves: half the way to the limit (FILLED), then as much as it takes (PARTIAL: it must see
    the first swap's state), then the same limit again -- the pool rests at the limit to rounding, so this one finds nothing
    or an ulp-scale remainder -- and the limit with a strict caller's margin of 2^-30: NONE.
    (The issue names three swaps, the third reporting CFMM_LIMIT_NONE.  With the SAME limit that cannot be promised: the new
    reserves are rounded again, and their spot rate lands within a few ulps on either side of the limit.  So the third swap is
    held to "NONE, or PARTIAL with at most 2^-40 of the first amount", and NONE is asserted on the swap that carries the margin
    the header tells strict callers to pass.  DESIGN §3.3o says the same.)"""
    g = P.group(fx, gname)
    ctx, twin = fresh(fx, gname), fresh(fx, gname)
    try:
        row, c_in, c_out = typical_row(gname, g)
        idx = np.full(4, row, dtype=np.int64)
        ci = np.full(4, c_in, dtype=np.int32)
        co = None if c_out is None else np.full(4, c_out, dtype=np.int32)
        one = lambda a: np.array([a]) if a is not None else None   # noqa: E731
        q1 = (one(c_in), one(c_out), one(row))
        r = 0.9 * ctx.quote_rate(0, None, *q1, want_out=False)[1][0]
        a0 = twin.quote_to_rate(0, one(r), *q1)[0][0]
        lim = np.array([r, r, r, r * (1.0 + 2.0 ** -30)])
        used, out, status = ctx.swap_limit(0, np.array([0.5 * a0, INF, INF, INF]), lim, ci, co, idx)
        assert ctx.get_option("swap_launches") == 4
        # the twin, call by call
        o1 = twin.swap(0, one(0.5 * a0), *q1)[0]
        a1 = twin.quote_to_rate(0, one(r), *q1)[0][0]
        o2 = twin.swap(0, one(a1), *q1)[0]
        assert status[0] == cr.LIMIT_FILLED and bits(used[0]) == bits(0.5 * a0) and bits(out[0]) == bits(o1)
        assert status[1] == cr.LIMIT_PARTIAL and bits(used[1]) == bits(a1) and bits(out[1]) == bits(o2)
        assert 0.25 * a0 < a1 < 0.75 * a0                      # the second swap saw the first's state, not the upload's
        a2 = twin.quote_to_rate(0, one(r), *q1)[0][0]
        assert bits(used[2]) == bits(a2) and used[2] <= 2.0 ** -40 * a0
        assert status[2] == (cr.LIMIT_NONE if a2 == 0.0 else cr.LIMIT_PARTIAL)
        assert status[3] == cr.LIMIT_NONE and bits(used[3]) == 0 and bits(out[3]) == 0
        if a2 > 0.0:
            twin.swap(0, one(a2), *q1)
        for a, b in zip(state(ctx, gname, g), state(twin, gname, g)):
            np.testing.assert_array_equal(a, b)
        spot = ctx.quote_rate(0, None, *q1, want_out=False)[1][0]
        assert abs(spot - r) <= 1e-12 * r                      # the pool rests at the limit
    finally:
        ctx.close()
        twin.close()


@pytest.mark.parametrize("gname", [g for g in P.GROUPS if g != "univ3"])
def test_a_refused_state_moves_nothing_and_unnamed_rows_keep_every_bit(fx, gname):
    g = P.group(fx, gname)
    ctx = fresh(fx, gname)
    try:
        before, probed = state(ctx, gname, g), probes(ctx, gname, g)
        row, c_in, c_out = typical_row(gname, g)
        other = (row + 1) % g["a"].size
        idx = np.array([row, other], dtype=np.int64)
        ci = np.array([c_in, int(g["cin"][other])], dtype=np.int32)
        co = None if c_out is None else np.array([c_out, int(g["cout"][other])], dtype=np.int32)
        # no limit and an amount no reserve can take: cfmm_pools_set_* would refuse the state; beside it a swap that finds
        # its pool below the limit already
        used, out, status = ctx.swap_limit(0, np.array([1e300, 1.0]), np.array([0.0, 1e300]), ci, co, idx)
        assert status[0] == cr.LIMIT_REFUSED and np.isnan(used[0]) and np.isnan(out[0])
        assert status[1] == cr.LIMIT_NONE and bits(used[1]) == 0 and bits(out[1]) == 0
        assert ctx.get_option("swap_refused") == 1
        for a, b in zip(before + tuple(probed), state(ctx, gname, g) + tuple(probes(ctx, gname, g))):
            np.testing.assert_array_equal(a, b)
        # one applied swap: every other row keeps every bit
        lim = 0.5 * ctx.quote_rate(0, None, ci[:1], None if co is None else co[:1], idx[:1], want_out=False)[1]
        used, out, status = ctx.swap_limit(0, np.array([INF]), lim, ci[:1], None if co is None else co[:1], idx[:1])
        assert status[0] == cr.LIMIT_PARTIAL and used[0] > 0.0 and out[0] > 0.0
        after = state(ctx, gname, g)[0].reshape(g["R"].shape)
        keep = np.arange(g["a"].size) != row
        np.testing.assert_array_equal(after[keep], before[0].reshape(g["R"].shape)[keep])
        assert np.any(after[row] != before[0].reshape(g["R"].shape)[row])
    finally:
        ctx.close()


@pytest.mark.parametrize("count", [1, 64, 65])
def test_counts_around_a_wavefront(fx, count):
    """a sparse batch of `count` swaps over the product group's pools, rows repeating (several waves), against the twin"""
    g = P.group(fx, "product")
    ctx, twin = fresh(fx, "product"), fresh(fx, "product")
    try:
        m = g["a"].size
        idx = (np.arange(count, dtype=np.int64) * 5) % m
        ci = g["cin"][idx].astype(np.int32)
        lim = 0.95 * ctx.quote_rate(0, None, ci, None, idx, want_out=False)[1]
        amount = np.where(np.arange(count) % 3 == 0, INF, 1e-3 * g["R"][idx, ci])
        used, out, status = ctx.swap_limit(0, amount, lim, ci, None, idx)
        for q in range(count):   # the twin one swap at a time: the caller's order
            one = (ci[q:q + 1], None, idx[q:q + 1])
            a = min(amount[q], twin.quote_to_rate(0, lim[q:q + 1], *one, want_out=False)[0][0])
            o = twin.swap(0, np.array([a]), *one)[0]
            assert bits(used[q]) == bits(a) and bits(out[q]) == bits(o), q
        np.testing.assert_array_equal(state(ctx, "product", g)[0], state(twin, "product", g)[0])
        assert ctx.get_option("swap_launches") == int(np.max(np.bincount(idx)))
    finally:
        ctx.close()
        twin.close()


def test_univ3_across_a_tick_boundary_and_into_an_empty_ticks_range(fx):
    """Limits from the 80-digit fixture that lie beyond the current tick (depth 1 and 4) and inside an empty tick's range: the
    swap takes the fixture's amount, the pool rests at the limit price -- where cfmm_pools_set_prices at the price it reports
    puts a twin, quote for quote -- or, in an empty range, at the live tick behind it; and the solver still runs."""
    fxs = TP.load()
    t = TP.group(fxs, "univ3")
    g = P.group(fx, "univ3")
    npools = g["current_price"].size
    seen = set()
    for cls in ("depth1", "depth4", "empty_in_path"):
        rows = np.flatnonzero(t["cls"] == cls)
        assert rows.size > 0, cls
        for j in rows[:2]:
            p, c_in, r = int(t["pool"][j]), int(t["cin"][j]), float(t["r"][j])
            seen.add(cls)
            ctx, twin = fresh(fx, "univ3"), fresh(fx, "univ3")
            try:
                q1 = (np.array([c_in], dtype=np.int32), None, np.array([p], dtype=np.int64))
                used, out, status = ctx.swap_limit(0, np.array([INF]), np.array([r]), *q1)
                K = TP.K_of("univ3", cls)
                assert status[0] == cr.LIMIT_PARTIAL
                assert abs(used[0] - t["a"][j]) <= K * TP.U * (t["a"][j] + t["cond"][j])
                price = ctx.prices(0, npools)
                gamma = float(g["pool_gamma"][p])
                spot = ctx.quote_rate(0, None, *q1, want_out=False)[1][0]
                if cls == "empty_in_path":
                    assert spot < r                                          # the live tick behind the empty range
                else:
                    want = r / gamma if c_in == 0 else gamma / r             # rate = γ·price (coin 0 in), γ/price (coin 1 in)
                    assert abs(price[p] - want) <= 1e-12 * want and abs(spot - r) <= 1e-12 * r
                twin.set_prices(0, np.array([p], dtype=np.int64), price[p:p + 1])
                np.testing.assert_array_equal(bits(twin.prices(0, npools)), bits(price))
                for a, b in zip(probes(ctx, "univ3", g), probes(twin, "univ3", g)):
                    np.testing.assert_array_equal(a, b)
                again = ctx.swap_limit(0, np.array([INF]), np.array([r * (1.0 + 2.0 ** -30)]), *q1)
                assert again[2][0] == cr.LIMIT_NONE
                psi, _ = ctx.eval(np.ones(N_TOKENS))                           # the sweep runs on the moved pool
                assert np.all(np.isfinite(psi))
            finally:
                ctx.close()
                twin.close()
    assert seen == {"depth1", "depth4", "empty_in_path"}


def test_router_swap_limit_and_amount_to_rate(fx):
    """the router's calls: tokens map to coins, the host mirror follows, a following route_ runs"""
    pools = [cr.ProductTwoCoin([1e6, 2e6], 0.997, [1, 2]), cr.ProductTwoCoin([3e5, 1e5], 0.997, [2, 3]),
             cr.ProductTwoCoin([1e6, 1e6], 0.997, [1, 3])]
    r = cr.Router(cr.LinearNonnegative(np.ones(3)), pools, 3)
    spot = cr.spot_price(r, [0], 1)[0]                                      # pool 0: coin 1 (token 2) in
    amt, out = cr.amount_to_rate(r, [0], 2, 1, 0.9 * spot)
    assert amt[0] > 0.0 and out[0] > 0.0
    np.testing.assert_array_equal(bits(out), bits(cr.quote(r, [0], 1, amt)))
    used, got, status = cr.swap_limit_(r, [0, 1], [2, 2], [1, 3], [INF, 1.0], [0.9 * spot, 0.0])
    assert status.tolist() == [cr.LIMIT_PARTIAL, cr.LIMIT_FILLED] and bits(used[0]) == bits(amt[0]) and bits(got[0]) == bits(out[0])
    np.testing.assert_allclose(r.cfmms[0].R, [1e6 - out[0], 2e6 + 0.997 * amt[0]], rtol=1e-15)
    assert abs(cr.spot_price(r, [0], 1)[0] - 0.9 * spot) <= 1e-12 * spot
    with pytest.raises(cr.ArgumentError, match="not a coin of pool 0"):
        cr.amount_to_rate(r, [0], 3, 1, 1.0)
    with pytest.raises(cr.ArgumentError, match="both sides"):
        cr.swap_limit_(r, [0], 1, 1, 1.0, 1.0)
    cr.route_(r)
    assert np.all(np.isfinite(cr.netflows(r)))


def repeated_batch(gname, g, ctx):
    """seven swaps over four rows of both halves of the segment, the first row named three times and the last one twice:
    (idx, coin_in, coin_out or None, amounts, limits) -- half the way to 0.9 of the spot rate, then as much as it takes"""
    idx0, ci0, co0, fallback = one_per_pool(gname, g)
    m = idx0.size
    idx = np.array([0, m - 1, m // 2, 0, m - 1, 1, 0], dtype=np.int64)
    ci = ci0[idx]
    co = None if co0 is None else co0[idx]
    spot = ctx.quote_rate(0, None, ci, co, idx, want_out=False)[1]
    lim = 0.9 * spot
    a0 = ctx.quote_to_rate(0, lim, ci, co, idx, want_out=False)[0]
    amount = np.array([0.5, INF, 0.25, INF, INF, 0.0, INF]) * np.where(a0 > 0.0, a0, 1.0)
    lim[5] = 0.0                                                           # one swap without a limit (and nothing to tender)
    amount[5] = fallback[1]
    return idx, ci, co, amount, lim


@pytest.mark.parametrize("gname", P.GROUPS)
def test_a_multi_device_parent_behaves_as_a_single_device(fx, gname):
    """a two-device-id context on one GPU: a sparse batch that spans both shards and names rows several times gives the bits of
    the single-device context -- used, out, status, the whole segment's state -- also when the caller wants no status"""
    from cfmmrouter_amd._lib import ptr
    g = P.group(fx, gname)
    one = fresh(fx, gname)
    multi, blind = cr.Context(N_TOKENS, [0, 0]), cr.Context(N_TOKENS, [0, 0])
    try:
        upload(multi, gname, g)
        upload(blind, gname, g)
        idx, ci, co, amount, lim = repeated_batch(gname, g, one)
        want = one.swap_limit(0, amount, lim, ci, co, idx)
        got = multi.swap_limit(0, amount, lim, ci, co, idx)
        for a, b in zip(got[:2], want[:2]):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(got[2], want[2])
        assert {cr.LIMIT_FILLED, cr.LIMIT_PARTIAL} <= set(want[2].tolist())
        assert want[0][3] > 0.0 and want[0][6] <= 2.0 ** -40 * want[0][3]   # row 0: the second swap saw the first, the third finds the pool at the limit
        np.testing.assert_array_equal(state(multi, gname, g)[0], state(one, gname, g)[0])
        for a, b in zip(probes(multi, gname, g), probes(one, gname, g)):
            np.testing.assert_array_equal(a, b)
        assert multi.get_option("swap_refused") == one.get_option("swap_refused")
        # status == NULL on the parent
        n = idx.size
        used, out = np.full(n, -1.0), np.full(n, -1.0)
        cin, cout = np.ascontiguousarray(ci, dtype=np.int32), None if co is None else np.ascontiguousarray(co, dtype=np.int32)
        blind._check(blind._L.cfmm_swap_limit(blind._h, 0, n, ptr(idx), ptr(cin), ptr(cout), ptr(np.ascontiguousarray(amount)),
                                              ptr(np.ascontiguousarray(lim)), ptr(used), ptr(out), None))
        np.testing.assert_array_equal(bits(used), bits(want[0]))
        np.testing.assert_array_equal(bits(out), bits(want[1]))
        np.testing.assert_array_equal(state(blind, gname, g)[0], state(one, gname, g)[0])
        # the checks are the parent's own: refused before any shard moves
        before = state(multi, gname, g)[0]
        with pytest.raises(cr.ArgumentError, match="cfmm_swap_limit: query 1: rate_limit must be finite and >= 0"):
            multi.swap_limit(0, np.array([amount[0], amount[0]]), np.array([lim[0], -1.0]), ci[:2], None if co is None else co[:2], idx[:2])
        with pytest.raises(cr.ArgumentError, match="cfmm_swap_limit: query 0: amount_in must be finite and >= 0"):
            multi.swap_limit(0, np.array([INF]), np.array([0.0]), ci[:1], None if co is None else co[:1], idx[:1])
        np.testing.assert_array_equal(state(multi, gname, g)[0], before)
    finally:
        one.close()
        multi.close()
        blind.close()


def test_univ3_a_refused_landing_price_moves_nothing_and_unnamed_pools_keep_every_bit(fx):
    """UniV3's refusal is the host's: an amount that drives the price of the last tick (δmax = inf) to 0 lands on a price no pool
    can take -- used and out NaN, CFMM_LIMIT_REFUSED, every pool where it was; then one applied swap moves its pool alone"""
    g = P.group(fx, "univ3")
    ctx = fresh(fx, "univ3")
    try:
        before, probed = state(ctx, "univ3", g), probes(ctx, "univ3", g)
        idx, ci = np.array([0, 1], dtype=np.int64), np.array([0, 0], dtype=np.int32)
        used, out, status = ctx.swap_limit(0, np.array([1e300, 1.0]), np.array([0.0, 1e300]), ci, None, idx)
        assert status[0] == cr.LIMIT_REFUSED and np.isnan(used[0]) and np.isnan(out[0])
        assert status[1] == cr.LIMIT_NONE and bits(used[1]) == 0 and bits(out[1]) == 0
        assert ctx.get_option("swap_refused") == 1
        for a, b in zip(before + tuple(probed), state(ctx, "univ3", g) + tuple(probes(ctx, "univ3", g))):
            np.testing.assert_array_equal(a, b)
        lim = 0.9 * ctx.quote_rate(0, None, ci[:1], None, idx[:1], want_out=False)[1]
        used, out, status = ctx.swap_limit(0, np.array([INF]), lim, ci[:1], None, idx[:1])
        assert status[0] == cr.LIMIT_PARTIAL and used[0] > 0.0 and out[0] > 0.0
        after = state(ctx, "univ3", g)[0]
        np.testing.assert_array_equal(after[1:], before[0][1:])
        assert after[0] != before[0][0]
    finally:
        ctx.close()


def test_router_univ3_limit_across_ticks_then_route(fx):
    """the router's call on a UniV3 pool, the limit two tick boundaries away: the host mirror follows the device to the limit
    price, and a following route_ runs on the moved market"""
    pools = [cr.UniV3(1.04, [1.21, 1.1, 1.0, 0.9, 0.8], [2e11, 3e11, 4e11, 3e11, 2e11], 0.997, [1, 2]),
             cr.ProductTwoCoin([1e6, 1e6], 0.997, [1, 2])]
    r = cr.Router(cr.LinearNonnegative(np.ones(2)), pools, 2)
    spot = cr.spot_price(r, [0], 0)[0]
    limit = 0.85 * spot                                                    # price 1.04 -> 0.884: past the ticks at 1.0 and 0.9
    room, _ = cr.amount_to_rate(r, [0], 1, 2, limit)
    used, out, status = cr.swap_limit_(r, [0], 1, 2, INF, limit)
    assert status[0] == cr.LIMIT_PARTIAL and bits(used[0]) == bits(room[0]) and out[0] > 0.0
    assert abs(r.cfmms[0].current_price - limit / 0.997) <= 1e-12 * limit and r.cfmms[0].current_price < 0.9
    assert abs(cr.spot_price(r, [0], 0)[0] - limit) <= 1e-12 * limit
    cr.route_(r)
    assert np.all(np.isfinite(cr.netflows(r)))
