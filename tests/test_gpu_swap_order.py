"""cfmm_swap_order on the device: orders of 1 .. 8 paths EXECUTED in the caller's order, each all or nothing ACROSS its paths, with
one limit on the order's total.  There is no tolerance anywhere: every comparison is bit equality against calls the project
already has -- the amounts, hop amounts and states against cfmm_swap_path on the flat paths on a twin context, the totals
against the serial sum (numpy's float64 adds, in path order) and against cfmm_split_paths' total_out.  test_gpu_swap_path's
market, helpers and doctored_market; segments of 32 .. 64 pools: every test runs in seconds.

The inputs of the one-wave test must make no path refuse and let at most 5 % of the paths end in exactly 0.0.  The seed was
fixed on the CPU with test_gpu_swap_path's reference_walk: ORDER_SEED 8 refuses none of the 273 paths of the 65 orders and lets
1 end in 0.0 (path 187; seeds 1 .. 7 let two to five, seed 2 refuses one).  The test asserts both on the restatement before the device is asked, and on the device's answers after."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import (OBJ_LINEAR_NONNEGATIVE, ORDER_APPLIED, ORDER_LIMIT, ORDER_PATH_HELD, ORDER_REFUSED, PATH_APPLIED,
                                 PATH_REFUSED, SPLIT_OK, SPLIT_SATURATED, ptr)
from cfmmrouter_amd.cfmms import _upload
from test_gpu_pool_update import assert_same
from test_gpu_quote import N
from test_gpu_quote_path import SEGMENTS, bits, same_bits, scale_in, used_slots
from test_gpu_quote_path import market as standing_market
from test_gpu_split_paths import make_orders
from test_gpu_swap import V, backend
from test_gpu_swap_path import (FUNNEL, THIN, TINY, coins_for, doctored_market, explicit, input_conditions, market, reference_walk,
                                same_states, sliced, states, three_segments)

pytestmark = pytest.mark.gpu

NSEG = len(SEGMENTS)
ORDER_SEED = 8                          # the one-wave market and orders
M_ORDERS = 64                           # pools per segment of that market
KS = (1, 2, 3, 7, 8)                    # paths per order, cycling
COUNTS = (1, 8, 9, 64, 65)              # a lone group, a full wavefront and one more, two blocks and one more (the grid stride)
HOPS = (1, 2, 1, 3, 1)                  # hops per path, cycling (a period that spreads the hops evenly over the eight segments); path 5 of every 64 has eight


def order_first_of(count, ks=KS):
    return np.concatenate(([0], np.cumsum([ks[g % len(ks)] for g in range(count)]))).astype(np.int64)


def disjoint_orders(batches, count, seed=ORDER_SEED, m=M_ORDERS, lo=-4.0, hi=-2.0):
    """-> (order_first, paths): `count` orders of K = 1, 2, 3, 7, 8, ... paths that share no pool at all.  Hop k of path p lies in
    segment (p + 3k) % 8 -- a path never visits a segment twice -- on the next unused row of a permutation of that segment's
    rows; coins cycle through every ordered pair; the first amount is R_in * 10^u, u uniform in [lo, hi]"""
    first = order_first_of(count)
    n = int(first[-1])
    n_hops = np.array([8 if p % 64 == 5 else HOPS[p % len(HOPS)] for p in range(n)], dtype=np.int32)
    Hn = int(n_hops.max())
    p, k = np.meshgrid(np.arange(n), np.arange(Hn), indexing="ij")
    seg = ((p + 3 * k) % NSEG).astype(np.int32)
    perm = [np.argsort(synth.uniform(seed + 400 + s, 6, m)).astype(np.int64) for s in range(NSEG)]
    used = [0] * NSEG
    row = np.zeros((n, Hn), dtype=np.int64)
    for q in range(n):
        for h in range(n_hops[q]):
            s = int(seg[q, h])
            assert used[s] < m, "the market is too small for pool-disjoint orders"
            row[q, h] = perm[s][used[s]]
            used[s] += 1
    ci, co = coins_for(batches, seg, p, k)
    u = lo + (hi - lo) * synth.uniform(seed + 300, 4, n)
    lead = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(n)])
    return first, (n_hops, seg, row, ci, co, lead * 10.0 ** u)


def serial_totals(first, y):
    """y_0 + y_1 + ... per order in increasing path number, the first term taken as it is"""
    out = np.empty(len(first) - 1)
    for g in range(len(first) - 1):
        t = np.float64(y[first[g]])
        for q in range(int(first[g]) + 1, int(first[g + 1])):
            t = t + np.float64(y[q])
        out[g] = t
    return out


def take_orders(first, paths, orders):
    """the orders `orders` of a batch as a batch of their own"""
    idx = np.concatenate([np.arange(first[g], first[g + 1]) for g in orders])
    new_first = np.concatenate(([0], np.cumsum([first[g + 1] - first[g] for g in orders]))).astype(np.int64)
    return new_first, sliced(paths, idx)


def run(ctx, first, paths, limit=None, hops=True):
    return ctx.swap_order(first, *paths, min_total_out=limit, hops=hops)


# ---- 1. one wave equals swap_path -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_wave():
    """the market, the 65 pool-disjoint orders and the restatement's verdict on their paths: computed once, left unchanged"""
    batches = market(m=M_ORDERS, seed=ORDER_SEED)
    first, paths = disjoint_orders(batches, max(COUNTS))
    ref, ref_refused = reference_walk(batches, paths)
    return batches, first, paths, ref, ref_refused


@pytest.mark.parametrize("count", COUNTS)
def test_one_wave_equals_swap_path_on_the_flat_paths(one_wave, count):
    batches, first_all, paths_all, ref_all, refused_all = one_wave
    first = first_all[:count + 1]
    n = int(first[-1])
    paths = sliced(paths_all, slice(0, n))
    ref, ref_refused = ref_all[:n], refused_all[:n]
    print(f"numpy restatement: {int(np.sum(ref_refused))} of {n} paths refused, {int(np.sum(ref == 0.0))} end in exactly 0.0")
    assert not np.any(ref_refused) and np.all(np.isfinite(ref)) and np.all(ref >= 0) and np.sum(ref == 0.0) <= n // 20
    assert sorted(set(np.diff(first).tolist())) == sorted(set(KS[:count])) and (paths[0].max() == 8) == (n > 5)
    twin = backend(batches)
    try:
        want, want_st, want_hops = twin.ctx.swap_path(*paths, hops=True)
        want_states = states(twin.ctx, batches)
    finally:
        twin.close()
    assert np.all(want_st == PATH_APPLIED)
    used = used_slots(paths[0], want_hops.shape[0])
    for blocks in (None, 1):
        be = backend(batches)
        try:
            ctx = be.ctx
            if blocks is not None:
                ctx.set_option("order_max_blocks", blocks)
            out, total, status, path_status, hops = run(ctx, first, paths)
            input_conditions(path_status, out, f"one wave, {count} orders, order_max_blocks {blocks}")
            assert np.all(status == ORDER_APPLIED) and ctx.get_option("swap_refused") == 0 and ctx.get_option("swap_launches") == 1
            same_bits(out, want, "path_amount_out")
            same_bits(hops[used], want_hops[used], "hop_out")
            assert np.all(np.isnan(hops[~used]))
            same_bits(total, serial_totals(first, want), "total_out")
            same_states(states(ctx, batches), want_states, f"final state (order_max_blocks {blocks})")
        finally:
            be.close()
    live = ref > 0
    np.testing.assert_allclose(want[live], ref[live], rtol=1e-6)                 # (the restatement describes these very paths)


def test_the_grid_option_is_checked():
    batches = market(m=32, seed=48)
    be = backend(batches)
    try:
        assert be.ctx.get_option("order_max_blocks") >= 1
        with pytest.raises(cr.ArgumentError, match="order_max_blocks"):
            be.ctx.set_option("order_max_blocks", 0)
    finally:
        be.close()


# ---- 2. the total is the split's --------------------------------------------------------------------------------------------------
def test_the_total_is_the_splits_and_one_ulp_more_is_the_limit():
    """split_paths on a standing market, then swap_order with the split's own total as the limit: APPLIED with the same bits; with
    the next number above it: LIMIT, every path HELD, the outputs still the quotes, no bit of any segment changed"""
    batches = standing_market()
    first, _, n_hops, seg, row, ci, co = make_orders(batches, "interleaved", 8, first_k=4)     # K = 1, 2, 3, 8, 1, 2, 3, 8
    amount = 1e-3 * np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in first[:-1]])
    be, held = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        x, y, total, st = ctx.split_paths(first, amount, n_hops, seg, row, ci, co)
        good = np.flatnonzero(((st == SPLIT_OK) | (st == SPLIT_SATURATED)) & (total > 0))
        print(f"split statuses {st.tolist()}; orders executed {good.tolist()}")
        assert good.size >= 6 and {1, 2, 3, 8} <= set(np.diff(first)[good].tolist())
        f, paths = take_orders(first, (n_hops, seg, row, ci, co, x), good)
        was = states(held.ctx, batches)
        out, tot, status, pst, hops = run(held.ctx, f, paths, limit=np.nextafter(total[good], np.inf))
        assert np.all(status == ORDER_LIMIT) and np.all(pst == ORDER_PATH_HELD) and held.ctx.get_option("swap_refused") == good.size
        same_bits(tot, total[good], "the total of an order that misses its limit is the sum")
        same_bits(out, np.concatenate([y[first[g]:first[g + 1]] for g in good]), "the outputs are still the quotes")
        same_states(states(held.ctx, batches), was, "an order over its limit moves no bit")
        out, tot, status, pst, hops = run(ctx, f, paths, limit=total[good])
        assert np.all(status == ORDER_APPLIED) and np.all(pst == PATH_APPLIED)
        same_bits(tot, total[good], "total_out is cfmm_split_paths' total_out")
        same_bits(out, np.concatenate([y[first[g]:first[g + 1]] for g in good]), "path_amount_out")
        one = np.flatnonzero(np.diff(f) == 1)
        assert one.size >= 1
        same_bits(tot[one], out[f[:-1][one]], "with one path the total is the path's output")
        assert any(np.any(bits(a) != bits(b)) for a, b in zip(states(ctx, batches), was))       # ... and the market has moved
    finally:
        be.close()
        held.close()


# ---- 3. all or nothing across paths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("product", "solidly", "univ3"))
def test_a_refusing_path_leaves_its_sibling_paths_unapplied(case):
    """one order of three paths whose second holds the refusing hop, between two ordinary orders: nothing of it moves -- while
    swap_path on the same flat paths applies the two siblings"""
    batches = doctored_market()
    a = lambda s, r, c: 0.01 * scale_in(batches[s])[r, c]
    first_hop = (3, 4, 0, 1) if case == "univ3" else (1, 5, 0, 1)               # hop 0: a UniV3 pool, or a GeometricMean pool
    last = (2, THIN, 0, 1) if case == "solidly" else (0, TINY, 0, 1)
    refusing = [first_hop, (0, FUNNEL, 0, 1), last]
    sib_a, sib_c = [(0, 1, 0, 1), (4, 2, 0, 2)], [(5, 3, 1, 6), (6, 5, 1, 0)]
    before = [[(0, 2, 0, 1)], [(1, 6, 0, 1), (3, 9, 1, 0)]]                     # an ordinary order of two paths
    after = [[(6, 7, 1, 0), (4, 9, 0, 2)]]                                      # ... and one of one
    flat = before + [sib_a, refusing, sib_c] + after
    amounts = [a(0, 2, 0), a(1, 6, 0), a(0, 1, 0), a(*first_hop[:3]), a(5, 3, 1), a(6, 7, 1)]
    paths = explicit(flat, amounts)
    first = np.array([0, 2, 5, 6], dtype=np.int64)
    be, twin, old = backend(batches), backend(batches), backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        out, total, status, pst, hops = run(ctx, first, paths)
        assert status.tolist() == [ORDER_APPLIED, ORDER_REFUSED, ORDER_APPLIED] and ctx.get_option("swap_refused") == 1
        assert pst.tolist() == [PATH_APPLIED, PATH_APPLIED, ORDER_PATH_HELD, PATH_REFUSED, ORDER_PATH_HELD, PATH_APPLIED]
        assert np.isnan(total[1]) and np.isnan(out[3]) and np.all(out[[2, 4]] > 0) and np.all(np.isfinite(out[[2, 4]]))
        assert np.all(hops[:2, 3] > 0) and np.isnan(hops[2, 3])                  # NaN from the refusing hop on
        # the market equals the twin's, on which only the two other orders ran
        f2, p2 = take_orders(first, paths, [0, 2])
        w_out, w_total, w_status, w_pst, w_hops = run(twin.ctx, f2, p2)
        assert np.all(w_status == ORDER_APPLIED)
        same_bits(out[[0, 1, 5]], w_out, "the other orders' paths")
        same_bits(total[[0, 2]], w_total, "the other orders' totals")
        same_states(states(ctx, batches), states(twin.ctx, batches), "the refused order moved nothing")
        for s, r in ((0, 1), (4, 2), (5, 3), (6, 5)):                          # in particular the siblings' pools
            same_bits(states(ctx, batches)[s][r], was[s][r], f"sibling pool ({s}, {r})")
        # the contrast, today's behaviour unchanged: swap_path on the same flat paths applies the two siblings
        o_out, o_status = old.ctx.swap_path(*paths)
        assert o_status.tolist() == [PATH_APPLIED, PATH_APPLIED, PATH_APPLIED, PATH_REFUSED, PATH_APPLIED, PATH_APPLIED]
        same_bits(o_out[[2, 4]], out[[2, 4]], "the siblings' quotes")
        moved = states(old.ctx, batches)
        assert all(np.any(bits(moved[s][r]) != bits(was[s][r])) for s, r in ((0, 1), (4, 2), (5, 3), (6, 5)))
    finally:
        be.close()
        twin.close()
        old.close()


# ---- 4. orders that share pools run in the caller's order -------------------------------------------------------------------------
def chained_orders(batches, count, m, seed):
    """`count` orders of K = 1, 2, 3, ... paths.  Order g's first path starts at the chain pool (segment 3g % 8, row g % 8) and
    its last path ends at order g + 1's chain pool, so every order shares a pool with its predecessor; the other hops (one per
    path) fall on rows 8 .. m - 1 drawn at random, so orders far apart share pools too.  Inside an order no pool occurs twice."""
    ks = (1, 2, 3)
    first = order_first_of(count, ks)
    chain = lambda g: ((3 * g) % NSEG, g % 8)
    draw = synth.uniform(seed + 700, 5, 64 * count)
    flat, at = [], 0
    for g in range(count):
        K = ks[g % len(ks)]
        taken = {chain(g), chain(g + 1)}
        for k in range(K):
            while True:
                free = (int(draw[at] * NSEG) % NSEG, 8 + int(draw[at + 1] * (m - 8)) % (m - 8))
                at += 2
                if free not in taken:
                    break
            taken.add(free)
            flat.append(([chain(g)] if k == 0 else []) + [free] + ([chain(g + 1)] if k == K - 1 else []))
    n = len(flat)
    Hn = max(len(p) for p in flat)
    n_hops = np.array([len(p) for p in flat], dtype=np.int32)
    seg, row = np.zeros((n, Hn), dtype=np.int32), np.zeros((n, Hn), dtype=np.int64)
    for q, path in enumerate(flat):
        for h, (s_, r_) in enumerate(path):
            seg[q, h], row[q, h] = s_, r_
    p, k = np.meshgrid(np.arange(n), np.arange(Hn), indexing="ij")
    ci, co = coins_for(batches, seg, p, k)
    u = -5.0 + 1.5 * synth.uniform(seed + 300, 4, n)
    lead = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(n)])
    return first, (n_hops, seg, row, ci, co, lead * 10.0 ** u)


def order_waves(first, paths):
    """the planner's rule (csrc/swap_order_waves.h), restated"""
    n_hops, seg, row = paths[:3]
    free, waves = {}, 0
    for g in range(len(first) - 1):
        named = [(int(seg[q, k]), int(row[q, k])) for q in range(first[g], first[g + 1]) for k in range(n_hops[q])]
        assert len(set(named)) == len(named)
        w = max(free.get(x, 0) for x in named)
        for x in named:
            free[x] = w + 1
        waves = max(waves, w + 1)
    return waves


@pytest.mark.parametrize("univ3", (False, True), ids=("no_univ3", "univ3"))
def test_orders_that_share_pools_equal_one_order_per_call(univ3):
    m, count = 32, 60
    batches = market(m=m, seed=62, univ3=univ3)
    first, paths = chained_orders(batches, count, m, seed=62)
    waves = order_waves(first, paths)
    assert waves > 10
    # every third order has a limit no output can meet
    limit = np.where(np.arange(count) % 3 == 1, 1e300, 0.0)
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        out, total, status, pst, hops = run(ctx, first, paths, limit=limit)
        print(f"shared pools: {waves} waves; statuses {np.bincount(status, minlength=4).tolist()}; {int(np.sum(out == 0.0))} of {out.size} paths end in 0.0")
        assert ctx.get_option("swap_launches") == waves and ctx.get_option("swap_ns") > 0
        assert ctx.get_option("swap_refused") == np.sum(status != ORDER_APPLIED)
        assert np.sum(status == ORDER_APPLIED) >= count // 2 and np.sum(status == ORDER_LIMIT) >= count // 4
        for g in range(count):
            f1, p1 = take_orders(first, paths, [g])
            o1, t1, s1, ps1, h1 = run(twin.ctx, f1, p1, limit=limit[g:g + 1])
            sl = slice(first[g], first[g + 1])
            assert s1[0] == status[g], g
            np.testing.assert_array_equal(ps1, pst[sl])
            same_bits(o1, out[sl], f"order {g}: path_amount_out")
            same_bits(t1, total[g:g + 1], f"order {g}: total_out")
            use = used_slots(p1[0], h1.shape[0])
            same_bits(h1[use], hops[:h1.shape[0], sl][use], f"order {g}: hop_out")
        same_states(states(ctx, batches), states(twin.ctx, batches), "final state")
    finally:
        be.close()
        twin.close()


def test_the_limit_stops_the_second_execution_of_an_order():
    batches = market(m=32, seed=44)
    order = [[(0, 3, 0, 1), (3, 7, 1, 0)], [(6, 2, 1, 0), (1, 9, 0, 1)]]
    amounts = [0.001 * batches[0].R[3, 0], 0.001 * batches[6].R[2, 1]]
    one = explicit(order, amounts)
    f1 = np.array([0, 2], dtype=np.int64)
    be, twin = backend(batches), backend(batches)
    try:
        o1, t1, s1, _ = run(twin.ctx, f1, one, hops=False)
        q2 = twin.ctx.quote_path(*one)                                         # what a second execution would give
        t2 = serial_totals(f1, q2)
        assert s1.tolist() == [ORDER_APPLIED] and 0 < t2[0] < t1[0]
        limit = 0.5 * (t1[0] + t2[0])
        assert t2[0] < limit < t1[0]
        twice = explicit(order + order, amounts + amounts)
        out, total, status, pst = run(be.ctx, np.array([0, 2, 4], dtype=np.int64), twice, limit=[limit, limit], hops=False)
        assert status.tolist() == [ORDER_APPLIED, ORDER_LIMIT] and be.ctx.get_option("swap_refused") == 1 and be.ctx.get_option("swap_launches") == 2
        assert pst.tolist() == [PATH_APPLIED, PATH_APPLIED, ORDER_PATH_HELD, ORDER_PATH_HELD]
        same_bits(total, [t1[0], t2[0]])                                       # the second: the quotes on the moved market, summed
        same_bits(out, np.concatenate([o1, q2]))
        same_states(states(be.ctx, batches), states(twin.ctx, batches), "only the first was executed")
        # a limit that is met exactly is met; a scalar serves every order
        o3, t3, s3, _ = run(be.ctx, f1, one, limit=t2[0], hops=False)
        assert s3.tolist() == [ORDER_APPLIED] and bits(t3)[0] == bits(t2)[0]
    finally:
        be.close()
        twin.close()


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------------
def test_zero_amounts_a_zero_path_in_an_applied_order_empty_calls_and_null_outputs():
    batches = market(m=32, seed=48)
    L = cr.lib()
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        every_kind = [[(s, 3 + s, 0, 1) for s in range(4)], [(s, 3 + s, 0, 1) for s in range(4, NSEG)]]
        out, total, status, pst, hops = run(ctx, np.array([0, 2], dtype=np.int64), explicit(every_kind, [0.0, 0.0]), limit=0.0)
        assert status.tolist() == [ORDER_APPLIED] and total[0] == 0.0 and np.all(out == 0.0) and np.all(hops == 0.0) and np.all(pst == PATH_APPLIED)
        same_states(states(ctx, batches), was, "amount 0")
        # a zero-amount path inside an applied order moves no bit of its pools; its sibling moves as swap_path moves it
        order = [[(0, 1, 0, 1), (4, 2, 0, 2)], [(1, 4, 0, 1), (6, 5, 1, 0)]]
        paths = explicit(order, [0.01 * batches[0].R[1, 0], 0.0])
        out, total, status, pst = run(ctx, np.array([0, 2], dtype=np.int64), paths, hops=False)
        want, _ = twin.ctx.swap_path(*paths)
        assert status.tolist() == [ORDER_APPLIED] and out[1] == 0.0 and out[0] > 0
        same_bits(out, want)
        same_bits(total, serial_totals([0, 2], want))
        same_states(states(ctx, batches), states(twin.ctx, batches), "a zero path in an applied order")
        # count == 0 invalidates nothing, through the wrapper and through the library with NULL arrays
        be.find_arb(V)
        trades = [np.array(x, copy=True) for x in be.trades()]
        e = np.zeros((0, 2), dtype=np.int32)
        o, t, s, ps = ctx.swap_order(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), e, e, e, e, np.zeros(0))
        assert o.size == 0 and t.size == 0 and s.size == 0 and ps.size == 0
        ctx._check(L.cfmm_swap_order(ctx._h, 0, None, 0, 2, *([None] * 12)))
        assert_same([np.asarray(x) for x in be.trades()], trades)
        # hop_out, path_status and min_total_out as NULL
        order = [[(0, 6, 0, 1), (5, 2, 0, 3)], [(6, 9, 1, 0)]]
        paths = explicit(order, [0.01 * batches[0].R[6, 0], 0.01 * batches[6].R[9, 1]])
        n_hops, seg, row, ci, co, amt = paths
        c = lambda a: np.ascontiguousarray(a.T)
        got, tot, st = np.full(2, 7.0), np.full(1, 7.0), np.full(1, 7, dtype=np.int32)
        ctx._check(L.cfmm_swap_order(ctx._h, 1, ptr(np.array([0, 2], dtype=np.int64)), 2, 2, ptr(n_hops), ptr(c(seg)), ptr(c(row)), ptr(c(ci)),
                                     ptr(c(co)), ptr(amt), None, ptr(got), None, ptr(tot), None, ptr(st)))
        want, _ = twin.ctx.swap_path(*paths)
        same_bits(got, want)
        same_bits(tot, serial_totals([0, 2], want))
        assert st.tolist() == [ORDER_APPLIED]
        same_states(states(ctx, batches), states(twin.ctx, batches), "NULL outputs")
    finally:
        be.close()
        twin.close()


def orders_of_three_segments():
    """three_segments' 64 paths as 32 orders of two: neighbouring paths visit different rows, and rows shared between orders
    make several waves"""
    batches, paths = three_segments()
    return batches, np.arange(0, 65, 2, dtype=np.int64), paths


def test_large_market_mode_gives_the_same_bits():
    """two-coin segments only (large-market mode has no N-coin kernel), one token moved beyond the LDS limit"""
    from test_gpu_pool_update import batch_with
    small, first, paths = orders_of_three_segments()
    big = [batch_with(b, Ai=np.where(b.Ai == 1, 8193, b.Ai)) for b in small]
    be_s, be_b = cr.DeviceBackend(N, small), cr.DeviceBackend(8193, big)
    try:
        a = run(be_s.ctx, first, paths)
        b = run(be_b.ctx, first, paths)
        assert np.all(a[2] == ORDER_APPLIED) and be_s.ctx.get_option("swap_launches") > 1
        for x, y in zip(a[:4], b[:4]):
            same_bits(y, x)
        use = used_slots(paths[0], 3)
        same_bits(b[4][use], a[4][use])
        same_states(states(be_b.ctx, big), states(be_s.ctx, small))
    finally:
        be_s.close()
        be_b.close()


def test_a_multi_device_parent_is_unsupported_and_moves_nothing():
    batches, first, paths = orders_of_three_segments()
    multi = cr.Context(N, [0, 0])
    try:
        for b in batches:
            _upload(multi, b)
        was = states(multi, batches)
        with pytest.raises(NotImplementedError, match="cfmm_swap_order is not available on a multi-device context"):
            multi.swap_order(first, *paths)
        same_states(states(multi, batches), was)
    finally:
        multi.close()


def test_a_call_invalidates_trades_and_cancels_an_armed_route():
    from test_gpu_swap import assert_equals_fresh, state, with_state
    batches, first, paths = orders_of_three_segments()
    c = synth.linear_prices(N, seed=3)
    be = backend(batches)
    try:
        ctx = be.ctx
        ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N))                 # pre-armed evaluations (option "armed" is on)
        be.find_arb(V)
        be.trades()
        out, total, status, pst = run(ctx, first, paths, hops=False)
        assert np.all(status == ORDER_APPLIED)
        with pytest.raises(Exception, match="no materialised trades"):
            ctx.trades()
        now = [with_state(b, state(ctx, b, s)) for s, b in enumerate(batches)]
        assert_equals_fresh(be, now)                                           # eval, find_arb, trades, state
    finally:
        be.close()


def test_bad_input_names_order_path_and_hop_and_changes_nothing():
    L = cr.lib()
    batches, first, paths = orders_of_three_segments()
    n_hops, seg, row, ci, co, amt = paths
    be = backend(batches)
    try:
        ctx = be.ctx
        be.find_arb(V)
        trades = [np.array(x, copy=True) for x in be.trades()]
        was = states(ctx, batches)
        c = lambda a: np.ascontiguousarray(a.T)

        def refused(match, first=first, seg=seg, row=row, ci=ci, co=co, amt=amt, lim=None):
            G = first.size - 1
            out, hv, pst = np.full(amt.size, 7.0), np.full((3, amt.size), 7.0), np.full(amt.size, 7, dtype=np.int32)
            tot, st = np.full(G, 7.0), np.full(G, 7, dtype=np.int32)
            rc = L.cfmm_swap_order(ctx._h, first.size - 1, ptr(np.ascontiguousarray(first)), amt.size, 3, ptr(n_hops), ptr(c(seg)), ptr(c(row)),
                                   ptr(c(ci)), ptr(c(co)), ptr(np.ascontiguousarray(amt)), ptr(lim), ptr(out), ptr(hv), ptr(tot), ptr(pst), ptr(st))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and msg.startswith("cfmm_swap_order: ") and match in msg, (rc, msg)
            assert np.all(out == 7.0) and np.all(hv == 7.0) and np.all(pst == 7) and np.all(tot == 7.0) and np.all(st == 7)

        def edit(a, p, k, value):
            a = a.copy()
            a[p, k] = value
            return a
        # paths 2 and 3 are order 1's paths 0 and 1; path 5 (order 2, path 1) has 3 hops
        refused("order 2: path 1, hop 2: row 64 out of range (segment 1 has 64 pools)", row=edit(row, 5, 2, 64))
        refused("order 1: path 0, hops 0 and 2: row 9 of segment 2 appears twice", seg=edit(edit(seg, 2, 0, 2), 2, 2, 2), row=edit(edit(row, 2, 0, 9), 2, 2, 9))
        refused("order 0: path 1, hop 0: coin_in 2 out of range", ci=edit(ci, 1, 0, 2))
        bad = amt.copy(); bad[7] = np.nan
        refused("order 3: path 1, hop 0: amount_in must be finite and >= 0", amt=bad)
        lim = np.zeros(first.size - 1); lim[4] = -1.0
        refused("order 4: min_total_out must be finite and >= 0", lim=lim)
        # order 1 made of three paths (2, 3, 4) whose first and third share a pool
        f3 = np.array([0, 2, 5] + list(range(7, 64, 2)) + [64], dtype=np.int64)
        s2, r2 = int(seg[2, 0]), int(row[2, 0])
        assert (int(seg[4, 0]), int(row[4, 0])) != (s2, r2)
        refused(f"order 1: paths 0 and 2 share pool (segment {s2}, row {r2})", first=f3, seg=edit(seg, 4, 0, s2), row=edit(row, 4, 0, r2))
        wrong = first.copy(); wrong[3] = wrong[2] + 9
        refused("order 2: 9 paths (an order has 1 .. 8)", first=wrong)
        assert L.cfmm_swap_order(ctx._h, 1, None, 1, 9, *([None] * 12)) == -1 and "max_hops" in L.cfmm_last_error(ctx._h).decode()
        same_states(states(ctx, batches), was)
        assert_same([np.asarray(x) for x in be.trades()], trades)                # the earlier trades are still readable
    finally:
        be.close()
