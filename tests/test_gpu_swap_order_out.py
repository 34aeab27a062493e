"""cfmm_swap_order_out on the device: exact-output orders of 1 .. 8 paths EXECUTED in the caller's order, each all or nothing across
its paths, with one limit on the order's total input.  No tolerance anywhere: amounts, hop amounts and states are held to
cfmm_swap_path_out on the flat paths on a twin context, totals to the serial sum and to cfmm_split_paths_out's total_in.
test_gpu_swap_order's market and orders; the wanted amounts are a part of what the forward walk of each path yields on the
standing market, so that every hop can give what it is asked for."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import (ORDER_APPLIED, ORDER_LIMIT, ORDER_PATH_HELD, ORDER_REFUSED, ORDER_UNOBTAINABLE, PATH_APPLIED, SPLIT_OK,
                                 SWAP_APPLIED, SWAP_REFUSED, SWAP_UNOBTAINABLE)
from test_gpu_quote_path import bits, same_bits, scale_in, used_slots
from test_gpu_quote_path import market as standing_market
from test_gpu_split_paths_out import make_orders_out
from test_gpu_swap import backend
from test_gpu_swap_order import (COUNTS, KS, M_ORDERS, ORDER_SEED, chained_orders, disjoint_orders, order_waves, serial_totals, take_orders)
from test_gpu_swap_path import explicit, market, same_states, sliced, states
from test_gpu_swap_path_out import EDGE, THIN, TINY, doctored_market

pytestmark = pytest.mark.gpu


def run(ctx, first, paths, want, limit=None, hops=True):
    return ctx.swap_order_out(first, *paths[:5], want, max_total_in=limit, hops=hops)


# ---- 1. one wave equals swap_path_out ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_wave():
    """the market, the 65 pool-disjoint orders and half of what each path yields forward: computed once, left unchanged"""
    batches = market(m=M_ORDERS, seed=ORDER_SEED)
    first, paths = disjoint_orders(batches, max(COUNTS))
    be = backend(batches)
    try:
        fwd = be.ctx.quote_path(*paths)
    finally:
        be.close()
    return batches, first, paths, 0.5 * fwd


@pytest.mark.parametrize("count", COUNTS)
def test_one_wave_equals_swap_path_out_on_the_flat_paths(one_wave, count):
    batches, first_all, paths_all, want_all = one_wave
    first = first_all[:count + 1]
    n = int(first[-1])
    paths, want = sliced(paths_all, slice(0, n)), want_all[:n]
    assert np.all(np.isfinite(want)) and np.sum(want == 0.0) <= n // 20
    assert sorted(set(np.diff(first).tolist())) == sorted(set(KS[:count]))
    twin = backend(batches)
    try:
        cost, cost_st, cost_hops = twin.ctx.swap_path_out(*paths[:5], want, hops=True)
        want_states = states(twin.ctx, batches)
    finally:
        twin.close()
    print(f"one wave: {n} paths, {int(np.sum(cost_st != SWAP_APPLIED))} not applied, {int(np.sum(cost == 0.0))} cost exactly 0.0")
    assert np.all(cost_st == SWAP_APPLIED) and np.sum(cost == 0.0) <= n // 20
    used = used_slots(paths[0], cost_hops.shape[0])
    for blocks in (None, 1):
        be = backend(batches)
        try:
            ctx = be.ctx
            if blocks is not None:
                ctx.set_option("order_max_blocks", blocks)
            got, total, status, pst, hops = run(ctx, first, paths, want)
            assert np.all(status == ORDER_APPLIED) and np.all(pst == PATH_APPLIED)
            assert ctx.get_option("swap_refused") == 0 and ctx.get_option("swap_launches") == 1
            same_bits(got, cost, "path_amount_in")
            same_bits(hops[used], cost_hops[used], "hop_in")
            assert np.all(np.isnan(hops[~used]))
            same_bits(total, serial_totals(first, cost), "total_in")
            same_states(states(ctx, batches), want_states, f"final state (order_max_blocks {blocks})")
        finally:
            be.close()


# ---- 2. the total is the split's --------------------------------------------------------------------------------------------------
def test_the_total_is_the_splits_and_one_ulp_less_is_the_limit():
    batches = standing_market()
    first, amount, n_hops, seg, row, ci, co = make_orders_out(batches, "interleaved", 8, first_k=4, u=-3.0)   # K = 1, 2, 3, 8, 1, 2, 3, 8
    be, held = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        x, c, total, st = ctx.split_paths_out(first, amount, n_hops, seg, row, ci, co)
        good = np.flatnonzero((st == SPLIT_OK) & (total > 0))
        print(f"split statuses {st.tolist()}; orders executed {good.tolist()}")
        assert good.size >= 4 and len(set(np.diff(first)[good].tolist())) >= 3
        f, paths = take_orders(first, (n_hops, seg, row, ci, co, x), good)
        shares = paths[5]
        costs = np.concatenate([c[first[g]:first[g + 1]] for g in good])
        was = states(held.ctx, batches)
        got, tot, status, pst, hops = run(held.ctx, f, paths, shares, limit=np.nextafter(total[good], 0.0))
        assert np.all(status == ORDER_LIMIT) and np.all(pst == ORDER_PATH_HELD)
        same_bits(tot, total[good], "the total of an order over its limit is the sum")
        same_bits(got, costs, "the inputs are still the quotes")
        same_states(states(held.ctx, batches), was, "an order over its limit moves no bit")
        got, tot, status, pst, hops = run(ctx, f, paths, shares, limit=total[good])
        assert np.all(status == ORDER_APPLIED) and np.all(pst == PATH_APPLIED)
        same_bits(tot, total[good], "total_in is cfmm_split_paths_out's total_in")
        same_bits(got, costs, "path_amount_in")
        assert any(np.any(bits(a) != bits(b)) for a, b in zip(states(ctx, batches), was))
    finally:
        be.close()
        held.close()


# ---- 5. exact output: unobtainable, refused, and what only a split can fill --------------------------------------------------------
@pytest.mark.parametrize("case", ("unobtainable", "refused", "both"))
def test_a_path_that_fails_leaves_its_sibling_paths_unapplied(case):
    batches, o_edge = doctored_market()
    cannot = [(1, 5, 0, 1), (0, TINY, 0, 1), (4, 2, 0, 2)]                      # TINY cannot give what the weighted pool asks of it
    refuses = [(1, 6, 0, 1), (2, THIN, 0, 1), (0, EDGE, 0, 1)]                  # THIN would be left outside Solidly's window
    sib_a, sib_c = [(0, 1, 0, 1), (5, 2, 0, 3)], [(6, 5, 1, 0), (5, 3, 1, 6)]
    ordinary = [(0, 2, 0, 1), (4, 9, 0, 2)]
    probe = backend(batches)
    try:
        def feasible(path):
            s0, r0, c0, _ = path[0]
            return 0.25 * probe.ctx.quote_path(*explicit([path], [1e-3 * scale_in(batches[s0])[r0, c0]]))[0]
        w_a, w_c, w_o = feasible(sib_a), feasible(sib_c), feasible(ordinary)
    finally:
        probe.close()
    assert min(w_a, w_c, w_o) > 0
    middle = {"unobtainable": [cannot], "refused": [refuses], "both": [cannot, refuses]}[case]
    w_mid = {"unobtainable": [1e-3 * batches[4].R[2, 2]], "refused": [o_edge], "both": [1e-3 * batches[4].R[2, 2], o_edge]}[case]
    flat = [sib_a] + middle + [sib_c, ordinary]
    paths = explicit(flat, [w_a] + w_mid + [w_c, w_o])
    want = paths[5]
    K = len(middle) + 2
    first = np.array([0, K, K + 1], dtype=np.int64)
    be, twin, old = backend(batches), backend(batches), backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        got, total, status, pst, hops = run(ctx, first, paths, want)
        code = {"unobtainable": ORDER_UNOBTAINABLE, "refused": ORDER_REFUSED, "both": ORDER_REFUSED}[case]   # refused > unobtainable
        assert status.tolist() == [code, ORDER_APPLIED] and ctx.get_option("swap_refused") == 1
        mid_st = {"unobtainable": [SWAP_UNOBTAINABLE], "refused": [SWAP_REFUSED], "both": [SWAP_UNOBTAINABLE, SWAP_REFUSED]}[case]
        assert pst.tolist() == [ORDER_PATH_HELD] + mid_st + [ORDER_PATH_HELD, PATH_APPLIED]
        assert (np.isposinf(total[0]) if case == "unobtainable" else np.isnan(total[0])) and np.isfinite(total[1])
        for j, s_ in enumerate(mid_st):
            assert np.isposinf(got[1 + j]) if s_ == SWAP_UNOBTAINABLE else np.isnan(got[1 + j])
        # the held paths answer what swap_path_out quotes for them, and the market is the one on which only the last order ran
        o_got, o_st = old.ctx.swap_path_out(*paths[:5], want)
        assert o_st.tolist() == [SWAP_APPLIED] + mid_st + [SWAP_APPLIED, SWAP_APPLIED]      # today's behaviour: the siblings are applied
        same_bits(got[[0, K - 1]], o_got[[0, K - 1]], "the held paths' quotes")
        f2, p2 = take_orders(first, paths, [1])
        w = run(twin.ctx, f2, p2, p2[5])
        assert w[2].tolist() == [ORDER_APPLIED]
        same_bits(got[K:], w[0])
        same_bits(total[1:], w[1])
        same_states(states(ctx, batches), states(twin.ctx, batches), "the failing order moved nothing")
        moved = states(old.ctx, batches)
        assert all(np.any(bits(moved[s][r]) != bits(was[s][r])) for s, r in ((0, 1), (5, 2), (6, 5), (5, 3)))
    finally:
        be.close()
        twin.close()
        old.close()


def test_three_paths_fill_an_order_that_every_single_path_answers_inf_for():
    """split_paths_out's own case, executed: B = 1.5 R from three equal pools of reserve R"""
    R, g_ = 1.0e5, 0.997
    make = lambda: cr.Router(cr.LinearNonnegative(np.ones(2)), [cr.ProductTwoCoin([R, R], g_, [1, 2]) for _ in range(3)], 2)
    r, twin = make(), make()
    try:
        pools, toks = [[0], [1], [2]], [[1, 2]] * 3
        B = 1.5 * R
        assert np.all(np.isposinf(cr.quote_path_out(r, pools, toks, B)))
        x, c, total, st = cr.split_paths_out(r, [pools], [toks], B)
        assert st[0] == cr.SPLIT_OK and np.isfinite(total[0]) and np.all(x[0] < R)
        # a whole-order limit one ulp below the cost holds everything; the cost itself applies
        got, tot, status, pst = cr.swap_order_out_(r, [pools], [toks], x, max_total_in=np.nextafter(total[0], 0.0))
        assert status.tolist() == [cr.ORDER_LIMIT] and pst[0].tolist() == [cr.ORDER_PATH_HELD] * 3
        assert all(np.array_equal(p.R, [R, R]) for p in r.cfmms)
        got, tot, status, pst = cr.swap_order_out_(r, [pools], [toks], x, max_total_in=total[0])
        assert status.tolist() == [cr.ORDER_APPLIED] and pst[0].tolist() == [PATH_APPLIED] * 3
        same_bits(tot, total)
        same_bits(got[0], c[0])
        cost, cost_st = cr.swap_path_out_(twin, pools, toks, x[0], max_in=c[0])
        assert np.all(cost_st == SWAP_APPLIED)
        for a, b in zip(r.cfmms, twin.cfmms):
            same_bits(a.R, b.R)
        assert all(p.R[1] < R for p in r.cfmms)
    finally:
        r.close()
        twin.close()


# ---- 4. orders that share pools -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("univ3", (False, True), ids=("no_univ3", "univ3"))
def test_orders_that_share_pools_equal_one_order_per_call(univ3):
    m, count = 32, 60
    batches = market(m=m, seed=62, univ3=univ3)
    first, paths = chained_orders(batches, count, m, seed=62)
    waves = order_waves(first, paths)
    assert waves > 10
    limit = np.where(np.arange(count) % 3 == 1, 0.0, 1e300)                     # every third order may cost nothing: over its limit
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        want = 0.25 * twin.ctx.quote_path(*paths)                               # (on the standing market)
        got, total, status, pst, hops = run(ctx, first, paths, want, limit=limit)
        print(f"shared pools: {waves} waves; statuses {np.bincount(status, minlength=4).tolist()}")
        assert ctx.get_option("swap_launches") == waves and ctx.get_option("swap_refused") == np.sum(status != ORDER_APPLIED)
        assert np.sum(status == ORDER_APPLIED) >= count // 2 and np.sum(status == ORDER_LIMIT) >= count // 4
        for g in range(count):
            f1, p1 = take_orders(first, paths, [g])
            sl = slice(first[g], first[g + 1])
            g1, t1, s1, ps1, h1 = run(twin.ctx, f1, p1, want[sl], limit=limit[g:g + 1])
            assert s1[0] == status[g], g
            np.testing.assert_array_equal(ps1, pst[sl])
            same_bits(g1, got[sl], f"order {g}: path_amount_in")
            same_bits(t1, total[g:g + 1], f"order {g}: total_in")
            use = used_slots(p1[0], h1.shape[0])
            same_bits(h1[use], hops[:h1.shape[0], sl][use], f"order {g}: hop_in")
        same_states(states(ctx, batches), states(twin.ctx, batches), "final state")
    finally:
        be.close()
        twin.close()


def test_bad_input_is_named_as_the_exact_output_entry_names_it():
    batches = market(m=32, seed=48)
    be = backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        order = [[(0, 1, 0, 1), (4, 2, 0, 2)], [(1, 4, 0, 1)], [(6, 5, 1, 0), (0, 1, 1, 0)]]
        first = np.array([0, 3], dtype=np.int64)
        with pytest.raises(cr.ArgumentError, match=r"cfmm_swap_order_out: order 0: paths 0 and 2 share pool \(segment 0, row 1\)"):
            run(ctx, first, explicit(order, [1.0, 1.0, 1.0]), np.ones(3))
        ok = explicit(order[:2], [1.0, 1.0])
        with pytest.raises(cr.ArgumentError, match="cfmm_swap_order_out: order 0: path 1, hop 0: amount_out must be finite and >= 0"):
            run(ctx, np.array([0, 2], dtype=np.int64), ok, np.array([1e-6, -1.0]))
        with pytest.raises(cr.ArgumentError, match="cfmm_swap_order_out: order 0: max_total_in must be finite and >= 0"):
            run(ctx, np.array([0, 2], dtype=np.int64), ok, np.array([1e-6, 1e-6]), limit=np.inf)
        same_states(states(ctx, batches), was)
    finally:
        be.close()
