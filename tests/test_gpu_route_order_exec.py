"""The router level of order execution: swap_order_ / swap_order_out_ through a Router equal the chain of swap_path_ calls and keep
the host mirror in step; route_order_ / route_order_out_ (find -> split -> execute) apply on the standing market at
max_slippage = 0, and a limit that went stale because another swap moved one of the order's pools gives ORDER_LIMIT with the
market untouched.  Bit equality against calls the project already has; no tolerance."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED, SWAP_APPLIED
from test_gpu_quote_path import bits, same_bits
from test_gpu_swap_path import mixed_pools

pytestmark = pytest.mark.gpu


def five_pools():
    """examples/split_order.py's market: three direct pools 1 -> 2 and the detour 1 -> 3 -> 2"""
    return [cr.ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), cr.ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
            cr.ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]


def router_of(pools, n):
    return cr.Router(cr.LinearNonnegative(np.ones(n)), pools, n)


def mirror_state(r):
    return [np.array([p.current_price]) if isinstance(p, cr.UniV3) else np.array(p.R, copy=True) for p in r.cfmms]


def same_mirror(a, b, what=""):
    for i, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, f"{what} pool {i}")


def test_swap_order_through_a_router_equals_the_chain_of_swap_paths():
    n = 6
    pools = [[[0, 1, 3], [2, 4, 5]], [[3, 5, 4]], [[0]]]                        # order 0: two paths 1 -> 5; order 1 shares pools with it
    tokens = [[[1, 2, 3, 5], [1, 4, 6, 5]], [[3, 5, 6, 4]], [[2, 1]]]
    amounts = [np.array([50.0, 40.0]), np.array([30.0]), np.array([20.0])]
    r, twin = router_of(mixed_pools(), n), router_of(mixed_pools(), n)
    try:
        cr.route_(r, solver="native")
        out, total, status, pst, hops = cr.swap_order_(r, pools, tokens, amounts, min_total_out=0.0, hops=True)
        assert status.tolist() == [cr.ORDER_APPLIED] * 3 and all(np.all(p == PATH_APPLIED) for p in pst)
        assert all(np.all(np.asarray(x) == 0) for x in r.Δs)                    # the old trades are gone
        at = 0
        for g in range(3):
            want, want_st, want_hops = cr.swap_path_(twin, pools[g], tokens[g], amounts[g], hops=True)
            assert np.all(want_st == PATH_APPLIED)
            same_bits(out[g], want, f"order {g}")
            t = np.float64(want[0])
            for y in want[1:]:
                t = t + np.float64(y)
            assert bits(total[g:g + 1])[0] == bits([t])[0]
            for j in range(len(pools[g])):
                k = len(pools[g][j])
                same_bits(hops[:k, at + j], want_hops[:k, j], f"order {g}, path {j}: hop_out")
            at += len(pools[g])
        same_mirror(mirror_state(r), mirror_state(twin), "the host mirror after sync_host")
        ctx, L = r._backend.ctx, r._layout
        for i, pool in enumerate(r.cfmms):                                     # ... and it is the device's state
            _, b, row = L.locate(i)
            s, batch = L.seg_of[b], L.batches[b]
            if isinstance(pool, cr.UniV3):
                assert pool.current_price == ctx.prices(s, len(batch))[row]
            else:
                same_bits(pool.R, ctx.reserves(s, len(batch), len(pool.R))[row])
        # the router's refusals are split_paths' and swap_path_'s
        with pytest.raises(cr.ArgumentError, match="order 0: paths 0 and 1 share pool 3"):
            cr.swap_order_(r, [[[3], [3]]], [[[3, 5], [3, 5]]], 1.0)
        with pytest.raises(cr.ArgumentError, match="path_amount_in must be a scalar or have one entry per path"):
            cr.swap_order_(r, pools, tokens, [np.ones(2), np.ones(2), np.ones(1)])
        with pytest.raises(cr.ArgumentError, match="min_total_out must be a scalar or have one entry per order"):
            cr.swap_order_(r, pools, tokens, amounts, min_total_out=[1.0, 2.0])
        cr.route_(r, solver="native")                                          # ... and the router routes on
    finally:
        r.close()
        twin.close()


def test_route_order_applies_on_the_standing_market_and_a_stale_limit_holds_everything():
    r, moved = router_of(five_pools(), 3), router_of(five_pools(), 3)
    try:
        amount = 1.0e5
        # find -> split -> execute, no slippage allowed: the market has not moved since the split, so the total is met bit for bit
        pools, tokens, x, y, total, st, out, got, status, pst = cr.route_order_(r, 1, 2, amount, max_slippage=0.0, max_paths=8)
        assert st[0] == cr.SPLIT_OK and len(pools[0]) == 4 and status.tolist() == [cr.ORDER_APPLIED]
        assert bits(got)[0] == bits(total)[0] and np.all(pst[0] == PATH_APPLIED)
        same_bits(out[0], y[0])
        assert r.cfmms[0].R[0] > 1.0e5                                         # the host mirror followed
        # the same order on a market one of whose pools an ordinary swap_ has moved since it was routed
        routed = cr.route_order(moved, 1, 2, amount, max_paths=8)
        same_bits(routed[4], total)
        cr.swap_(moved, [routed[0][0][1][0]], [0], [100.0], [1])                 # 100 of token 1 into the second path's first pool
        was = mirror_state(moved)
        out2, got2, status2, pst2 = cr.swap_order_(moved, routed[0], routed[1], routed[2], min_total_out=routed[4])
        assert status2.tolist() == [cr.ORDER_LIMIT] and pst2[0].tolist() == [cr.ORDER_PATH_HELD] * 4
        assert 0 < got2[0] < routed[4][0]
        same_mirror(mirror_state(moved), was, "a stale limit moves nothing:")
        # with half a per cent of slippage allowed the order goes through
        res = cr.route_order_(moved, 1, 2, amount, max_slippage=0.005, max_paths=8)
        assert res[8].tolist() == [cr.ORDER_APPLIED]
        # an order for which nothing is found (here: nothing to sell) is not sent to the device
        none = cr.route_order_(moved, 1, 2, 0.0)
        assert none[0] == [[]] and none[8].tolist() == [cr.ORDER_REFUSED] and none[7][0] == 0.0
        with pytest.raises(cr.ArgumentError, match="max_slippage"):
            cr.route_order_(moved, 1, 2, amount, max_slippage=1.5)
    finally:
        r.close()
        moved.close()


def test_route_order_out_is_the_mirror():
    r, moved = router_of(five_pools(), 3), router_of(five_pools(), 3)
    try:
        want = 1.5e5                                                            # more than the deepest pool holds: no single path can give it
        pools, tokens, x, c, total, st, cost, paid, status, pst = cr.route_order_out_(r, 1, 2, want, max_slippage=0.0)
        assert st[0] == cr.SPLIT_OK and len(pools[0]) >= 3 and status.tolist() == [cr.ORDER_APPLIED]
        assert bits(paid)[0] == bits(total)[0] and np.all(pst[0] == PATH_APPLIED)
        same_bits(cost[0], c[0])
        routed = cr.route_order_out(moved, 1, 2, want)
        same_bits(routed[4], total)
        cr.swap_(moved, [routed[0][0][0][0]], [0], [100.0], [1])                 # the first path's first pool gives up some of token 2
        was = mirror_state(moved)
        cost2, paid2, status2, pst2 = cr.swap_order_out_(moved, routed[0], routed[1], routed[2], max_total_in=routed[4])
        assert status2.tolist() == [cr.ORDER_LIMIT] and np.all(pst2[0] == cr.ORDER_PATH_HELD) and paid2[0] > routed[4][0]
        same_mirror(mirror_state(moved), was, "a stale limit moves nothing:")
        res = cr.route_order_out_(moved, 1, 2, want, max_slippage=0.01)
        assert res[8].tolist() == [cr.ORDER_APPLIED]
        # the exact-output chain through the router equals swap_path_out_ on the shares
        twin = router_of(five_pools(), 3)
        try:
            cr.swap_(twin, [routed[0][0][0][0]], [0], [100.0], [1])
            q = cr.route_order_out(twin, 1, 2, want)
            chain_cost, chain_st = cr.swap_path_out_(twin, q[0][0], q[1][0], q[2][0], max_in=q[3][0])
            assert np.all(chain_st == SWAP_APPLIED)
            same_bits(res[6][0], chain_cost)
            same_mirror(mirror_state(moved), mirror_state(twin), "after the executed order:")
        finally:
            twin.close()
    finally:
        r.close()
        moved.close()
