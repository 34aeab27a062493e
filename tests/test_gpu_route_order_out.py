"""The router-level exact-output chain on the device: find_disjoint_paths_out -> split_paths_out -> swap_path_out_, and
route_order_out on top, on a market where single paths fail: the default probe (amount_out / max_paths) finds the paths that
probe=amount_out misses, and executing the answer buys exactly the amount."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import FOUND, SPLIT_NONE, SPLIT_OK, SPLIT_UNOBTAINABLE, SWAP_APPLIED
from test_gpu_find_disjoint import five_pools
from test_gpu_quote_path import bits, same_bits

pytestmark = pytest.mark.gpu


def test_router_level_find_split_execute_and_route_order_out():
    r = cr.Router(cr.LinearNonnegative(np.ones(3)), five_pools(), 3)
    try:
        # a small order: every path can give it alone
        B = 1.0e4
        cost, pools, tokens, status = cr.find_disjoint_paths_out(r, [1, 2, 1], [2, 1, 2], [B, 0.0, 1.5e5], max_paths=8, max_hops=3)
        assert {tuple(p) for p in pools[0]} == {(0,), (1,), (2,), (3, 4)} and len(pools[0]) == 4
        assert tokens[0] == [[1, 3, 2] if p == [3, 4] else [1, 2] for p in pools[0]] and status[0].tolist() == [FOUND] * 4
        assert pools[1] == [] and cost[1].size == 0                        # amount 0: nothing found
        assert pools[2] == [] and cost[2].size == 0                        # 150 000: no path can give it alone
        same_bits(cr.quote_path_out(r, pools[0], tokens[0], np.full(4, B)), cost[0], "cr.quote_path_out on cr.find_disjoint_paths_out")
        assert np.all(cost[0][1:] >= cost[0][:-1])
        single, path, _, _ = cr.find_path_out(r, 1, 2, B, max_hops=3)
        assert path[0] == pools[0][0] and bits(single[0]) == bits(cost[0][0])
        x, c, total, st = cr.split_paths_out(r, [pools[0]], [tokens[0]], B)
        assert st.tolist() == [SPLIT_OK] and total[0] < cost[0][0] and abs(np.sum(x[0]) - B) <= 8 * 2.0 ** -53 * B
        routed = cr.route_order_out(r, [1, 2], [2, 1], [B, 0.0], max_paths=8, max_hops=3, probe=[B, 0.0])
        assert routed[0] == [pools[0], []] and routed[1] == [tokens[0], []]
        same_bits(routed[2][0], x[0], "route_order_out's shares")
        same_bits(routed[3][0], c[0], "route_order_out's costs")
        assert bits(routed[4][0]) == bits(total[0]) and not bits(routed[4][1:2])[0] and routed[5].tolist() == [SPLIT_OK, SPLIT_NONE]
        assert routed[2][1].size == 0 and routed[3][1].size == 0
        # a large order: 150 000 of token 2, more than any pool holds.  Probed with the amount nothing is found ...
        big = 1.5e5
        assert np.isposinf(cr.find_path_out(r, 1, 2, big, max_hops=3)[0][0])
        miss = cr.route_order_out(r, 1, 2, big, probe=big)
        assert miss[0] == [[]] and np.isposinf(miss[4][0]) and miss[5].tolist() == [SPLIT_UNOBTAINABLE] and miss[2][0].size == 0
        # ... the default probe, a quarter of it, finds the three paths that can carry a share, and they suffice together
        pools_b, tokens_b, xb, cb, total_b, st_b = cr.route_order_out(r, 1, 2, big)
        assert sorted(pools_b[0]) == [[0], [1], [3, 4]] and st_b.tolist() == [SPLIT_OK] and np.isfinite(total_b[0])
        assert np.all(np.isposinf(cr.quote_path_out(r, pools_b[0], tokens_b[0], np.full(3, big))))   # every single path fails
        assert abs(np.sum(xb[0]) - big) <= 8 * 2.0 ** -53 * big
        same_bits(cr.quote_path_out(r, pools_b[0], tokens_b[0], xb[0]), cb[0], "the costs are quote_path_out's at the shares")
        # more than the found paths hold together: UNOBTAINABLE from split_paths_out
        over = cr.route_order_out(r, 1, 2, 3.0e5, probe=1.0e4)
        assert len(over[0][0]) == 4 and over[5].tolist() == [SPLIT_UNOBTAINABLE] and np.isposinf(over[4][0])
        # executing the answer buys exactly the shares for exactly the costs, and the pools gave exactly the amount
        held = lambda t: np.array([float(np.sum(p.R[np.asarray(p.Ai) == t])) for p in r.cfmms])
        h1, h2 = held(1), held(2)
        paid, applied = cr.swap_path_out_(r, pools_b[0], tokens_b[0], xb[0], max_in=cb[0])
        assert np.all(applied == SWAP_APPLIED)
        same_bits(paid, cb[0], "swap_path_out_ costs what split_paths_out promised")
        assert abs(np.sum(h2 - held(2)) - big) <= 1e-9 * big
        # ... and took what was paid: a pool's reserve grows by γ times what is tendered to it (the fee stays out of the reserve)
        fee = np.array([r.cfmms[p[0]].γ for p in pools_b[0]])
        assert abs(np.sum(held(1) - h1) - np.sum(fee * cb[0])) <= 1e-9 * total_b[0]
        after = cr.route_order_out(r, 1, 2, B, max_paths=8, max_hops=3, probe=B)
        assert after[4][0] > total[0]                                      # the market it left is dearer
    finally:
        r.close()
