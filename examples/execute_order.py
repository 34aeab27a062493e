"""Executing a routed order with ONE slippage limit on its total: 100 000 of token 1 for token 2 on examples/split_order.py's
five-pool market, an order that no single path fills well.

`route_order` finds the order's four pool-disjoint paths and splits the amount over them; `swap_order_` (cfmm_swap_order)
executes that answer ALL OR NOTHING ACROSS THE PATHS: every path is walked, the outputs are added in path order, and only when
the total clears `min_total_out` does any pool move.  `swap_path_` cannot say that: its limits are per path, and a path that
misses its limit leaves its siblings applied.

The second half shows what the limit is for.  On a second copy of the market the order is routed, then somebody else's
ordinary `swap_` moves one of its pools, and the order is sent with the limit it was routed with: ORDER_LIMIT, every path held,
and no bit of any pool moved.  `route_order_` is the three steps in one call, with the limit stated as a slippage."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr

STATUS = {cr.ORDER_APPLIED: "applied", cr.ORDER_LIMIT: "held: the total misses the limit", cr.ORDER_REFUSED: "refused",
          cr.ORDER_UNOBTAINABLE: "unobtainable"}


def market():
    """split_order.py's pools"""
    return [cr.ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]),        # 1 -> 2, the deepest
            cr.ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),        # 1 -> 2, half as deep, a lower fee
            cr.ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]),        # 1 -> 2, shallow
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),        # the detour: 1 -> 3 ...
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]        # ... 3 -> 2


def reserves(router):
    return np.concatenate([np.asarray(p.R, dtype=np.float64) for p in router.cfmms])


def main():
    amount, slippage = 1.0e5, 0.001
    router = cr.Router(cr.LinearNonnegative(np.ones(3)), market(), 3)
    alone, _, _, _ = cr.find_path(router, 1, 2, amount, max_hops=3)                                   # read-only
    pools, tokens, x, y, total, st = cr.route_order(router, 1, 2, amount, max_paths=8, max_hops=3)     # read-only: find -> split
    limit = total * (1.0 - slippage)
    print(f"{amount:g} of token 1 for token 2: the best single path gives {alone[0]:.9g}, {len(pools[0])} paths give {total[0]:.9g}")
    out, got, status, path_status = cr.swap_order_(router, pools, tokens, x, min_total_out=limit)
    print(f"  swap_order_ with min_total_out {limit[0]:.9g}: {STATUS[int(status[0])]}, {got[0]:.9g} out "
          f"(the split's total bit for bit: {bool(got[0] == total[0])})")
    router.close()

    # the same order on a market that moves between routing and execution
    stale = cr.Router(cr.LinearNonnegative(np.ones(3)), market(), 3)
    pools2, tokens2, x2, _, total2, _ = cr.route_order(stale, 1, 2, amount, max_paths=8, max_hops=3)
    first_pool = pools2[0][0][0]
    cr.swap_(stale, [first_pool], [0], [2.0e3], [1])                                                  # somebody sells 2000 of token 1 into it
    before = reserves(stale)
    out2, got2, status2, path_status2 = cr.swap_order_(stale, pools2, tokens2, x2, min_total_out=total2 * (1.0 - slippage))
    untouched = bool(np.array_equal(before.view(np.uint64), reserves(stale).view(np.uint64)))
    print(f"  after a swap_ moved pool {first_pool}: {STATUS[int(status2[0])]}; the order would now give {got2[0]:.9g}, "
          f"{(1.0 - got2[0] / total2[0]) * 100:.3g} % less; paths held: {int(np.sum(path_status2[0] == cr.ORDER_PATH_HELD))} of "
          f"{len(pools2[0])}; no bit of any pool moved: {untouched}")
    # routed afresh on the moved market, in one call
    res = cr.route_order_(stale, 1, 2, amount, max_slippage=slippage, max_paths=8, max_hops=3)
    print(f"  route_order_ on the moved market: {STATUS[int(res[8][0])]}, {res[7][0]:.9g} out")
    stale.close()
    return ((float(alone[0]), pools[0], float(total[0])), (float(got[0]), int(status[0]), path_status[0].tolist()),
            (float(got2[0]), float(total2[0]), int(status2[0]), path_status2[0].tolist(), untouched), (float(res[7][0]), int(res[8][0])))


if __name__ == "__main__":
    main()
