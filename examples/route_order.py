"""Routing an order without leaving the device: 100 000 of token 1 for token 2 on examples/split_order.py's five-pool market.

split_order.py writes the order's four paths out by hand.  Here they are FOUND: `find_disjoint_paths`
(cfmm_find_disjoint_paths) runs `find_path`'s layered search up to eight times, each round on the market without the pools of
the paths before it, and answers with the paths in the form `split_paths` takes -- the three direct pools and the detour
1 -> 3 -> 2, best first, no pool twice.  `split_paths` (cfmm_split_paths) then says how much goes down each, and one
`swap_path_` call executes the shares.  `route_order` is the first two steps in one call."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED

STATUS = {cr.SPLIT_OK: "split", cr.SPLIT_NONE: "nothing to split", cr.SPLIT_NAN: "not a number",
          cr.SPLIT_SATURATED: "the paths cannot absorb it all"}


def market():
    """split_order.py's pools"""
    return [cr.ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]),        # 1 -> 2, the deepest
            cr.ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),        # 1 -> 2, half as deep, a lower fee
            cr.ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]),        # 1 -> 2, shallow
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),        # the detour: 1 -> 3 ...
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]        # ... 3 -> 2


def main():
    router = cr.Router(cr.LinearNonnegative(np.ones(3)), market(), 3)
    amount = 1.0e5
    alone, pools, tokens, _ = cr.find_disjoint_paths(router, 1, 2, amount, max_paths=8, max_hops=3)   # read-only
    paths, toks = pools[0], tokens[0]
    print(f"{amount:g} of token 1 for token 2: {len(paths)} paths that share no pool, found on the device")
    for p, tk, yi in zip(paths, toks, alone[0]):
        print(f"  path {p} (tokens {tk}): {yi:.9g} out if it carried the whole order")
    x, y, total, st = cr.split_paths(router, [paths], [toks], amount)                                 # read-only: one launch
    for p, xi, yi in zip(paths, x[0], y[0]):
        print(f"  share of path {p}: {xi:.9g} in -> {yi:.9g} out")
    print(f"  split_paths: {total[0]:.9g} out ({STATUS[int(st[0])]}), {total[0] - alone[0][0]:.6g} more than the best single path")
    routed = cr.route_order(router, 1, 2, amount, max_paths=8, max_hops=3)                            # find -> split in one call
    print(f"  route_order: the same paths {routed[0][0] == paths}, the same total {bool(routed[4][0] == total[0])}")
    out, applied = cr.swap_path_(router, paths, toks, x[0])
    print(f"  swap_path_ at the shares: {np.sum(out):.9g} out, "
          f"{'executed' if np.all(applied == PATH_APPLIED) else 'not executed'}")
    router.close()
    return (paths, toks, alone[0].tolist()), (x[0].tolist(), y[0].tolist(), float(total[0]), int(st[0])), (out.tolist(), applied.tolist()), routed


if __name__ == "__main__":
    main()
