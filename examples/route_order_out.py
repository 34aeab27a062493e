"""Buying an exact amount that no single path can give: 150 000 of token 2, paid in token 1, on examples/split_order.py's
five-pool market -- whose deepest pool holds 100 000 of token 2.

`find_path_out` finds nothing for this order: every path answers +inf.  `route_order_out` (cfmm_find_disjoint_paths_out, then
cfmm_split_paths_out) probes the search with the size a share will have -- amount_out / max_paths by default -- so it finds the
paths that can each carry a share, and then says how much of the amount to buy through each and what that costs.  One
`swap_path_out_` call executes the shares with their costs as the limits, and the pools are shown to have given exactly the
amount and taken exactly the total (their reserves grow by it less the fees)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import SWAP_APPLIED

STATUS = {cr.SPLIT_OK: "split", cr.SPLIT_NONE: "nothing to buy", cr.SPLIT_NAN: "not a number",
          cr.SPLIT_UNOBTAINABLE: "the paths cannot give that much"}


def market():
    """split_order.py's pools"""
    return [cr.ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]),        # 1 -> 2, the deepest
            cr.ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),        # 1 -> 2, half as deep, a lower fee
            cr.ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]),        # 1 -> 2, shallow
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),        # the detour: 1 -> 3 ...
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]        # ... 3 -> 2


def held(router, token):
    """what the pools hold of a token, pool by pool"""
    return np.array([float(np.sum(p.R[np.asarray(p.Ai) == token])) for p in router.cfmms])


def main():
    router = cr.Router(cr.LinearNonnegative(np.ones(3)), market(), 3)
    want = 1.5e5
    alone, one_path, _, _ = cr.find_path_out(router, 1, 2, want, max_hops=3)                           # read-only
    print(f"{want:g} of token 2, paid in token 1: the best single path costs {alone[0]:g} (path {one_path[0]})")
    whole = cr.route_order_out(router, 1, 2, want, max_paths=4, max_hops=3, probe=want)                # probed with the whole amount
    print(f"  route_order_out probed with the whole amount: {len(whole[0][0])} paths, total {whole[4][0]:g} ({STATUS[int(whole[5][0])]})")
    pools, tokens, x, c, total, st = cr.route_order_out(router, 1, 2, want, max_paths=4, max_hops=3)   # probed with want / 4
    paths, toks = pools[0], tokens[0]
    print(f"  route_order_out probed with a share's size: {len(paths)} paths that share no pool ({STATUS[int(st[0])]})")
    for p, tk, xi, ci in zip(paths, toks, x[0], c[0]):
        print(f"  path {p} (tokens {tk}): buys {xi:.9g} for {ci:.9g}")
    print(f"  total_in: {total[0]:.9g}")
    before_in, before_out = held(router, 1), held(router, 2)
    cost, applied = cr.swap_path_out_(router, paths, toks, x[0], max_in=c[0])
    took, gave = held(router, 1) - before_in, before_out - held(router, 2)
    kept = np.sum([router.cfmms[p[0]].γ * ci for p, ci in zip(paths, cost)])   # a reserve grows by γ times what is tendered
    print(f"  swap_path_out_ at the shares: {'executed' if np.all(applied == SWAP_APPLIED) else 'not executed'}; "
          f"paid {np.sum(cost):.9g} of token 1; the pools gave {np.sum(gave):.9g} of token 2 and their reserves of token 1 "
          f"grew by {np.sum(took):.9g} (what was paid less the fees: {kept:.9g})")
    router.close()
    return ((float(alone[0]), one_path[0]), (len(whole[0][0]), float(whole[4][0]), int(whole[5][0])),
            (paths, toks, x[0].tolist(), c[0].tolist(), float(total[0]), int(st[0])), (cost.tolist(), applied.tolist()),
            (float(np.sum(gave)), float(np.sum(took)), float(kept)))


if __name__ == "__main__":
    main()
