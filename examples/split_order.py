"""Splitting an order: 100 000 of token 1 for token 2, over three parallel pools and a two-hop detour.

Three Product pairs of different depth trade token 1 for token 2 directly; two more make the detour 1 -> 3 -> 2.  The order is as
large as the deepest pool, so sending all of it down `find_path`'s single best path (cfmm_find_path) pays for the slippage of
one pool.  `split_paths` (cfmm_split_paths) asks the device how much should go down each of the four paths: five rounds of 64
grid points per path, each round handing out what is left slice by slice to the path whose next slice buys the most, one
wavefront for the whole search.  One `swap_path_` call then EXECUTES the four shares -- the paths share no pool, so each gets
exactly what `split_paths` quoted -- and the pools are shown to have moved."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED

STATUS = {cr.SPLIT_OK: "split", cr.SPLIT_NONE: "nothing to split", cr.SPLIT_NAN: "not a number",
          cr.SPLIT_SATURATED: "the paths cannot absorb it all"}


def main():
    pools = [cr.ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]),        # 1 -> 2, the deepest
             cr.ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),        # 1 -> 2, half as deep, a lower fee
             cr.ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]),        # 1 -> 2, shallow
             cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),        # the detour: 1 -> 3 ...
             cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]        # ... 3 -> 2
    router = cr.Router(cr.LinearNonnegative(np.ones(3)), pools, 3)
    amount = 1.0e5
    single, path, tokens, _ = cr.find_path(router, 1, 2, amount, max_hops=2)
    print(f"{amount:g} of token 1 for token 2, all through find_path's path {path[0]}: {single[0]:.9g} out")
    paths, toks = [[0], [1], [2], [3, 4]], [[1, 2], [1, 2], [1, 2], [1, 3, 2]]
    x, y, total, st = cr.split_paths(router, [paths], [toks], amount)                # read-only: one launch
    for p, tk, xi, yi in zip(paths, toks, x[0], y[0]):
        print(f"  path {p} (tokens {tk}): {xi:.9g} in -> {yi:.9g} out")
    print(f"  split_paths: {total[0]:.9g} out ({STATUS[int(st[0])]}), {total[0] - single[0]:.6g} more than the single path")
    before = [pl.R.copy() for pl in router.cfmms]
    out, applied = cr.swap_path_(router, paths, toks, x[0])
    print(f"  swap_path_ at the four shares: {np.sum(out):.9g} out, "
          f"{'executed' if np.all(applied == PATH_APPLIED) else 'not executed'}")
    moved = [bool(np.any(pl.R != b)) for pl, b in zip(router.cfmms, before)]
    print(f"  pools moved: {moved}; pool 0's reserves {before[0].tolist()} -> {router.cfmms[0].R.tolist()}")
    router.close()
    return (float(single[0]), path[0]), (x[0].tolist(), y[0].tolist(), float(total[0]), int(st[0])), (out.tolist(), applied.tolist()), moved


if __name__ == "__main__":
    main()
