"""Buying an exact amount through a path, with a cost limit: what a chain transaction of the "exact output" kind does.

A buyer needs exactly 500 of token 4 and holds token 1.  The route is three pools of three kinds -- a Product pair 1/2, a
GeometricMean pair 2/3 and a Curve pool 3/4.  `quote_path_out` prices the purchase and changes nothing: it walks the path
from the last pool backwards and answers how much of token 1 to tender.  The buyer accepts half a percent of slippage on top
of that quote and sends `swap_path_out_` (cfmm_swap_path_out) with that limit: the path executes ALL OR NOTHING -- the last
pool gives exactly 500, every pool moves on the device as `swap_out_` would move it, and the cost is the quote's, bit for bit.

Then another trader's swap moves the first pool (`swap_`), and the buyer tries the same purchase with the same limit: it
would now cost more than the limit, so the path is not applied -- the answer is the quote it would have cost, the status
says "over the limit", and no pool of the path has changed a bit: there is no half-made purchase to unwind."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import SWAP_APPLIED, SWAP_OVER_LIMIT


def main():
    pools = [cr.ProductTwoCoin([1.00e5, 2.00e5], 0.997, [1, 2]),                    # 1 -> 2 at about 2.00
             cr.GeometricMeanTwoCoin([2.00e5, 1.04e5], [0.5, 0.5], 0.997, [2, 3]),  # 2 -> 3 at about 0.52
             cr.Curve([1.0e5, 1.0e5], 0.9995, [3, 4], 2.0, 1e15)]                   # 3 -> 4 at about 1.00
    router = cr.Router(cr.LinearNonnegative(np.ones(4)), pools, 4)
    path, tokens, want = [0, 1, 2], [1, 2, 3, 4], 500.0
    quoted = float(cr.quote_path_out(router, [path], [tokens], [want])[0])              # read-only
    limit = 1.005 * quoted
    print(f"buying exactly {want:g} of token 4 along {tokens}: quoted {quoted:.6g} of token 1, limit {limit:.6g}")
    cost, status, hops = cr.swap_path_out_(router, [path], [tokens], [want], max_in=[limit], hops=True)
    first = (float(cost[0]), int(status[0]))
    print(f"  purchase 1: cost {cost[0]:.6g} ({'executed' if status[0] == SWAP_APPLIED else 'not applied'}); "
          f"tendered per hop {hops[0, 0]:.6g} -> {hops[1, 0]:.6g} -> {hops[2, 0]:.6g} -> {want:g} out")
    print(f"  the Curve pool now holds {router.cfmms[2].R[1]:.9g} of token 4 (it gave exactly {want:g})")
    cr.swap_(router, [0], [0], [2000.0])                                                # another trade moves the first pool
    before = [np.array(p.R, copy=True) for p in router.cfmms]
    cost, status = cr.swap_path_out_(router, [path], [tokens], [want], max_in=[limit])
    second = (float(cost[0]), int(status[0]))
    what = {SWAP_APPLIED: "executed", SWAP_OVER_LIMIT: "over the limit, nothing moved"}.get(int(status[0]), "not applied, nothing moved")
    print(f"  purchase 2, after another trade moved the first pool: would cost {cost[0]:.6g} > {limit:.6g}: {what}")
    untouched = all(np.array_equal(p.R, b) for p, b in zip(router.cfmms, before))
    router.close()
    return quoted, limit, first, second, untouched


if __name__ == "__main__":
    main()
