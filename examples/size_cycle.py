"""Sizing an arbitrage cycle: find it at a probe amount, ask the device how much to put in, make it, all or nothing.

The three pools of examples/execute_cycle.py -- a Product pair, a GeometricMean pair and a Curve pool -- quote slightly different
prices for the same three tokens.  `find_path` (cfmm_find_path) from token 1 back to token 1 finds the cycle at a small probe
amount.  Where execute_cycle.py quotes a hand-made ladder of sizes and takes the best, `size_path` (cfmm_size_path) SEARCHES the
size on the device: five rounds of 64 trial sizes, each round between the neighbours of the best size of the round before, one
wavefront for the whole search.  `swap_path_` then EXECUTES that size with `min_out` set to its own input.  A second `size_path`
on the market the execution left finds nothing worth making, or next to nothing: the cycle has been closed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED

STATUS = {cr.SIZED: "sized", cr.SIZED_NONE: "no size gains", cr.SIZED_AT_LIMIT: "the limit binds", cr.SIZED_NAN: "not a number"}


def main():
    pools = [cr.ProductTwoCoin([1.00e5, 2.00e5], 0.997, [1, 2]),                    # 1 -> 2 at about 2.00
             cr.GeometricMeanTwoCoin([2.00e5, 1.04e5], [0.5, 0.5], 0.997, [2, 3]),  # 2 -> 3 at about 0.52
             cr.Curve([1.0e5, 1.0e5], 0.9995, [3, 1], 2.0, 1e15)]                   # 3 -> 1 at about 1.00
    router = cr.Router(cr.LinearNonnegative(np.ones(3)), pools, 3)
    probe, limit = 100.0, 1.0e4
    found, path, tokens, status = cr.find_path(router, 1, 1, probe, max_hops=3)
    print(f"{probe:g} of token 1 back to token 1: {found[0]:.6g} through pools {path[0]} (tokens {tokens[0]})")
    x, y, gain, st = cr.size_path(router, path, tokens, limit)                        # read-only: one launch
    print(f"  size_path up to {limit:g}: {x[0]:.9g} in -> {y[0]:.9g} out, gain {gain[0]:.9g} ({STATUS[int(st[0])]})")
    out, applied = cr.swap_path_(router, path, tokens, x, min_out=x)
    print(f"  swap_path_ at that size with min_out = its input: {out[0]:.9g} out, "
          f"{'executed' if applied[0] == PATH_APPLIED else 'not executed'}")
    x2, y2, gain2, st2 = cr.size_path(router, path, tokens, limit)
    print(f"  size_path on the market it left: gain {gain2[0]:.3g} at {x2[0]:.6g} in ({STATUS[int(st2[0])]})")
    router.close()
    return ((float(found[0]), path[0], tokens[0], int(status[0])), (float(x[0]), float(y[0]), float(gain[0]), int(st[0])),
            (float(out[0]), int(applied[0])), (float(x2[0]), float(gain2[0]), int(st2[0])))


if __name__ == "__main__":
    main()
