"""Executing an arbitrage cycle: quote it at a few sizes, make the best one, all or nothing.

Three pools of three kinds -- a Product pair, a GeometricMean pair and a Curve pool -- quote slightly different prices for
the same three tokens, so carrying token 1 round the cycle 1 -> 2 -> 3 -> 1 returns more than went in, up to a size.
`quote_path` prices the cycle at a ladder of sizes in one launch and changes nothing.  `swap_path_` (cfmm_swap_path) then
EXECUTES the best size with `min_out` set to its own input: the three pools move on the device exactly as three `swap_`
calls would move them, but only if the whole cycle returns at least what it costs -- a pool refused on the way, or a market
that has moved in the meantime, leaves every pool untouched instead of a half-made cycle to unwind.  A second execution of
the same cycle meets the market the first one left and no longer clears its limit."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED, PATH_BELOW_LIMIT


def main():
    pools = [cr.ProductTwoCoin([1.00e5, 2.00e5], 0.997, [1, 2]),                    # 1 -> 2 at about 2.00
             cr.GeometricMeanTwoCoin([2.00e5, 1.04e5], [0.5, 0.5], 0.997, [2, 3]),  # 2 -> 3 at about 0.52
             cr.Curve([1.0e5, 1.0e5], 0.9995, [3, 1], 2.0, 1e15)]                   # 3 -> 1 at about 1.00
    router = cr.Router(cr.LinearNonnegative(np.ones(3)), pools, 3)
    cycle, tokens = [0, 1, 2], [1, 2, 3, 1]
    sizes = 50.0 * 1.25 ** np.arange(20)
    quoted = cr.quote_path(router, [cycle] * sizes.size, [tokens] * sizes.size, sizes)     # read-only: one launch
    best = int(np.argmax(quoted - sizes))
    print(f"cycle {tokens}: best of {sizes.size} sizes is {sizes[best]:.6g} in -> {quoted[best]:.6g} out")
    results = []
    for attempt in range(2):
        out, status = cr.swap_path_(router, [cycle], [tokens], [sizes[best]], min_out=[sizes[best]])
        what = {PATH_APPLIED: "executed", PATH_BELOW_LIMIT: "below the limit, nothing moved"}.get(int(status[0]), "refused, nothing moved")
        print(f"  execution {attempt + 1}: {sizes[best]:.6g} in, {out[0]:.6g} out: {what}")
        results.append((float(out[0]), int(status[0])))
    print(f"  the Product pool now holds {router.cfmms[0].R[0]:.6g} / {router.cfmms[0].R[1]:.6g}")
    router.close()
    return list(zip(sizes.tolist(), quoted.tolist())), best, results[0], results[1]


if __name__ == "__main__":
    main()
