"""Finding a route: "I have 1000 of token 1 and want token 3 -- through which pools, and how much do I get?"

Seven pools of four kinds quote five tokens at consistent prices, but at very different depths: the direct pool 1 <-> 3 is
shallow, a Curve pool and a deep Product pool lead there through token 5, and other detours exist.  `find_path`
(cfmm_find_path) searches every walk of at most three pools ON THE DEVICE -- one pass over the pools per hop -- and answers
with one executable path.  `quote_path` prices that path again (the same bits), `swap_path_` EXECUTES it with `min_out` set
to the amount found, all or nothing, and the same question asked afterwards meets the market the execution left: a worse
price, possibly through other pools."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED


def main():
    price = {1: 1.0, 2: 2.0, 3: 0.5, 4: 4.0, 5: 1.0}                       # value of one unit of each token
    R = lambda value, *tokens: [value / price[t] for t in tokens]          # reserves of equal value: the pool quotes those prices
    pools = [cr.ProductTwoCoin(R(2e4, 1, 3), 0.997, [1, 3]),                               # 0: the direct pool, shallow
             cr.ProductTwoCoin(R(1e5, 1, 2), 0.997, [1, 2]),                               # 1
             cr.ProductTwoCoin(R(1e6, 2, 3), 0.997, [2, 3]),                               # 2
             cr.GeometricMeanTwoCoin(R(2e6, 1, 4), [0.5, 0.5], 0.997, [1, 4]),             # 3
             cr.Curve(R(1e6, 1, 5), 0.9995, [1, 5], 2.0, 1e15),                            # 4: tokens 1 and 5 trade one for one
             cr.ProductTwoCoin(R(2e6, 5, 3), 0.997, [5, 3]),                               # 5: deep
             cr.GeometricMean(R(3e6, 2, 4, 3), [1 / 3, 1 / 3, 1 / 3], 0.997, [2, 4, 3])]   # 6: three coins
    router = cr.Router(cr.LinearNonnegative(np.ones(5)), pools, 5)
    token_in, token_out, amount = 1, 3, 1000.0
    found, path, tokens, status = cr.find_path(router, token_in, token_out, amount, max_hops=3)
    direct = cr.quote(router, [0], 0, amount)[0]
    print(f"{amount:g} of token {token_in} for token {token_out}: the direct pool gives {direct:.6g}; "
          f"found {found[0]:.6g} through pools {path[0]} (tokens {tokens[0]})")
    quoted = cr.quote_path(router, path, tokens, amount)
    print(f"  quote_path on that path: {quoted[0]:.6g} ({'the same bits' if quoted[0] == found[0] else 'DIFFERENT'})")
    out, st = cr.swap_path_(router, path, tokens, amount, min_out=found)
    print(f"  swap_path_ with min_out = the amount found: {out[0]:.6g} out, {'executed' if st[0] == PATH_APPLIED else 'not executed'}")
    after, path2, tokens2, status2 = cr.find_path(router, token_in, token_out, amount, max_hops=3)
    print(f"  the same question afterwards: {after[0]:.6g} through pools {path2[0]} -- {'a worse price' if after[0] < found[0] else 'NOT worse'}")
    router.close()
    return (float(found[0]), path[0], tokens[0], int(status[0])), float(direct), float(quoted[0]), (float(out[0]), int(st[0])), (float(after[0]), path2[0], int(status2[0]))


if __name__ == "__main__":
    main()
