"""Finding the cheapest way to buy an exact amount: "I want exactly 1000 of token 3 and pay in token 1 -- through which pools,
and what does it cost?"

The market is that of examples/find_route.py: seven pools of four kinds quote five tokens at consistent prices, but at very
different depths -- the direct pool 1 <-> 3 is shallow, a Curve pool and a deep Product pool lead there through token 5, and
other detours exist.  `find_path_out` (cfmm_find_path_out) searches every walk of at most three pools ON THE DEVICE, backwards
from the wanted output -- one pass over the pools per hop -- and answers with one executable path and its cost.
`quote_path_out` prices that path again (the same bits), `swap_path_out_` EXECUTES it with `max_in` set to the cost found,
all or nothing, and the same order placed afterwards meets the market the execution left: it costs more, possibly through other
pools.  Nothing between the question and the execution is computed on the host: examples/buy_exact.py had to be handed its
path."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import SWAP_APPLIED


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
    token_in, token_out, want = 1, 3, 1000.0
    found, path, tokens, status = cr.find_path_out(router, token_in, token_out, want, max_hops=3)
    direct = cr.quote_out(router, [0], 0, want)[0]
    print(f"exactly {want:g} of token {token_out}, paid in token {token_in}: the direct pool asks {direct:.6g}; "
          f"found {found[0]:.6g} through pools {path[0]} (tokens {tokens[0]})")
    quoted = cr.quote_path_out(router, path, tokens, want)
    print(f"  quote_path_out on that path: {quoted[0]:.6g} ({'the same bits' if quoted[0] == found[0] else 'DIFFERENT'})")
    cost, st = cr.swap_path_out_(router, path, tokens, want, max_in=found)
    print(f"  swap_path_out_ with max_in = the cost found: {cost[0]:.6g} paid, {'executed' if st[0] == SWAP_APPLIED else 'not executed'}")
    after, path2, tokens2, status2 = cr.find_path_out(router, token_in, token_out, want, max_hops=3)
    print(f"  the same order afterwards: {after[0]:.6g} through pools {path2[0]} -- {'it costs more' if after[0] > found[0] else 'NOT more'}")
    too_much, _, _, status3 = cr.find_path_out(router, token_in, token_out, 1e9, max_hops=3)
    print(f"  a billion of token {token_out}: no pool holds that much -- cost {too_much[0]}, status {'none' if status3[0] == cr.FOUND_NONE else status3[0]}")
    router.close()
    return ((float(found[0]), path[0], tokens[0], int(status[0])), float(direct), float(quoted[0]), (float(cost[0]), int(st[0])),
            (float(after[0]), path2[0], int(status2[0])), (float(too_much[0]), int(status3[0])))


if __name__ == "__main__":
    main()
