"""Limit swaps: "sell up to this much, but not below my price" -- and "move this pool to the outside price".

`quote_rate` answers what the price is after a trade.  `amount_to_rate` (cfmm_quote_to_rate) is its inverse: how much a pool
takes before its marginal rate -- units out per unit in for the next unit, fee included -- has fallen to a limit.
`swap_limit_` (cfmm_swap_limit) executes against it: it tenders min(amount_in, that amount), so an order larger than the pool can
absorb at the limit is filled partially and the pool comes to rest at the limit.
    1. a seller with 50 000 of token 1 and a limit of 97 % of the spot rate, against one pool of each kind: the fill, its status,
       and the pool's spot rate afterwards -- the limit;
    2. the arbitrageur's trade on one chosen pool: a Curve pool quotes token 1 in token 5 at par while the outside market pays
       0.97; selling token 1 into it "as much as it takes" (amount inf) down to the outside rate takes exactly what is
       profitable, and afterwards the pool offers nothing above the outside rate."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr

STATUS = {cr.LIMIT_FILLED: "filled", cr.LIMIT_PARTIAL: "partial: the pool rests at the limit", cr.LIMIT_NONE: "nothing to do",
          cr.LIMIT_REFUSED: "refused"}


def market():
    price = {1: 1.0, 2: 2.0, 3: 0.5, 4: 4.0, 5: 1.0}                       # value of one unit of each token
    R = lambda value, *tokens: [value / price[t] for t in tokens]          # noqa: E731  reserves of equal value
    pools = [cr.ProductTwoCoin(R(2e5, 1, 3), 0.997, [1, 3]),                               # 0 Product: shallow, fills partially
             cr.GeometricMeanTwoCoin(R(2e7, 1, 4), [0.5, 0.5], 0.997, [1, 4]),             # 1 GeometricMean: deep, fills
             cr.UniV3(1.04, [1.21, 1.1, 1.0, 0.9, 0.8], [2e11, 3e11, 4e11, 3e11, 2e11], 0.997, [1, 5]),   # 2 UniV3, five ticks
             cr.GeometricMean(R(3e6, 1, 2, 3), [1 / 3, 1 / 3, 1 / 3], 0.997, [1, 2, 3]),   # 3 weighted, three coins
             cr.Curve(R(1e6, 1, 5), 0.9995, [1, 5], 2.0, 1e15),                            # 4 Curve: tokens 1 and 5 near par
             cr.SolidlyStableTwoCoin(R(1e6, 1, 5), 0.9995, [1, 5])]                        # 5 Solidly stable pair
    names = ["Product", "GeometricMean", "UniV3", "weighted (3 coins)", "Curve", "Solidly"]
    token_out = [3, 4, 5, 2, 5, 5]
    return cr.Router(cr.LinearNonnegative(np.ones(5)), pools, 5), names, token_out


def main():
    router, names, token_out = market()
    have = 5e4
    results = {}
    for i, name in enumerate(names):
        coin_out = 1                                                       # every pool's second coin
        spot = cr.spot_price(router, [i], 0, coin_out)[0]
        limit = 0.97 * spot
        room, would_get = cr.amount_to_rate(router, [i], 1, token_out[i], limit)            # read-only
        used, out, status = cr.swap_limit_(router, [i], 1, token_out[i], have, limit)
        after = cr.spot_price(router, [i], 0, coin_out)[0]
        print(f"{name}: spot {spot:.6g}, limit {limit:.6g}: room for {room[0]:.6g}; sold {used[0]:.6g} of {have:g} for {out[0]:.6g} "
              f"({STATUS[int(status[0])]}); spot afterwards {after:.6g}")
        assert used[0] == min(have, room[0])                               # the swap tenders what the quote said there is room for
        if status[0] == cr.LIMIT_PARTIAL:
            assert used[0] == room[0] and out[0] == would_get[0]
            assert abs(after - limit) <= 1e-12 * limit                     # the pool rests at the limit
        else:
            assert status[0] == cr.LIMIT_FILLED and used[0] == have and after > limit
        results[name] = (spot, limit, room[0], used[0], out[0], int(status[0]), after)
    assert {r[5] for r in results.values()} == {cr.LIMIT_FILLED, cr.LIMIT_PARTIAL}
    router.close()

    # the arbitrageur's trade on ONE pool: the Curve pool against an outside market that pays 0.97 token 5 per token 1
    router, names, token_out = market()
    curve, outside = 4, 0.97
    spot = cr.spot_price(router, [curve], 0, 1)[0]
    used, out, status = cr.swap_limit_(router, [curve], 1, 5, np.inf, outside)              # as much as it takes
    after = cr.spot_price(router, [curve], 0, 1)[0]
    profit = out[0] - outside * used[0]                                    # in token 5: bought in the pool, sold outside
    print(f"Curve pool: spot {spot:.6g} against an outside rate of {outside}: sold {used[0]:.6g} of token 1 into it for {out[0]:.6g} "
          f"of token 5 (average {out[0] / used[0]:.6g}), profit {profit:.6g} of token 5; the pool now quotes {after:.6g}")
    assert status[0] == cr.LIMIT_PARTIAL and profit > 0 and abs(after - outside) <= 1e-12
    again = cr.swap_limit_(router, [curve], 1, 5, np.inf, outside * (1 + 1e-9))            # a strict caller's margin
    assert again[2][0] == cr.LIMIT_NONE and again[0][0] == 0.0             # nothing left above the outside rate
    cr.route_(router)                                                      # the solver runs on the moved market
    router.close()
    return results, (spot, used[0], out[0], profit, after)


if __name__ == "__main__":
    main()
