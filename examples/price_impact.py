"""Price impact: "what is the price right now, and what does MY order do to it?"

A ladder of sizes goes through one pool of each kind, and then through a path that `find_path` chooses.  Per size the
device answers, in one call, what comes out and the MARGINAL rate the trade leaves behind (`quote_rate`, cfmm_quote_rate: the
right derivative of the quote, fee included -- at size 0 the pool's spot rate).  Three prices follow:
    execution price   amount_out / amount_in          what this order pays on average
    marginal rate     d amount_out / d amount_in      what the NEXT unit would get
    price impact      1 - execution price / spot      the share of the spot value the order loses to its own size
The impact is 0 at size 0 and rises along the ladder; the marginal rate falls (faster than the execution price: it is the
price of the last unit, not the average).  Along a path the marginal rate is the product of its hops' rates -- the chain rule,
which is what `quote_path_rate` (cfmm_quote_path_rate) returns."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr

# of token 1, coin 0 of every pool below.  The ladder starts at 1e-3 of the stable pools' reserves: the impact of a smaller order
# through the Solidly pair (cubic in the size: 5e-16 at 10 units) lies below the rounding of the quote it is computed from.
SIZES = np.array([0.0, 1e3, 3e3, 1e4, 3e4, 1e5])

def main():
    price = {1: 1.0, 2: 2.0, 3: 0.5, 4: 4.0, 5: 1.0}                       # value of one unit of each token
    R = lambda value, *tokens: [value / price[t] for t in tokens]          # reserves of equal value: the pool quotes those prices
    pools = [cr.ProductTwoCoin(R(2e5, 1, 3), 0.997, [1, 3]),                               # 0 Product
             cr.GeometricMeanTwoCoin(R(2e6, 1, 4), [0.5, 0.5], 0.997, [1, 4]),             # 1 GeometricMean, two coins
             cr.UniV3(1.04, [1.21, 1.1, 1.0, 0.9, 0.8], [2e11, 3e11, 4e11, 3e11, 2e11], 0.997, [1, 5]),   # 2 UniV3: five ticks, the price inside the second
             cr.GeometricMean(R(3e6, 1, 2, 3), [1 / 3, 1 / 3, 1 / 3], 0.997, [1, 2, 3]),   # 3 weighted, three coins
             cr.Curve(R(1e6, 1, 5), 0.9995, [1, 5], 2.0, 1e15),                            # 4 Curve: tokens 1 and 5 one for one
             cr.SolidlyStableTwoCoin(R(1e6, 1, 5), 0.9995, [1, 5]),                        # 5 Solidly stable pair
             cr.ProductTwoCoin(R(2e6, 5, 3), 0.997, [5, 3])]                               # 6 a deep pool from token 5 to token 3
    names = ["Product", "GeometricMean", "UniV3", "weighted (3 coins)", "Curve", "Solidly"]
    router = cr.Router(cr.LinearNonnegative(np.ones(5)), pools, 5)
    sizes = SIZES
    results = {}
    for i, name in enumerate(names):
        which = np.full(sizes.size, i)
        coin_out = 1                                                       # every pool's second coin (the three-coin pool: token 2)
        out, rate = cr.quote_rate(router, which, 0, sizes, coin_out)
        impact = cr.price_impact(router, which, 0, sizes, coin_out)
        spot = cr.spot_price(router, [i], 0, coin_out)[0]
        print(f"{name}: spot rate {spot:.6g}")
        for a, o, r, imp in zip(sizes, out, rate, impact):
            exe = o / a if a > 0 else spot
            print(f"  {a:>8g} in: execution price {exe:.6g}, marginal rate {r:.6g}, impact {100 * imp:.4f} %")
        assert rate[0] == spot and impact[0] == 0.0                        # nothing tendered: the spot rate, no impact
        assert np.all(np.diff(impact) > 0)                                 # a larger order loses a larger share
        assert np.all(np.diff(rate) <= 0) and rate[-1] < rate[0]           # ... and leaves a worse price behind
        results[name] = (out, rate, impact)

    # a path chosen by the device: the best route for 1000 of token 1 into token 3
    found, path, tokens, status = cr.find_path(router, 1, 3, 1000.0, max_hops=3)
    path, tokens = path[0], tokens[0]
    n = sizes.size
    out, rate, hop_out, hop_rate = cr.quote_path_rate(router, [path] * n, [tokens] * n, sizes, hops=True)
    impact = cr.path_price_impact(router, [path] * n, [tokens] * n, sizes)
    print(f"path through pools {path} (tokens {tokens}): spot rate {rate[0]:.6g}")
    for q, a in enumerate(sizes):
        product = hop_rate[0, q]
        for k in range(1, len(path)):
            product = product * hop_rate[k, q]
        print(f"  {a:>8g} in: {out[q]:.6g} out, marginal rate {rate[q]:.6g} = the product of its hops' rates "
              f"{' x '.join(f'{hop_rate[k, q]:.6g}' for k in range(len(path)))}, impact {100 * impact[q]:.4f} %")
        assert rate[q] == product                                          # the chain rule, bit for bit
    assert impact[0] == 0.0 and np.all(np.diff(impact) > 0)
    assert out[1] == found[0]                                              # the path's own quote at the size it was found for
    router.close()
    return results, (path, tokens, out, rate, hop_rate, impact)


if __name__ == "__main__":
    main()
