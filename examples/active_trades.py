"""Following a chain, down to the list of trades to execute.

Route a market, apply the trades, let a block move a few pools, look for arbitrage at the same prices -- and read back only
the pools that now trade and are worth executing (`active_trades`: selected on the device, cfmm_select_trades), not the
whole market's r.Δs / r.Λs."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth


def main(m=5000, n_tokens=32, moved=20, min_value=1e-6):
    pi = synth.token_price_vector(n_tokens, seed=3)
    Ai = synth.token_pairs(3, 1, m, n_tokens)
    R = (100.0 + 900.0 * synth.uniform(3, 3, m))[:, None] / pi[Ai - 1]      # every pool quotes π ...
    R[:, 0] *= np.exp(0.0032 * (2.0 * synth.uniform(3, 4, m) - 1.0))        # ... up to ±0.32 %, around a 0.3 % fee
    pools = cr.ProductTwoCoin.batch(R, np.full(m, 0.997), Ai)
    router = cr.Router(cr.LinearNonnegative(pi), [pools], n_tokens)
    cr.route_(router, solver="native")
    prices = router.v.copy()
    cr.update_reserves_(router, sync_host=False)                             # the routed trades are executed
    rows = np.argsort(synth.uniform(3, 5, m))[:moved]                        # a block arrives: these pools moved
    cr.update_pools_(router, {int(i): pools.R[i] * [1.03, 0.97] for i in rows})
    cr.find_arb_(router, prices)
    idx, Δ, Λ, value = cr.active_trades(router, min_value)
    best = np.argsort(-value)[:5]                                            # the caller sorts the short list
    print(f"{idx.size} of {m} pools trade for at least {min_value} (moved: {moved})")
    for k in best:
        print(f"  pool {idx[k]}: tender {Δ[k]}, receive {Λ[k]}, worth {value[k]:.6g}")
    router.close()
    return idx, Δ, Λ, value, rows


if __name__ == "__main__":
    main()
