"""From a routed market to the amounts to sign: exact-output quotes.

Route a market, let a block move a few pools, select the trades worth executing (`active_trades`) -- and then, for each of
them, ask the question an executor asks: "I want exactly this much out of that pool as it stands on the device now; how much
must I tender?" (`quote_out`: cfmm_quote_out, the inverse of `quote`).  The forward quote of the answer confirms it."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth


def main(m=5000, n_tokens=32, moved=20, min_value=1e-6, keep=0.9):
    pi = synth.token_price_vector(n_tokens, seed=3)
    Ai = synth.token_pairs(3, 1, m, n_tokens)
    R = (100.0 + 900.0 * synth.uniform(3, 3, m))[:, None] / pi[Ai - 1]      # every pool quotes π ...
    R[:, 0] *= np.exp(0.0032 * (2.0 * synth.uniform(3, 4, m) - 1.0))        # ... up to ±0.32 %, around a 0.3 % fee
    pools = cr.ProductTwoCoin.batch(R, np.full(m, 0.997), Ai)
    router = cr.Router(cr.LinearNonnegative(pi), [pools], n_tokens)
    cr.route_(router, solver="native")                                      # 1. route
    prices = router.v.copy()
    cr.update_reserves_(router, sync_host=False)
    rows = np.argsort(synth.uniform(3, 5, m))[:moved]                        # a block arrives: these pools moved
    cr.update_pools_(router, {int(i): pools.R[i] * [1.03, 0.97] for i in rows})
    cr.find_arb_(router, prices)
    idx, Δ, Λ, value = cr.active_trades(router, min_value)                   # 2. the trades worth executing
    # 3. the executor wants `keep` of each trade's output, exactly: what does that cost in each pool as it stands?
    coin_in = np.argmax(Δ > 0, axis=1).astype(np.int32)
    want = keep * Λ[np.arange(idx.size), 1 - coin_in]
    tender = cr.quote_out(router, idx, coin_in, want)
    # 4. the forward quote of that input gives the wanted output back
    got = cr.quote(router, idx, coin_in, tender)
    print(f"{idx.size} of {m} pools trade for at least {min_value} (moved: {moved})")
    for k in np.argsort(-value)[:5]:
        print(f"  pool {idx[k]}: for exactly {want[k]:.9g} of coin {1 - coin_in[k]} tender {tender[k]:.9g} of coin {coin_in[k]} "
              f"(the full trade tenders {Δ[k, coin_in[k]]:.9g}); quote confirms {got[k]:.9g}")
    router.close()
    return idx, Δ, Λ, want, tender, got


if __name__ == "__main__":
    main()
