"""Back-running a pending swap: apply it on the device, then route the arbitrage it opens.

A router follows a market that is at rest: every pool quotes the same prices, up to less than its fee, so `route_` finds
nothing worth trading.  A large pending swap is then applied to a few pools with `swap_` (cfmm_swap): each pool answers
what `quote` would have answered and moves to R + γΔ − Λ on the device -- no reserves are recomputed on the host, nothing is
re-uploaded.  The next `route_` runs on the market the swap left behind and finds the back-run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth


def main(m=2000, n_tokens=16, hit=3, size=0.05):
    pi = synth.token_price_vector(n_tokens, seed=5)
    Ai = synth.token_pairs(5, 1, m, n_tokens)
    R = (100.0 + 900.0 * synth.uniform(5, 3, m))[:, None] / pi[Ai - 1]      # every pool quotes π ...
    R[:, 0] *= np.exp(0.002 * (2.0 * synth.uniform(5, 4, m) - 1.0))         # ... up to ±0.2 %, inside a 0.3 % fee
    pools = cr.ProductTwoCoin.batch(R, np.full(m, 0.997), Ai)
    router = cr.Router(cr.LinearNonnegative(pi), [pools], n_tokens)
    cr.route_(router, solver="native")
    before = float(pi @ cr.netflows(router))
    # the pending swap: `size` of the reserve of coin 0 into each of `hit` pools, the largest pool twice in a row
    rows = np.argsort(-pools.R[:, 0])[:hit]
    victim = np.concatenate([rows, rows[:1]])
    amount = size * pools.R[victim, 0]
    quoted = cr.quote(router, victim[:hit], 0, amount[:hit])
    got = cr.swap_(router, victim, 0, amount)                                # applied in order; the host mirror follows
    assert np.array_equal(got[:hit], quoted)                                 # a swap answers what the quote answered
    cr.route_(router, solver="native")                                       # the back-run, on the moved market
    after = float(pi @ cr.netflows(router))
    Δ = np.asarray(router.Δs)
    print(f"market at rest: arbitrage worth {before:.6g}")
    for k, i in enumerate(victim):
        print(f"  swap {k}: {amount[k]:.6g} of coin 0 into pool {i} -> {got[k]:.6g} of coin 1")
    print(f"back-run after the swaps: arbitrage worth {after:.6g}, {int(np.sum(np.any(Δ != 0, axis=1)))} pools trade")
    router.close()
    return before, after, got, victim


if __name__ == "__main__":
    main()
