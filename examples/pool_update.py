"""Follow a chain without re-uploading the market: load a snapshot, route, apply the few pools a new block moved
(`update_pools_`: their new state goes to the device in one small scatter per segment), route again.

The reference does this by mutating `cfmm.R` and calling `route!` again; here the pools live on the GPU, so the change is
handed over explicitly.  `chain.snapshot_delta(old, new)` computes the same `changes` from two snapshots."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain

HERE = os.path.dirname(os.path.abspath(__file__))


def main(solver="native", path=os.path.join(HERE, "data", "snapshot.jsonl")):
    tokens, batches = chain.load_snapshot(path)
    n = len(tokens)
    usd = {"USDC": 1.0, "DAI": 1.0, "USDT": 1.0, "FRAX": 0.998, "LUSD": 1.004}
    c = np.array([usd[t] for t in tokens])
    router = cr.Router(cr.LinearNonnegative(c), batches, n)
    cr.route_(router, v=c.copy(), solver=solver)
    before = float(c @ cr.netflows(router))
    print(f"block 1: profit {before:.2f} USD")
    # block 2: a swap drained 2 % of one side of the first constant-product pair, and the first concentrated pool's price fell 0.1 %
    first_v3 = sum(len(b) for b in batches[:2])                  # batches: constant product, weighted, concentrated
    changes = {0: batches[0].R[0] * [0.98, 1.0204], first_v3: float(batches[2].current_price[0]) * 0.999}
    cr.update_pools_(router, changes)
    cr.route_(router, v=c.copy(), solver=solver)
    after = float(c @ cr.netflows(router))
    print(f"block 2: profit {after:.2f} USD after {len(changes)} pool updates")
    router.close()
    return before, after, changes


if __name__ == "__main__":
    main()
