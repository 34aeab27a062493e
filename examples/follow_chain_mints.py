"""Follow a chain through a block with a mint, a burn and a swap, without re-uploading the market.

Two snapshots of the same pools: in the second one a position was minted in the first concentrated-liquidity pool (a new
initialised tick), one was burned in the second (a tick disappears), and a swap moved the first constant-product pair.
`chain.snapshot_delta(old, new, ladders=True)` turns the difference into pool states -- `(price, lower_ticks, liquidity)` for
the two pools whose tick ladder changed -- and `update_pools_` applies them on the device (cfmm_pools_set_ticks,
cfmm_pools_set_reserves); the next route! sees the new market.

    python examples/follow_chain_mints.py
"""
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cfmmrouter_amd as cr
from cfmmrouter_amd import chain

HERE = os.path.dirname(os.path.abspath(__file__))


def next_block(recs):
    """-> the records one block later"""
    new = copy.deepcopy(recs)
    v3 = [r for r in new if r["type"] == "concentrated"]
    # a mint of L between a NEW tick and an initialised one: +L at the lower tick, -L at the upper one
    a, L = v3[0], 10 ** 18
    lo, hi = a["ticks"][1][0] + 40, a["ticks"][4][0]
    a["ticks"] = sorted([[t, str(int(net) - (L if t == hi else 0))] for t, net in a["ticks"]] + [[lo, str(L)]])
    a.pop("liquidity", None)                                 # (the active liquidity follows from the ticks)
    # a burn that clears an initialised tick: its liquidity now starts at the next one
    b = v3[1]
    gone = b["ticks"].pop(2)
    b["ticks"][2][1] = str(int(b["ticks"][2][1]) + int(gone[1]))
    b.pop("liquidity", None)
    # a swap through the first constant-product pair
    cp = next(r for r in new if r["type"] == "constant_product")
    cp["reserves"] = [str(int(cp["reserves"][0]) * 98 // 100), str(int(cp["reserves"][1]) * 10204 // 10000)]
    return new


def main(solver="native", path=os.path.join(HERE, "data", "snapshot.jsonl")):
    with open(path) as f:
        recs = [json.loads(line) for line in f if line.strip() and not line.lstrip().startswith("#")]
    old, new = chain.load_snapshot(recs), chain.load_snapshot(next_block(recs))
    tokens, batches = old
    n = len(tokens)
    usd = {"USDC": 1.0, "DAI": 1.0, "USDT": 1.0, "FRAX": 0.998, "LUSD": 1.004}
    c = np.array([usd[t] for t in tokens])
    router = cr.Router(cr.LinearNonnegative(c), batches, n)
    cr.route_(router, v=c.copy(), solver=solver)
    before = float(c @ cr.netflows(router))
    print(f"block 1: profit {before:.2f} USD")
    changes = chain.snapshot_delta(old, new, ladders=True)
    for pos, state in sorted(changes.items()):
        what = f"ladder of {len(state[1])} ticks at price {state[0]:.6g}" if isinstance(state, tuple) else f"reserves {np.asarray(state)}"
        print(f"  pool {pos}: {what}")
    cr.update_pools_(router, changes)
    cr.route_(router, v=c.copy(), solver=solver)
    after = float(c @ cr.netflows(router))
    print(f"block 2: profit {after:.2f} USD after {len(changes)} pool updates")
    router.close()
    return before, after, changes


if __name__ == "__main__":
    main()
