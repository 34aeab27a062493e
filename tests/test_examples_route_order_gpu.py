"""examples/route_order.py on the device: the four paths of split_order.py's order are FOUND, no pool twice; the split over them
is bit for bit what split_paths answers for split_order.py's hand-written paths in the same order; route_order composes the two
steps; one swap_path_ call executes the shares."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import PATH_APPLIED, SPLIT_OK

pytestmark = pytest.mark.gpu

HAND = {(0,): [1, 2], (1,): [1, 2], (2,): [1, 2], (3, 4): [1, 3, 2]}       # split_order.py's paths and their tokens


def test_route_order_example(capsys):
    import route_order
    (paths, toks, alone), (x, y, total, st), (out, applied), routed = route_order.main()
    text = capsys.readouterr().out
    assert "4 paths that share no pool, found on the device" in text and "executed" in text and "not executed" not in text
    assert "the same paths True, the same total True" in text
    assert {tuple(p) for p in paths} == set(HAND) and len(paths) == 4       # the set of found paths is {[0], [1], [2], [3, 4]}
    assert [toks[k] for k in range(4)] == [HAND[tuple(p)] for p in paths]
    assert paths[0] == [0] and all(a >= b for a, b in zip(alone, alone[1:]))  # best first: the deepest pool
    assert st == SPLIT_OK and total > alone[0] and abs(sum(x) - 1.0e5) <= 1e-15 * 1.0e5 and all(v > 0 for v in x)
    assert all(a == PATH_APPLIED for a in applied) and out == y             # executed at split_paths' bits
    # the same split from the hand-written lists, in the found order, on a fresh market
    r = cr.Router(cr.LinearNonnegative(np.ones(3)), route_order.market(), 3)
    try:
        hx, hy, htotal, hst = cr.split_paths(r, [[list(p) for p in paths]], [[HAND[tuple(p)] for p in paths]], 1.0e5)
        assert htotal[0] == total and hx[0].tolist() == x and hy[0].tolist() == y and hst[0] == st
    finally:
        r.close()
    assert routed[0][0] == paths and routed[1][0] == toks and routed[2][0].tolist() == x and routed[3][0].tolist() == y
    assert routed[4][0] == total and routed[5][0] == st
