"""examples/route_order_out.py on the device: an order that no single path can fill is found nothing for when probed with the whole
amount, is split over three paths when probed with a share's size, one swap_path_out_ call executes the shares at the quoted
costs, and the pools have given exactly the amount and taken exactly the total (their reserves grow by it less the fees)."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import SPLIT_OK, SPLIT_UNOBTAINABLE, SWAP_APPLIED

pytestmark = pytest.mark.gpu


def test_route_order_out_example(capsys):
    import route_order_out
    (alone, one_path), whole, (paths, toks, x, c, total, st), (cost, applied), (gave, took, kept) = route_order_out.main()
    text = capsys.readouterr().out
    assert "executed" in text and "not executed" not in text
    want = 1.5e5
    assert math.isinf(alone) and alone > 0 and one_path == []              # no single path can give the amount
    assert whole == (0, math.inf, SPLIT_UNOBTAINABLE)                      # ... so probing with it finds nothing
    assert st == SPLIT_OK and sorted(paths) == [[0], [1], [3, 4]]          # the three paths that can carry a quarter; pool 2 cannot
    assert toks == [[1, 3, 2] if p == [3, 4] else [1, 2] for p in paths]
    assert abs(sum(x) - want) <= 8 * 2.0 ** -53 * want and all(0 < v < want for v in x)
    assert total == (c[0] + c[1]) + c[2] and math.isfinite(total)
    assert all(a == SWAP_APPLIED for a in applied) and cost == c           # executed at split_paths_out's bits
    assert abs(gave - want) <= 1e-9 * want                                 # the pools gave exactly the amount ...
    assert abs(took - kept) <= 1e-9 * total and 0.997 * total <= kept <= 0.999 * total   # ... and took total_in, less their fees of 0.1 % .. 0.3 %
