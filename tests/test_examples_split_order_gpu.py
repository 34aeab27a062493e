"""examples/split_order.py on the device: the order's split over four paths beats find_path's single path, its shares sum to the
amount, one swap_path_ call executes them at the quoted outputs, and every pool has moved."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import PATH_APPLIED, SPLIT_OK

pytestmark = pytest.mark.gpu


def test_split_order_example(capsys):
    import split_order
    (single, path), (x, y, total, st), (out, applied), moved = split_order.main()
    text = capsys.readouterr().out
    assert "executed" in text and "not executed" not in text
    printed_single = float(re.search(r"path \[\d+(?:, \d+)*\]: ([0-9.e+]+) out", text).group(1))
    printed_split = float(re.search(r"split_paths: ([0-9.e+]+) out", text).group(1))
    assert printed_split > printed_single                                  # the printed split beats the printed single path
    assert st == SPLIT_OK and total > single and path == [0]               # the deepest pool is the best single path
    assert abs(sum(x) - 1.0e5) <= 1e-15 * 1.0e5 and all(v > 0 for v in x) and x[0] > x[1] > x[2]
    assert total == ((y[0] + y[1]) + y[2]) + y[3]
    assert all(a == PATH_APPLIED for a in applied) and out == y             # executed at split_paths' bits
    assert all(moved)
