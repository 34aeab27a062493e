"""examples/execute_order.py on the device: a routed order executes with a limit on its total at the split's bits; after an ordinary
swap_ has moved one of its pools the same order with the old limit is ORDER_LIMIT, every path is held and no bit of any pool
moved; routed afresh it goes through."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import ORDER_APPLIED, ORDER_LIMIT, ORDER_PATH_HELD, PATH_APPLIED

pytestmark = pytest.mark.gpu


def test_execute_order_example(capsys):
    import execute_order
    (alone, paths, total), (got, status, path_status), (got2, total2, status2, path_status2, untouched), (got3, status3) = execute_order.main()
    text = capsys.readouterr().out
    assert "applied" in text and "held: the total misses the limit" in text and "no bit of any pool moved: True" in text
    assert sorted(paths) == [[0], [1], [2], [3, 4]] and total > alone > 0      # no single path fills the order well
    assert status == ORDER_APPLIED and got == total and path_status == [PATH_APPLIED] * 4
    assert total2 == total and status2 == ORDER_LIMIT and path_status2 == [ORDER_PATH_HELD] * 4 and untouched
    assert 0 < got2 < total2 * (1.0 - 0.001) and math.isfinite(got2)           # the moved market gives less than the limit
    assert status3 == ORDER_APPLIED and 0 < got3 < total
