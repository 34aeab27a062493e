"""examples/size_cycle.py on the device: the cycle is found at a probe amount, sized, executed at that size with its own input
as the limit, and sizing it again on the market the execution left gains nothing, or next to nothing."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import FOUND, PATH_APPLIED, SIZED, SIZED_NONE

pytestmark = pytest.mark.gpu


def test_size_cycle_example(capsys):
    import size_cycle
    (found, pools, tokens, status), (x, y, gain, st), (out, applied), (x2, gain2, st2) = size_cycle.main()
    text = capsys.readouterr().out
    assert "executed" in text and "not executed" not in text and "sized" in text
    assert status == FOUND and sorted(pools) == [0, 1, 2] and tokens[0] == tokens[-1] == 1 and found > 100.0
    assert st == SIZED and 100.0 < x < 1.0e4 and gain > 0 and gain == y - x
    assert gain > found - 100.0                                            # more than the probe made
    assert applied == PATH_APPLIED and out == y                            # the first execution is applied, at quote_path's bits
    assert st2 == SIZED_NONE or (st2 == SIZED and gain2 < 1e-3 * gain)     # the second sizing gains less: the cycle is closed
    assert gain2 < gain
