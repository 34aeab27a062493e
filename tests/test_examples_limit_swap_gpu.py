"""examples/limit_swap.py on the device: a limit order against one pool of each kind (filled where the pool is deep, partial --
resting at the limit -- where it is not), and one Curve pool arbitraged to an outside price."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu


def test_limit_swap_example(capsys):
    import cfmmrouter_amd as cr
    import limit_swap
    results, (spot, used, out, profit, after) = limit_swap.main()          # (its own assertions hold, or it raises)
    text = capsys.readouterr().out
    assert set(results) == {"Product", "GeometricMean", "UniV3", "weighted (3 coins)", "Curve", "Solidly"}
    for name, (s, limit, room, sold, got, status, rest) in results.items():
        assert f"{name}: spot" in text
        assert limit == 0.97 * s and 0.0 < sold <= 5e4 and got > 0.0 and sold == min(5e4, room), name
        assert got / sold > limit                                           # the average price beats the limit: the last unit met it
        if status == cr.LIMIT_PARTIAL:
            assert abs(rest - limit) <= 1e-12 * limit, name
        else:
            assert status == cr.LIMIT_FILLED and rest > limit, name
    assert results["Product"][5] == cr.LIMIT_PARTIAL and results["GeometricMean"][5] == cr.LIMIT_FILLED
    assert spot > 0.97 and used > 0 and profit > 0 and abs(after - 0.97) <= 1e-12 and out / used > 0.97
    assert "the pool rests at the limit" in text and "profit" in text
