"""examples/price_impact.py on the device: a ladder of sizes through one pool of each kind and through a path found by find_path;
the impact is 0 at size 0 and rises along the ladder, the marginal rate falls, and a path's rate is the product of its hops'."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu


def test_price_impact_example(capsys):
    import price_impact
    results, (path, tokens, out, rate, hop_rate, impact) = price_impact.main()     # (its own assertions hold, or it raises)
    text = capsys.readouterr().out
    assert set(results) == {"Product", "GeometricMean", "UniV3", "weighted (3 coins)", "Curve", "Solidly"}
    for name, (o, r, imp) in results.items():
        assert f"{name}: spot rate" in text
        assert o[0] == 0.0 and imp[0] == 0.0 and np.all(np.diff(imp) > 0) and np.all(imp < 1.0), name
        assert np.all(np.diff(o) > 0) and np.all(r > 0), name
        assert np.all(r[1:] < o[1:] / price_impact.SIZES[1:]), name          # the last unit gets less than the average
    assert "execution price" in text and "marginal rate" in text and "impact" in text and "the product of its hops' rates" in text
    assert 1 <= len(path) <= 3 and tokens[0] == 1 and tokens[-1] == 3 and len(tokens) == len(path) + 1
    fold = hop_rate[0]
    for k in range(1, len(path)):
        fold = fold * hop_rate[k]
    np.testing.assert_array_equal(rate, fold)
    assert impact[0] == 0.0 and np.all(np.diff(impact) > 0)
