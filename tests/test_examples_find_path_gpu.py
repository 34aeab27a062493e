"""examples/find_route.py on the device: the best path of at most three pools between two tokens of a mixed market is found,
quoted (the same bits), executed with the found amount as its limit, and the same question afterwards gets a worse price."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import FOUND, PATH_APPLIED

pytestmark = pytest.mark.gpu


def test_find_route_example(capsys):
    import find_route
    (found, pools, tokens, status), direct, quoted, (out, st), (after, pools_after, status_after) = find_route.main()
    text = capsys.readouterr().out
    assert "the same bits" in text and "executed" in text and "not executed" not in text and "a worse price" in text
    assert status == FOUND and status_after == FOUND
    assert 1 <= len(pools) <= 3 and len(tokens) == len(pools) + 1 and tokens[0] == 1 and tokens[-1] == 3
    assert found > direct > 0 and pools != [0]                             # the route beats the shallow direct pool
    assert quoted == found and st == PATH_APPLIED and out == found         # quote_path's and swap_path_'s bits
    assert 0 < after < found                                               # the execution moved the market
