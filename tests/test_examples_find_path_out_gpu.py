"""examples/find_route_out.py on the device: the cheapest path of at most three pools that buys an exact amount on a mixed
market is found, quoted (the same bits), executed with the found cost as its limit, and the same order afterwards costs more."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import FOUND, FOUND_NONE, SWAP_APPLIED

pytestmark = pytest.mark.gpu


def test_find_route_out_example(capsys):
    import find_route_out
    (found, pools, tokens, status), direct, quoted, (cost, st), (after, pools_after, status_after), (too_much, status_none) = find_route_out.main()
    text = capsys.readouterr().out
    assert "the same bits" in text and "executed" in text and "not executed" not in text and "it costs more" in text
    assert status == FOUND and status_after == FOUND
    assert 1 <= len(pools) <= 3 and len(tokens) == len(pools) + 1 and tokens[0] == 1 and tokens[-1] == 3
    assert 0 < found < direct < math.inf and pools != [0]                  # the route beats the shallow direct pool
    assert quoted == found and st == SWAP_APPLIED and cost == found        # quote_path_out's and swap_path_out_'s bits
    assert found < after < math.inf                                        # the execution moved the market
    assert too_much == math.inf and status_none == FOUND_NONE              # more than any pool holds
