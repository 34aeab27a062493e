"""examples/execute_cycle.py on the device: a 3-pool cycle quoted at a ladder of sizes, the best one executed with a limit of
its own input, and a second execution that no longer clears it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import PATH_APPLIED, PATH_BELOW_LIMIT

pytestmark = pytest.mark.gpu


def test_execute_cycle_example(capsys):
    import execute_cycle
    quotes, best, first, second = execute_cycle.main()
    out = capsys.readouterr().out
    assert "executed" in out and "below the limit" in out
    assert first[1] == PATH_APPLIED and second[1] == PATH_BELOW_LIMIT
    assert 0 < best < len(quotes) - 1                                                  # the ladder reaches past the best size
    assert first[0] == quotes[best][1] and first[0] >= quotes[best][0] > second[0] > 0     # the quote's bits; the cycle paid, once
