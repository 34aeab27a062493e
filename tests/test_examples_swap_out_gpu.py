"""examples/buy_exact.py on the device: an exact amount bought through a 3-hop path with a cost limit, and the same purchase
rejected by its limit after another trade moved a pool of the path."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cfmmrouter_amd._lib import SWAP_APPLIED, SWAP_OVER_LIMIT  # noqa: E402

pytestmark = pytest.mark.gpu


def test_buy_exact_example(capsys):
    import buy_exact
    quoted, limit, first, second, untouched = buy_exact.main()
    out = capsys.readouterr().out
    assert "executed" in out and "over the limit, nothing moved" in out
    assert first == (quoted, SWAP_APPLIED)                                  # the quote's bits
    assert second[1] == SWAP_OVER_LIMIT and second[0] > limit > quoted > 0 and untouched
