"""The query kernels answer with the bits they answered with before their device code was folded into shared bodies
(kind_switch.h, query_read.h, one quote body, one post-swap state, one two-way search): tests/golden/query_bits.npz holds
every answer of every query entry on the market of tests/query_bits_record.py, recorded on the MI355X with the library of the
commit before the fold, and this build must give every one of them again -- amounts, hop arrays, statuses, the pool state
the moving entries leave and the trades of a sweep on that state (which reads the prepared constants they refreshed) -- as
unsigned integers, so NaN payloads and the sign of zero count."""
import os

import numpy as np
import pytest

import cfmmrouter_amd as cr
import query_bits_record as rec
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import FOUND, PATH_APPLIED, SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, SWAP_UNOBTAINABLE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_bits.npz")


@pytest.fixture(scope="module")
def both():
    assert os.path.getsize(GOLDEN) < 1 << 20
    with np.load(GOLDEN) as z:
        want = {k: z[k] for k in z.files if k != "commit"}
    return rec.record_all(cr, synth), want


def test_every_answer_of_every_query_entry_keeps_its_bits(both):
    got, want = both
    assert sorted(got) == sorted(want)
    differ = []
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        n = int(np.sum(rec.as_words(got[k]) != rec.as_words(want[k])))
        if n:
            differ.append(f"{k}: {n} of {want[k].size} words")
    print(f"query bits: {len(want)} arrays, {sum(v.size for v in want.values())} words compared")
    assert not differ, differ


def test_the_record_holds_the_cases_the_readers_exist_for(both):
    """on the stored record alone: the comparison above is one of refusals, limits, poisoned queries and found paths, not of
    empty answers"""
    _, w = both
    for s in range(6):
        for name in ("quote", "quote_out"):
            dev = w[f"{name}_dev{s}"]
            bad = [3, 4, 5, 10, 11, 12, 13, 14, 20, 21, 22, 23]
            assert np.all(np.isnan(dev[bad])) and np.sum(np.isnan(dev)) < 60, (name, s)
            assert np.any(w[f"{name}{s}"] == 0.0)
        assert np.any(np.isinf(w[f"quote_out{s}"]))
        st = w[f"swap_out{s}.status"]
        assert all(np.any(st == code) for code in (SWAP_APPLIED, SWAP_UNOBTAINABLE, SWAP_OVER_LIMIT)), (s, np.bincount(st))
    assert any(np.any(w[f"swap_out{s}.status"] == SWAP_REFUSED) or np.any(np.isnan(w[f"swap{s}"])) for s in range(6))
    spoilt = [40, 41, 42, 50, 51, 52, 59, 60, 61, 70, 71, 72, 73, 74, 80, 81, 82]
    for name in ("quote_path_dev", "size_path_dev.amount_in"):
        assert np.all(np.isnan(w[name][spoilt])), name
    back = w["quote_path_out_dev"][spoilt]                             # walked from the last hop: +inf may arrive before the bad hop is read
    assert np.all(np.isnan(back) | (back == np.inf)) and np.sum(np.isnan(back)) >= 12
    assert np.any(w["swap_path.status"] == PATH_APPLIED) and np.any(w["swap_path.status"] != PATH_APPLIED)
    assert np.any(w["swap_path_out.status"] == SWAP_APPLIED) and np.any(w["swap_path_out.status"] == SWAP_OVER_LIMIT)
    for name in ("find_path", "find_path_out"):
        assert np.sum(w[f"{name}.lds1.status"] == FOUND) > rec.FIND // 2 and np.any(w[f"{name}.lds1.n_hops"] > 1)
        assert np.array_equal(w[f"{name}.lds1.amount"].view(np.uint64), w[f"{name}.lds0.amount"].view(np.uint64))
