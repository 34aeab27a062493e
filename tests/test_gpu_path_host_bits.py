"""The order-level path entries answer with the bits they answered with before their host side was folded into one read-only
rig (path_rig.h), one driver of the executing entries (abi_swap_path.cpp swap_paths_run over swap_fill.h) and one parent search
(split_search.h): tests/golden/path_host_bits.npz holds every answer of split_paths, split_paths_out, their _dev forms,
swap_order and swap_order_out -- amounts, totals, hop amounts, statuses, the wave count, the pool state the executions leave and
the trades of a sweep on it -- and of quote_path, size_path and both splits on a two-shard parent, on the market of
tests/path_host_bits_record.py, recorded on the MI355X with the library of the commit before the fold.  This build must give
every word again, compared as unsigned integers, so NaN payloads and the sign of zero count."""
import os

import numpy as np
import pytest

import cfmmrouter_amd as cr
import path_host_bits_record as rec
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import (ORDER_APPLIED, ORDER_LIMIT, ORDER_PATH_HELD, ORDER_REFUSED, ORDER_UNOBTAINABLE, PATH_APPLIED, PATH_REFUSED,
                                 SPLIT_NONE, SPLIT_OK, SPLIT_UNOBTAINABLE, SWAP_REFUSED)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_host_bits.npz")


@pytest.fixture(scope="module")
def stored():
    """the record as it is stored: nothing of this build runs"""
    assert os.path.getsize(GOLDEN) < 1 << 20
    with np.load(GOLDEN) as z:
        assert len(str(z["commit"])) == 40
        return {k: z[k] for k in z.files if k != "commit"}


def test_every_answer_of_the_order_level_entries_keeps_its_bits(stored):
    got, want = rec.record_all(cr, synth), stored
    assert sorted(got) == sorted(want)
    differ = []
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        n = int(np.sum(rec.as_words(got[k]) != rec.as_words(want[k])))
        if n:
            differ.append(f"{k}: {n} of {want[k].size} words")
    print(f"path host bits: {len(want)} arrays, {sum(v.size for v in want.values())} words compared")
    assert not differ, differ


def test_the_record_holds_the_cases_the_rigs_exist_for(stored):
    """on the stored record alone: the comparison above is one of several waves with UniV3 moves between them, of limits,
    refusals and unobtainable orders, and of parent answers that equal the single context's -- not of empty answers"""
    w = stored
    for name in ("swap_order", "swap_order_out"):
        launches, waves, refused = w[f"{name}.launches"].tolist()
        st, pst = w[f"{name}.status"], w[f"{name}.path_status"]
        assert launches == waves >= 3 and refused == np.sum(st != ORDER_APPLIED), (name, launches, waves, refused)
        assert st[rec.LIMIT_ORDER] == ORDER_LIMIT and np.any(st == ORDER_APPLIED), (name, np.bincount(st))
        assert np.any(pst == ORDER_PATH_HELD) and np.any(pst == PATH_APPLIED)
        assert np.any(w[f"{name}.state2"] != w[f"{name}.price_before"]), name              # a UniV3 pool moved
        assert np.all(np.isfinite(w[f"{name}.state2"])) and np.any(w[f"{name}.sweep_delta"] != 0)
        assert np.any(np.isfinite(w[f"{name}.hops"]) & (w[f"{name}.hops"] > 0))
    first = rec.order_first_of(rec.EXEC_ORDERS, rec.EXEC_KS)
    for name, code in (("swap_order", PATH_REFUSED), ("swap_order_out", SWAP_REFUSED)):   # the refusing hop, both directions
        assert w[f"{name}.status"][rec.REFUSING_ORDER] == ORDER_REFUSED and w[f"{name}.path_status"][first[rec.REFUSING_ORDER]] == code, name
        assert np.isnan(w[f"{name}.total"][rec.REFUSING_ORDER]) and np.isnan(w[f"{name}.path"][first[rec.REFUSING_ORDER]]), name
        held = w[f"{name}.path_status"][first[rec.REFUSING_ORDER] + 1:first[rec.REFUSING_ORDER + 1]]
        assert held.size == 3 and np.all(held == ORDER_PATH_HELD), (name, held)               # its siblings pass and are held
    assert w["swap_order_out.status"][rec.UNOBTAINABLE_ORDER] == ORDER_UNOBTAINABLE and np.isinf(w["swap_order_out.total"][rec.UNOBTAINABLE_ORDER])
    for name in ("split_paths", "split_paths_out"):
        for form in ("", "_dev"):
            st = w[f"{name}{form}.status"]
            assert st[rec.NONE_ORDER] == SPLIT_NONE and np.any(st == SPLIT_OK), (name, form, np.bincount(st))
            assert np.array_equal(rec.as_words(w[f"{name}{form}.x"]), rec.as_words(w[f"{name}.x"]))   # the _dev form: the same arrays
            assert np.array_equal(rec.as_words(w[f"{name}{form}.total"]), rec.as_words(w[f"{name}.total"]))
    assert w["split_paths_out.status"][rec.UNOBTAINABLE_ORDER] == SPLIT_UNOBTAINABLE
    # the parent: a search of ROUNDS inner calls that answers the single context's words
    assert w["parent.launches"].tolist() == [rec.ROUNDS] * 3 and w["single.launches"].tolist() == [1, 1, 1]
    keys = [k for k in w if k.startswith("parent.") and k != "parent.launches"]
    assert len(keys) == 14
    for k in keys:
        assert np.array_equal(rec.as_words(w[k]), rec.as_words(w["single." + k[len("parent."):]])), k
    assert np.any(w["parent.split_paths.total"] > 0) and np.any(w["parent.size_path.amount_in"] > 0) and np.any(w["parent.quote_path"] > 0)
