"""The Python host mirror (router.py, cfmms.py, layout.py) against the commit before it was consolidated around PoolLayout
and the kind table: the Context calls it makes and the arrays it hands back, recorded there by
tests/golden/make_host_mirror_golden.py (tests/golden/host_mirror_parent.json names the commit), must be the same here.
Then PoolLayout's own answers.  No GPU and no shared library: host_mirror_record.RecordingContext stands in."""
import json
import os
import re

import numpy as np
import pytest

import cfmmrouter_amd as cr
import host_mirror_record as rec
from cfmmrouter_amd import _lib, objectives, router
from cfmmrouter_amd.layout import PoolLayout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_mirror_parent.json")


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{40}", g["commit"]) and set(g["scenarios"]) == set(rec.SCENARIOS)
    return g["scenarios"]


@pytest.mark.parametrize("name", list(rec.SCENARIOS))
def test_context_calls_and_results_are_the_parents(parent, name, monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the shared library was loaded"))
    now = json.loads(json.dumps(rec.record_scenario(name)))
    assert router.Context is _lib.Context                                  # the patch is gone again
    assert [s["step"] for s in now] == [s["step"] for s in parent[name]]
    for got, want in zip(now, parent[name]):
        assert got == want, got["step"]


def test_the_record_covers_what_it_is_meant_to(parent):
    calls = lambda name, step: [c[0] for s in parent[name] if s["step"] == step for c in s["calls"]]
    assert calls("mixed", "upload") == ["Context", "add_product", "add_geomean", "add_univ3", "add_solidly", "add_weighted",
                                        "add_weighted", "add_curve", "add_curve"]
    assert calls("batches", "upload") == ["Context", "add_product", "add_univ3", "add_curve"]       # the empty batch: no segment
    assert set(calls("mixed", "update_pools")) == {"set_reserves", "set_curve", "set_ticks"} and "set_prices" in calls("two_coin_in_order", "update_pools")
    assert [c for s in parent["two_coin_in_order"] if s["step"] == "trades" for c in s["calls"]] == [["trades", "out"]]
    for name in ("mixed", "batches", "single_batch", "two_coin_in_order"):
        by = {s["step"]: s for s in parent[name]}
        assert by["update_pools"]["error"] is None
        assert "out of range 0:" in by["update_pools out of range"]["error"] and "pool -1 " in by["update_pools out of range"]["negative"]
        refused = by["update_pools refused on the host"]
        assert refused["error"].startswith("ArgumentError: new state of a ") and refused["calls"] == []
        assert refused["state"] == "unchanged" and by["update_pools out of range"]["state"] != "unchanged"   # nothing moved
        assert by["update_pools refused by the context"]["error"].startswith("ArgumentError: recording context")
    assert calls("mixed", "update_pools refused by the context") == ["set_reserves", "set_reserves"]   # not the segment after it
    assert calls("batches", "route native LinearNonnegative") == ["route", "dual_value"] and calls("batches", "polish native") == ["polish", "dual_value"]
    assert calls("mixed", "route native LinearNonnegative").count("fg") == 4 and calls("mixed", "route native LinearNonnegative").count("eval") == 3


def test_native_polish_refuses_an_unknown_objective_like_native_route():
    class Other(objectives.Objective):
        pass

    with rec.recording() as log:
        r = cr.Router(cr.LinearNonnegative(np.ones(rec.N_TOKENS)), rec.two_coin_in_order(), rec.N_TOKENS)
        r.objective = Other()
        for call in (lambda: cr.route_(r, solver="native"), lambda: cr.polish_(r, native=True)):
            with pytest.raises(cr.ArgumentError, match="solver='native' knows LinearNonnegative and BasketLiquidation"):
                call()
        assert not [c for c in log if c[0] in ("route", "polish")]


def test_a_plugin_pool_names_its_own_fields():
    """CFMM is the plugin seam: it defines no `gamma` (the built-in types do), so a user's type may store one."""
    assert rec.PluginPool([1.0, 2.0], [1, 2]).gamma == 0.997 and not hasattr(cr.CFMM, "gamma")
    assert cr.ProductTwoCoin([1.0, 2.0], 0.9, [1, 2]).gamma == 0.9 and cr.Product([1.0, 2.0, 3.0], 0.9, [1, 2, 3]).gamma == 0.9


# ---- PoolLayout ----------------------------------------------------------------------------------------------------------
def layouts():
    out = {}
    for name in ("mixed", "all_host", "batches"):
        pools = rec.SCENARIOS[name][0]()
        out[name] = (pools, PoolLayout(*router._segments_of(pools)))
    return out


@pytest.mark.parametrize("name", ["mixed", "all_host", "batches"])
def test_locate_and_place_are_inverse(name):
    pools, L = layouts()[name]
    n = sum(len(b) for b in pools) if name == "batches" else len(pools)
    assert L.n_pools == n and sorted(L.place.tolist()) == list(range(n))
    for i in range(n):
        where = L.locate(i)
        k = L.m + where[1] if where[0] == "host" else int(L.offsets[where[1]]) + where[2]
        assert L.place[k] == i
        if name != "batches":
            if where[0] == "host":
                assert isinstance(pools[i], rec.PluginPool) and L.host[where[1]] == i
            else:
                b = L.batches[where[1]]
                assert b.kind == pools[i].kind and np.array_equal(b.Ai[where[2]], pools[i].Ai)
    for bad in (-1, n):
        with pytest.raises(cr.ArgumentError, match=rf"pool {bad} out of range 0:{n - 1}"):
            L.locate(bad)


@pytest.mark.parametrize("name", ["mixed", "all_host", "batches"])
def test_segments_skip_empties_and_number_from_zero(name):
    pools, L = layouts()[name]
    segs = L.segments()
    assert [s for s, _, _ in segs] == list(range(len(segs))) and all(len(b) for _, _, b in segs)
    assert [b for _, _, b in segs] == [b for b in L.batches if len(b)]
    assert [first for _, first, _ in segs] == [int(L.offsets[i]) for i, b in enumerate(L.batches) if len(b)]
    assert L.coins == [b.Ai.shape[1] for _, _, b in segs]
    if name == "batches":
        assert len(L.batches) == 4 and len(segs) == 3 and L.seg_of == {0: 0, 2: 1, 3: 2}
    if name == "all_host":
        assert segs == [] and L.m == 0 and not L.ragged and L.per_pool


@pytest.mark.parametrize("name", ["mixed", "all_host"])
def test_to_router_of_split_puts_each_pools_vector_at_its_router_position(name):
    pools, L = layouts()[name]
    flat = np.concatenate([np.full(b.Ai.shape[1], 100.0 * s + row) for s, b in enumerate(L.batches) for row in range(len(b))] or [np.zeros(0)])
    host_rows = [np.full(len(pools[i].Ai), -1.0 - i) for i in L.host]
    rows = L.to_router(L.split(flat), host_rows)
    assert len(rows) == len(pools)
    for i, row in enumerate(rows):
        where = L.locate(i)
        want = -1.0 - i if where[0] == "host" else 100.0 * where[1] + where[2]
        assert row.shape == (len(pools[i].Ai),) and np.all(row == want)
