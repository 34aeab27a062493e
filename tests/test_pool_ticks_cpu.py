"""UniV3 mints and burns, the parts that need no GPU: chain.snapshot_delta(..., ladders=True) on hand-edited copies of
examples/data/snapshot.jsonl; cfmm_pools_set_ticks declared alike in the header, the ctypes binding and the Julia module;
update_pools_ on a backend without a device context; and csrc/ladder_store.h (the host's tick ladders) driven by
tests/native/ladder_store_host.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain
from test_pool_update_cpu import first, position, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def concentrated(recs, nth=0):
    return [k for k, r in enumerate(recs) if r["type"] == "concentrated"][nth]


def edited(recs, k, edit):
    new = copy.deepcopy(recs)
    edit(new[k]["ticks"])
    new[k].pop("liquidity", None)          # (the active liquidity follows from the ticks)
    return new


def burn_and_mint_elsewhere(t):            # the ladder moves, the tick count stays
    t[1][0] = int(t[1][0]) + 10


def mint_adds_a_tick(t):                   # +L at a new lower tick, -L at an initialised upper one
    L = 10 ** 12
    t.insert(2, [int(t[1][0]) + 20, str(L)])
    t[4][1] = str(int(t[4][1]) - L)


def burn_removes_a_tick(t):                # an initialised tick is cleared; its liquidity starts at the next one
    gone = t.pop(2)
    t[2][1] = str(int(t[2][1]) + int(gone[1]))


@pytest.mark.parametrize("edit,ticks", [(burn_and_mint_elsewhere, 0), (mint_adds_a_tick, +1), (burn_removes_a_tick, -1)])
def test_a_changed_ladder_yields_the_three_part_state(edit, ticks):
    recs = records()
    k = concentrated(recs, 1)
    pos, batch, row = position(recs, k)
    new = edited(recs, k, edit)
    old_s, new_s = chain.load_snapshot(recs), chain.load_snapshot(new)
    with pytest.raises(cr.ArgumentError, match=rf"pool {pos}: tick ladder changed"):       # the default is unchanged
        chain.snapshot_delta(old_s, new_s)
    delta = chain.snapshot_delta(old_s, new_s, ladders=True)
    assert list(delta) == [pos]
    price, lt, lq = delta[pos]
    nb = next(b for b in new_s[1] if hasattr(b, "tick_off"))
    o, e = nb.tick_off[row], nb.tick_off[row + 1]
    assert isinstance(price, float) and price == nb.current_price[row] == batch.current_price[row]
    np.testing.assert_array_equal(lt, nb.lower_ticks[o:e])
    np.testing.assert_array_equal(lq, nb.liquidity[o:e])
    assert lt.size == batch.tick_off[row + 1] - batch.tick_off[row] + ticks
    assert np.all(np.diff(lt) < 0) and price <= lt[0]                                       # the form cfmm_pools_set_ticks takes


def test_a_ladder_and_a_price_move_in_one_delta():
    recs = records()
    k0, k1 = concentrated(recs, 0), concentrated(recs, 2)
    new = edited(recs, k0, mint_adds_a_tick)
    new[k0]["sqrt_price_x96"] = str(int(new[k0]["sqrt_price_x96"]) * 100001 // 100000)   # the minted pool's price moved too
    new[k1]["sqrt_price_x96"] = str(int(new[k1]["sqrt_price_x96"]) * 100001 // 100000)   # a swap only
    new[k1].pop("liquidity", None)
    delta = chain.snapshot_delta(chain.load_snapshot(recs), chain.load_snapshot(new), ladders=True)
    p0, p1 = position(recs, k0)[0], position(recs, k1)[0]
    assert sorted(delta) == sorted([p0, p1])
    assert isinstance(delta[p0], tuple) and len(delta[p0]) == 3 and isinstance(delta[p1], float)
    assert delta[p0][0] > position(recs, k0)[1].current_price[position(recs, k0)[2]]
    assert chain.snapshot_delta(chain.load_snapshot(recs), chain.load_snapshot(copy.deepcopy(recs)), ladders=True) == {}


def test_tokens_and_fees_still_raise_with_ladders():
    recs = records()
    old = chain.load_snapshot(recs)
    k = concentrated(recs, 1)
    pos = position(recs, k)[0]
    new = edited(recs, k, mint_adds_a_tick)
    new[k]["fee_pips"] = 3000 if new[k]["fee_pips"] != 3000 else 500
    with pytest.raises(cr.ArgumentError, match=rf"pool {pos}: fee changed"):
        chain.snapshot_delta(old, chain.load_snapshot(new), ladders=True)
    new = edited(recs, k, mint_adds_a_tick)
    new[k]["tokens"] = [new[k]["tokens"][1], new[k]["tokens"][0]]
    with pytest.raises(cr.ArgumentError, match=rf"pool {pos}: tokens changed"):
        chain.snapshot_delta(old, chain.load_snapshot(new), ladders=True)
    with pytest.raises(cr.ArgumentError, match="different pool sets"):
        chain.snapshot_delta(old, chain.load_snapshot(copy.deepcopy(recs)[1:]), ladders=True)
    new = copy.deepcopy(recs)
    new[first(recs, "constant_product")]["type"] = "solidly_stable"
    with pytest.raises(cr.ArgumentError, match="different pool sets"):
        chain.snapshot_delta(old, chain.load_snapshot(new), ladders=True)


class HostOnlyBackend:
    """a backend without a device context: update_pools_' only door is a reload"""

    def __init__(self):
        self.reloads = 0

    def reload(self, batches):
        self.reloads += 1


def test_the_host_backend_refuses_a_ladder_state():
    lt, lq = [30.0, 20.0, 10.0], [1e6, 0.0, 2e6]
    pools = [cr.UniV3(15.0, lt, lq, 0.997, [1, 2]), cr.UniV3(12.0, lt, lq, 1.0, [2, 3])]
    be = HostOnlyBackend()
    r = cr.Router(cr.LinearNonnegative(np.ones(3)), pools, 3, _backend=be)
    with pytest.raises(NotImplementedError, match="cannot change a UniV3 pool's tick ladder .*cfmm_pools_set_ticks"):
        cr.update_pools_(r, {0: (15.0, [30.0, 20.0, 10.0, 5.0], [1e6, 0.0, 2e6, 1e5])})
    assert be.reloads == 0
    b = r._batches[0]
    np.testing.assert_array_equal(b.tick_off, [0, 3, 6])                                    # the host mirror is as it was
    np.testing.assert_array_equal(b.lower_ticks, lt + lt)
    cr.update_pools_(r, {1: 11.0})                                                          # a bare price still goes through
    assert be.reloads == 1 and b.current_price[1] == 11.0


def test_header_binding_and_julia_agree_on_set_ticks():
    from test_julia_binding_static import C2J, c_declarations, julia_ccalls
    name, want = "cfmm_pools_set_ticks", ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "double*", "int64_t*", "double*", "double*"]
    assert c_declarations()[name] == ("int", want)
    lib_src = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    py = {"cfmm_ctx*": "_ctx", "int32_t": "C.c_int32", "int64_t": "C.c_int64", "int64_t*": "_i64p", "double*": "_f64p"}
    m = re.search(r"L\." + name + r"\.argtypes = \[([^\]]*)\]", lib_src)
    assert m and [a.strip() for a in m.group(1).split(",")] == [py[t] for t in want]
    calls = {n: (ret, args) for n, ret, args in julia_ccalls()}
    assert name in calls, f"{name}: no ccall in julia/src/CFMMRouterAMD.jl"
    ret, args = calls[name]
    assert ret in C2J["int"] and len(args) == len(want) and all(a in C2J[c] for a, c in zip(args, want))
    assert callable(cr.Context.set_ticks)


def test_ladder_store_against_a_list_of_vectors_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ladder_store_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ladder_store_host.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, "6000"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "LADDER_STORE_OK 6000 steps x 3 markets" in r.stdout
