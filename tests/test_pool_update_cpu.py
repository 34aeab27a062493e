"""Sparse pool-state updates, the parts that need no GPU: chain.snapshot_delta on examples/data/snapshot.jsonl and
hand-edited copies of it; the three cfmm_pools_set_* entries declared alike in the header, the ctypes binding and the Julia
module; and csrc/univ3_pool.h's per-pool UniV3 preparation (what the upload AND cfmm_pools_set_prices run) built for the
host behind tests/native/univ3_prepare_host.cpp, against the records the commit before that refactor uploaded
(tests/golden/univ3_prepare_parent.npz names the commit and says how it was recorded)."""
import copy
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPSHOT = os.path.join(ROOT, "examples", "data", "snapshot.jsonl")
EXTRA = [   # families the example snapshot does not hold
    {"type": "solidly_stable", "tokens": ["USDC", "DAI"], "decimals": [6, 18], "reserves": ["1000000000000", "1001000000000000000000000"],
     "fee_bps": 5},
    {"type": "curve", "tokens": ["USDC", "DAI", "USDT"], "decimals": [6, 18, 6],
     "balances": ["3000000000000", "3100000000000000000000000", "2900000000000"], "A": 200, "fee": 0.0004},
    {"type": "weighted", "tokens": ["USDC", "DAI", "FRAX"], "decimals": [6, 18, 18],
     "balances": ["500000000000", "510000000000000000000000", "490000000000000000000000"], "weights": [0.4, 0.3, 0.3], "fee": 0.002},
]


def records():
    with open(SNAPSHOT) as f:
        recs = [json.loads(line) for line in f if line.strip() and not line.lstrip().startswith("#")]
    return recs + copy.deepcopy(EXTRA)


def position(recs, k):
    """the position of record k in the concatenated batches of load_snapshot(recs)"""
    _, batches = chain.load_snapshot(recs)
    probe = copy.deepcopy(recs)
    key = "reserves" if "reserves" in probe[k] else "balances"
    if probe[k]["type"] == "concentrated":
        probe[k]["fee_pips"] = 777
    else:
        probe[k][key][0] = str(int(probe[k][key][0]) + 12345678)
    _, moved = chain.load_snapshot(probe)
    base = 0
    for a, b in zip(batches, moved):
        f = "γ" if probe[k]["type"] == "concentrated" else "R"
        rows = np.nonzero(np.any((getattr(a, f) != getattr(b, f)).reshape(len(a), -1), axis=1))[0] if hasattr(a, f) else np.zeros(0)
        if rows.size:
            return base + int(rows[0]), a, int(rows[0])
        base += len(a)
    raise AssertionError("probe changed nothing")


def first(recs, kind, n_tokens=None):
    return next(k for k, r in enumerate(recs) if r["type"] == kind and (n_tokens is None or len(r["tokens"]) == n_tokens))


def test_identical_snapshots_give_an_empty_delta():
    recs = records()
    assert chain.snapshot_delta(chain.load_snapshot(recs), chain.load_snapshot(copy.deepcopy(recs))) == {}
    assert chain.snapshot_delta(chain.load_snapshot(SNAPSHOT)[1], chain.load_snapshot(SNAPSHOT)[1]) == {}


@pytest.mark.parametrize("kind,n_tokens", [("constant_product", 2), ("weighted", 2), ("weighted", 3), ("solidly_stable", 2), ("curve", 3)])
def test_a_moved_reserve_is_found_per_kind(kind, n_tokens):
    recs = records()
    k = first(recs, kind, n_tokens)
    pos, _, _ = position(recs, k)
    new = copy.deepcopy(recs)
    key = "reserves" if "reserves" in new[k] else "balances"
    new[k][key][1] = str(int(new[k][key][1]) * 3 // 2)
    old_s, new_s = chain.load_snapshot(recs), chain.load_snapshot(new)
    delta = chain.snapshot_delta(old_s, new_s)
    assert list(delta) == [pos]
    base = 0
    for b in new_s[1]:
        if pos < base + len(b):
            row = pos - base
            if kind == "curve":
                R, al, be = delta[pos]
                assert (al, be) == (b.α[row], b.β[row]) and be != chain.load_snapshot(recs)[1][-1].β[row]   # D moved with the balances
            else:
                R = delta[pos]
            np.testing.assert_array_equal(R, b.R[row])
            break
        base += len(b)


def test_a_moved_price_is_found():
    recs = records()
    k = first(recs, "concentrated")
    pos, batch, row = position(recs, k)
    new = copy.deepcopy(recs)
    new[k]["sqrt_price_x96"] = str(int(new[k]["sqrt_price_x96"]) * 100001 // 100000)
    new[k].pop("liquidity", None)
    delta = chain.snapshot_delta(chain.load_snapshot(recs), chain.load_snapshot(new))
    assert list(delta) == [pos]
    assert isinstance(delta[pos], float) and delta[pos] > batch.current_price[row]


def test_structural_changes_are_refused_and_name_the_pool():
    recs = records()
    old = chain.load_snapshot(recs)

    def refused(new, match):
        with pytest.raises(cr.ArgumentError, match=match):
            chain.snapshot_delta(old, chain.load_snapshot(new))

    k = first(recs, "constant_product")
    pos, _, _ = position(recs, k)
    new = copy.deepcopy(recs)
    new[k]["fee_bps"] = 5
    refused(new, rf"pool {pos}: fee changed")
    new = copy.deepcopy(recs)
    new[k]["tokens"] = [new[k]["tokens"][1], new[k]["tokens"][0]]
    refused(new, rf"pool {pos}: tokens changed")
    new = copy.deepcopy(recs)          # the same indices, another token behind one of them
    for r in new:
        r["tokens"] = ["WETH" if t == "LUSD" else t for t in r["tokens"]]
    refused(new, r"pool \d+: tokens changed")
    k = first(recs, "concentrated")
    pos, _, _ = position(recs, k)
    new = copy.deepcopy(recs)          # a burn + mint elsewhere: the ladder moves, the tick count stays
    t = new[k]["ticks"]
    t[1][0] = int(t[1][0]) + 10
    new[k].pop("liquidity", None)
    refused(new, rf"pool {pos}: tick ladder changed")
    k = first(recs, "weighted", 2)
    pos, _, _ = position(recs, k)
    new = copy.deepcopy(recs)
    new[k]["weights"] = [0.7, 0.3]
    refused(new, rf"pool {pos}: weights changed")
    refused(copy.deepcopy(recs)[1:], "different pool sets")
    new = copy.deepcopy(recs)
    new[first(recs, "constant_product")]["type"] = "solidly_stable"
    refused(new, "different pool sets")


# ---- the three entries: header, ctypes binding and Julia ccalls agree ---------------------------------------------------
ENTRIES = {
    "cfmm_pools_set_reserves": ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "double*"],
    "cfmm_pools_set_curve": ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "double*", "double*", "double*"],
    "cfmm_pools_set_prices": ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "double*"],
}


def test_header_binding_and_julia_agree_on_the_new_entries():
    from test_julia_binding_static import C2J, c_declarations, julia_ccalls
    decls = c_declarations()
    calls = {name: (ret, args) for name, ret, args in julia_ccalls()}
    lib_src = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    py = {"cfmm_ctx*": "_ctx", "int32_t": "C.c_int32", "int64_t": "C.c_int64", "int64_t*": "_i64p", "double*": "_f64p"}
    for name, want in ENTRIES.items():
        assert decls[name] == ("int", want), name
        m = re.search(r"L\." + name + r"\.argtypes = \[([^\]]*)\]", lib_src)
        assert m and [a.strip() for a in m.group(1).split(",")] == [py[t] for t in want], name
        assert name in calls, f"{name}: no ccall in julia/src/CFMMRouterAMD.jl"
        ret, args = calls[name]
        assert ret in C2J["int"] and len(args) == len(want) and all(a in C2J[c] for a, c in zip(args, want)), name
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    assert re.search(r"^function update_pools!\(r::AMDRouter", jl, flags=re.M) and "update_pools!" in re.search(r"^export (.*)$", jl, flags=re.M).group(1)
    for verb in ("set_reserves", "set_curve", "set_prices"):
        assert callable(getattr(cr.Context, verb))
    assert callable(cr.update_pools_)


# ---- the per-pool UniV3 preparation reproduces the records of the upload before the refactor ------------------------------
def test_univ3_prepare_pool_reproduces_the_parents_upload(tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "univ3_prepare_parent.npz"))
    assert re.fullmatch(r"[0-9a-f]{40}", str(g["commit"])) and "univ3_build" in str(g["note"])
    so = str(tmp_path / "univ3_prepare_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"), "-O3", "-std=c++17", "-ffp-contract=off", "-mavx2", "-shared",
                    "-fPIC", os.path.join(ROOT, "tests", "native", "univ3_prepare_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.univ3_prepare_host.restype = ctypes.c_longlong
    lib.univ3_prepare_host.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 14
    cp, gamma, off = g["current_price"], g["gamma"], g["tick_off"]
    m, W = cp.size, int(g["ticks"].shape[0])
    assert m >= 200 and np.diff(off).min() == 1 and np.diff(off).max() == 12 and (g["liquidity"] == 0).any()
    out = {k: np.full_like(g[k], 77) for k in ("pg", "cur_a", "cur_b", "cur_c", "curR", "walk", "head")}
    ticks, thr = np.full((int(off[-1]) + 2 * m, 8), 77.0), np.full(int(off[-1]) + 2 * m + 4, 77.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lt, lq = np.ascontiguousarray(g["lower_ticks"]), np.ascontiguousarray(g["liquidity"])
    n = lib.univ3_prepare_host(m, p(cp), p(gamma), p(off), p(lt), p(lq), p(out["pg"]), p(out["cur_a"]), p(out["cur_b"]),
                               p(out["cur_c"]), p(out["curR"]), p(out["walk"]), p(ticks), p(thr), p(out["head"]))
    assert n == W
    for k, a in out.items():
        np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      g[k].view(np.uint64) if a.dtype == np.float64 else g[k], err_msg=k)
    np.testing.assert_array_equal(ticks[:W].view(np.uint64), g["ticks"].view(np.uint64))
    np.testing.assert_array_equal(thr[:W + 4].view(np.uint64), g["thr"].view(np.uint64))
