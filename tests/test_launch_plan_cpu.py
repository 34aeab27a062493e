"""The launch plan on the CPU: csrc/launch_plan.cpp's plan_launches, built for the host behind tests/native/launch_plan_host.cpp,
against tests/golden/launch_plan_parent.json -- every Segment / Group geometry field and every total that the commit before
the planner existed computed inside ensure_geometry (the file names that commit and says how it was recorded).  The plan
decides every block, grid and row offset of an evaluation, so a change of any of them shows here without a GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "launch_plan_host.cpp")
with open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json"), encoding="utf-8") as f:
    GOLDEN = json.load(f)
CASES = GOLDEN["cases"]

OPTS = ["max_grid", "block", "bin_copies", "direct_small", "fuse_segments", "geomean_exact", "cost_geomean", "cost_univ3", "pack"]
SEG_IN = ["kind", "m", "n_coins", "n_ticks_total", "has_walk", "packed", "n_fees"]
SEG_OUT = ["block", "grid", "row_off", "trade_off", "flat_off", "gbase"]
GROUP_HEAD = ["first", "nseg", "multi", "block", "grid", "row_off", "gtab_n", "xcd_map"]
TOTALS = ["rows", "pools", "trades", "flat", "touched_bytes", "any_ragged"]
GROUP_WORDS = len(GROUP_HEAD) + 32 + 32 + 4
P, G, U, W, C, S = range(6)   # CFMM_KIND_*


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan_launches built with the Makefile's host flags, loaded with ctypes -> plan(case) in the golden file's layout."""
    so = str(tmp_path_factory.mktemp("launch_plan_host") / "launch_plan_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-shared", "-fPIC", SHIM, os.path.join(CSRC, "launch_plan.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip = ctypes.POINTER(ctypes.c_int64)
    lib.launch_plan_host.argtypes = [ctypes.c_int, ip, ctypes.c_int, ip, ip, ip, ip]

    def run(case):
        segs = case["segs"]
        opts = np.array([case["opts"][k] for k in OPTS], dtype=np.int64)
        seg_in = np.array([[s[k] for k in SEG_IN] for s in segs], dtype=np.int64).reshape(len(segs), len(SEG_IN))
        seg_out = np.full((len(segs), len(SEG_OUT)), -7, dtype=np.int64)
        groups = np.full((max(len(segs), 1), GROUP_WORDS), -7, dtype=np.int64)
        totals = np.full(len(TOTALS), -7, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ip)
        ng = lib.launch_plan_host(case["n"], p(opts), len(segs), p(seg_in), p(seg_out), p(groups), p(totals))
        assert 0 <= ng <= len(segs)
        out = {"segs": [dict(zip(SEG_OUT, map(int, row))) for row in seg_out], "groups": []}
        for row in groups[:ng]:
            g = dict(zip(GROUP_HEAD, map(int, row[:8])))
            g.update(pattern=list(map(int, row[8:40])), rank=list(map(int, row[40:72])), seg_w=list(map(int, row[72:76])))
            out["groups"].append(g)
        out.update(zip(TOTALS, map(int, totals)))
        return out

    return run


def test_the_table_names_its_commit_and_covers_the_cases():
    assert "commit 2b56b9c" in GOLDEN["recorded_from"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")) <= 1 << 20
    by_kinds = lambda c: [s["kind"] for s in c["segs"]]
    single_product = [c for c in CASES if by_kinds(c) == [P] and c["n"] <= 8192]
    default = lambda c, **o: all(c["opts"][k] == (o[k] if k in o else d) for k, d in
                                 zip(OPTS, (0, 0, 0, 1, 1, 0, 10, 10, 1)))
    for m in (1, 2048, 2049, 131072, 131073, 1000000, 8000000):
        mine = [c for c in single_product if c["segs"][0]["m"] == m]
        assert any(default(c) for c in mine), m
        assert any(default(c, block=512) for c in mine) and any(default(c, block=1024) for c in mine), m
        assert any(c["opts"]["max_grid"] > 0 for c in mine) and any(default(c, direct_small=0) for c in mine), m
    assert any(c["n"] == 8193 for c in CASES)
    fused = [c for c in CASES if by_kinds(c) == [P, G, U] and c["n"] <= 8192]
    grids = lambda c: [g["grid"] for g in c["expect"]["groups"] if g["multi"]]
    assert any(g % 256 == 0 for c in fused for g in grids(c)) and any(g % 256 != 0 for c in fused for g in grids(c))
    assert any(c["opts"]["cost_geomean"] != 10 and c["opts"]["cost_univ3"] != 10 and c["expect"]["groups"][0]["xcd_map"] for c in fused)
    assert any(c["segs"][2]["n_ticks_total"] > 2 * c["segs"][2]["m"] and c["expect"]["groups"][0]["xcd_map"] for c in fused)
    assert any(c["opts"]["fuse_segments"] == 0 for c in fused) and any(c["opts"]["geomean_exact"] == 1 for c in fused)
    assert any([g["nseg"] for g in c["expect"]["groups"]] == [4, 1] for c in CASES)
    between = lambda kind: any(kind in by_kinds(c)[1:-1] and c["expect"]["groups"][0]["multi"] and c["expect"]["groups"][-1]["multi"]
                               for c in CASES)
    assert between(S) and between(W)
    assert any(not all(s["packed"] for s in c["segs"]) and P in by_kinds(c) for c in CASES)
    assert any(sum(s["n_fees"] for s in c["segs"]) > 256 and len(c["expect"]["groups"]) == 1 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_the_parent_commit(case, plan):
    got, want = plan(case), case["expect"]
    assert got["segs"] == want["segs"]
    assert got["groups"] == want["groups"]
    assert {k: got[k] for k in TOTALS} == {k: want[k] for k in TOTALS}
