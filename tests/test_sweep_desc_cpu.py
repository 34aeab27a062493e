"""The sweep descriptors on the CPU: csrc/launch_plan.cpp's build_sweep_desc, built for the host behind
tests/native/sweep_desc_host.cpp.  The descriptor's block table tells every block of a sweep_kernel / sweep_multi launch which
pools it sweeps and which partial row it writes; a wrong record is an out-of-bounds load on the device.  So, for every plan
shape of tests/test_launch_plan_cpu.py and for the benchmark's markets, WITHOUT a GPU:
  - every record equals the map the kernels computed on the device before the table existed, restated here (the two forms of
    sweep_multi, blockIdx / gridDim for a segment's own launch), lane by lane: the same pools, in the same order;
  - every pool of every segment is covered exactly once, no record reaches past its segment's m;
  - every block has a record, no two blocks share a partial row."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "sweep_desc_host.cpp")
with open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json"), encoding="utf-8") as f:
    PLAN_CASES = json.load(f)["cases"]

OPTS = ["max_grid", "block", "bin_copies", "direct_small", "fuse_segments", "geomean_exact", "cost_geomean", "cost_univ3", "pack"]
DEFAULTS = dict(zip(OPTS, (0, 0, 0, 1, 1, 0, 10, 10, 1)))
SEG_IN = ["kind", "m", "n_coins", "n_ticks_total", "has_walk", "packed", "n_fees"]
GROUP_HEAD = ["first", "nseg", "multi", "block", "grid", "row_off", "gtab_n", "xcd_map"]
GROUP_WORDS = len(GROUP_HEAD) + 32 + 32 + 4 + 3 + 4
REC = ["group", "block", "seg", "kind", "first", "stride", "full", "tail", "row"]
P, G, U, W, C, S = range(6)   # CFMM_KIND_*
RAGGED = (W, C)


def seg(kind, m, ticks_per_pool=0):
    return {"kind": kind, "m": m, "n_coins": 2, "n_ticks_total": m * ticks_per_pool, "has_walk": 1, "packed": 1, "n_fees": 1}


def market(name, n, segs, **opts):
    return {"name": name, "n": n, "opts": {**DEFAULTS, **opts}, "segs": segs}


# the benchmark's markets (benchlib/workloads.py), and the shapes of tests/test_gpu_sweep_entry.py
BENCH_CASES = [
    market("config3", 256, [seg(P, 500000), seg(G, 500000)]),
    market("config2", 64, [seg(P, 100000)]),
    market("product1m", 256, [seg(P, 1000000)]),
    market("config5", 256, [seg(U, 1000000, 2)]),
    market("config4shard", 512, [seg(P, 500000)]),
    market("univ3_ticks", 256, [seg(U, 1000000, 17)]),
] + [market("single_%d" % m, 16, [seg(P, m)]) for m in (1, 511, 513, 2048, 2049, 70001, 140000)] + [
    market("single_140000_tiles", 16, [seg(P, 140000)], max_grid=32),
    market("fused_1500", 16, [seg(P, 1500), seg(G, 1500)]),
    # 129 tiles of 512 each: "max_grid" = 256 gives the fused launch 2 x 128 blocks, a multiple of 256 (the XCD-aware map), and
    # the first block of each segment a second, partial tile
    market("fused_65600", 48, [seg(P, 65600), seg(G, 65600)], max_grid=256),
    market("fused_65600_cost", 48, [seg(P, 65600), seg(G, 65600)], max_grid=256, cost_geomean=40),
    market("fused_3", 16, [seg(P, 5000), seg(G, 3), seg(U, 1777, 2)]),
    market("fused_4", 16, [seg(P, 3), seg(G, 4099), seg(U, 70001, 2), seg(P, 513)]),
    market("fused_ncoin_between", 16, [seg(P, 3000), seg(G, 2000), dict(seg(W, 700), n_coins=3), seg(P, 1000), seg(U, 900, 2)]),
    market("gbins_3000", 8200, [seg(P, 3000)]),
    market("fused_max_grid_6", 16, [seg(P, 5000), seg(G, 7000)], max_grid=6),
]
CASES = PLAN_CASES + BENCH_CASES


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sweep_desc_host") / "sweep_desc_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-shared", "-fPIC", SHIM, os.path.join(CSRC, "launch_plan.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip = ctypes.POINTER(ctypes.c_int64)
    lib.sweep_desc_host.argtypes = [ctypes.c_int, ip, ctypes.c_int, ip, ip, ip, ip, ctypes.c_int64, ip]
    lib.sweep_desc_host.restype = ctypes.c_int64

    def run(case):
        segs = case["segs"]
        opts = np.array([case["opts"][k] for k in OPTS], dtype=np.int64)
        seg_in = np.array([[s[k] for k in SEG_IN] for s in segs], dtype=np.int64).reshape(len(segs), len(SEG_IN))
        groups = np.full((max(len(segs), 1), GROUP_WORDS), -7, dtype=np.int64)
        cap = 1 << 16
        recs = np.full((cap, len(REC)), -7, dtype=np.int64)
        ng, nbytes = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ip)
        nrec = lib.sweep_desc_host(case["n"], p(opts), len(segs), p(seg_in), p(groups), p(ng), p(recs), cap, p(nbytes))
        assert nrec >= 0, nrec
        out = []
        for row in groups[:int(ng[0])]:
            g = dict(zip(GROUP_HEAD, map(int, row[:8])))
            g.update(pattern=row[8:40].copy(), rank=row[40:72].copy(), seg_w=row[72:76].copy(), off=int(row[76]),
                     d_nseg=int(row[77]), d_grid=int(row[78]), d_m=list(map(int, row[79:83])))
            out.append(g)
        return out, recs[:nrec], int(nbytes[0])

    return run


def parent_map(g, b):
    """{segment of the launch, block of that segment, blocks of that segment} of blocks b, as the kernels computed them"""
    if g["multi"] and g["xcd_map"]:
        x, j = b & 7, b >> 3
        q = j >> 5
        p = (j + q) & 31
        sidx = g["pattern"][p]
        w = g["seg_w"][sidx]
        return sidx, (q * w + g["rank"][p]) * 8 + x, (g["grid"] >> 8) * w * 8
    if g["multi"]:
        nb = g["grid"] // g["nseg"]
        return b % g["nseg"], b // g["nseg"], np.full_like(b, nb)
    return np.zeros_like(b), b, np.full_like(b, g["grid"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_block_records_restate_the_device_maps(case, desc):
    groups, recs, nbytes = desc(case)
    segs = case["segs"]
    rows_seen = []
    end = 0
    for gi, g in enumerate(groups):
        first_kind = segs[g["first"]]["kind"]
        mine = recs[recs[:, 0] == gi]
        if first_kind in RAGGED:                       # sweep_ncoin keeps plain arguments
            assert g["off"] == -1 and len(mine) == 0
            continue
        # the descriptors follow each other, 128-byte aligned, inside the byte block
        assert g["off"] == end and g["off"] % 128 == 0
        assert g["d_nseg"] == g["nseg"] and g["d_grid"] == g["grid"]
        assert g["d_m"][:g["nseg"]] == [segs[g["first"] + k]["m"] for k in range(g["nseg"])]
        # every block has a record, in block order, with its own row
        assert len(mine) == g["grid"] and np.array_equal(mine[:, 1], np.arange(g["grid"]))
        r = dict(zip(REC, mine.T))
        assert np.array_equal(r["row"], r["block"])
        rows_seen.append(g["row_off"] + r["row"])
        sidx, local, nblocks = parent_map(g, r["block"])
        block = g["block"]
        assert np.array_equal(r["seg"], sidx)
        assert np.array_equal(r["kind"], np.array([segs[g["first"] + int(s)]["kind"] for s in sidx], dtype=np.int64))
        m = np.array([segs[g["first"] + int(s)]["m"] for s in sidx], dtype=np.int64)
        stride = nblocks * block
        assert np.array_equal(r["first"], local * block) and np.array_equal(r["stride"], stride)
        assert np.all(r["full"] >= 0) and np.all((r["tail"] >= 0) & (r["tail"] < block))
        # lane by lane: tiles of lane t = ceil((m - i0) / stride) for i0 = local * block + t < m, else 0
        t = np.arange(block, dtype=np.int64)[None, :]
        i0 = (local * block)[:, None] + t
        left = np.where(i0 < m[:, None], (m[:, None] - i0 + stride[:, None] - 1) // stride[:, None], 0)
        assert np.array_equal(r["full"][:, None] + (t < r["tail"][:, None]), left)
        # nothing reaches past m
        last_full = r["first"] + (block - 1) + (r["full"] - 1) * r["stride"]
        last_tail = r["first"] + (r["tail"] - 1) + r["full"] * r["stride"]
        assert np.all(np.where(r["full"] > 0, last_full, -1) < m) and np.all(np.where(r["tail"] > 0, last_tail, -1) < m)
        # every pool exactly once: whole tiles (first and stride are multiples of the block size), the last one partial
        for k in range(g["nseg"]):
            mk = segs[g["first"] + k]["m"]
            sel = sidx == k
            tiles = np.zeros((mk + block - 1) // block, dtype=np.int64)
            for f, s, full, tail in zip(r["first"][sel], r["stride"][sel], r["full"][sel], r["tail"][sel]):
                assert f % block == 0 and s % block == 0 and s > 0
                idx = f // block + np.arange(full + (1 if tail else 0)) * (s // block)
                assert idx.size == 0 or idx[-1] < tiles.size
                tiles[idx] += 1
                if tail:
                    assert idx[-1] == tiles.size - 1 and idx[-1] * block + tail == mk
            assert np.all(tiles == 1)
            assert mk % block == 0 or np.any(r["tail"][sel] == mk % block)
        end = g["off"] + HEAD_BYTES + (g["grid"] * 32 + 127) // 128 * 128
    assert nbytes == end
    if rows_seen:
        rows = np.concatenate(rows_seen)
        assert len(np.unique(rows)) == len(rows)


# sizeof(SweepDesc) rounded up to a multiple of 128 (sweep.h kSweepDescHead): 72 bytes of launch fields + 4 segment records of
# 112 bytes of pool streams, the size and four buffer pointers (152 bytes each); a block record is 32 bytes
HEAD_BYTES = (72 + 4 * 152 + 127) // 128 * 128


def test_the_cases_cover_what_can_go_wrong(desc):
    by_name = {c["name"]: c for c in CASES}
    fused = lambda name: [g for g in desc(by_name[name])[0] if g["multi"]]
    assert fused("config3")[0]["xcd_map"] and fused("config3")[0]["grid"] % 256 == 0
    assert fused("fused_65600")[0]["xcd_map"] and fused("fused_65600")[0]["grid"] == 256 and not fused("fused_1500")[0]["xcd_map"]
    cost = fused("fused_65600_cost")[0]        # (what tests/test_gpu_sweep_entry.py reads off the device context's segments)
    assert cost["xcd_map"] and cost["grid"] == 256 and 0 < cost["seg_w"][0] < 16 < cost["seg_w"][1]
    assert [g["nseg"] for g in fused("fused_3")] == [3] and [g["nseg"] for g in fused("fused_4")] == [4]
    assert len(fused("fused_ncoin_between")) == 2
    g, recs, _ = desc(by_name["single_2048"])
    assert g[0]["grid"] == 1 and recs[0, REC.index("full")] == 2 and recs[0, REC.index("tail")] == 0
    g, recs, _ = desc(by_name["single_140000"])
    assert g[0]["block"] == 1024 and g[0]["grid"] == 137 and recs[:, REC.index("full")].max() == 1
    g, recs, _ = desc(by_name["single_140000_tiles"])
    assert g[0]["block"] == 1024 and g[0]["grid"] == 32 and recs[:, REC.index("full")].min() == 4
    g, recs, _ = desc(by_name["product1m"])
    assert g[0]["block"] == 1024 and recs[:, REC.index("full")].min() >= 3
    # a grid larger than a segment's tiles leaves blocks with nothing to do: their records say so
    _, recs, _ = desc(by_name["fused_3"])
    idle = recs[(recs[:, REC.index("full")] == 0) & (recs[:, REC.index("tail")] == 0)]
    assert len(idle) > 0
