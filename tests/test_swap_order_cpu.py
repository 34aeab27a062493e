"""cfmm_swap_order / cfmm_swap_order_out, the parts that need no device: the constants and the argument list across the header,
the kernel's spelling, the Python binding and the Julia file; swap_order_ on a recording context (the mapping of orders to
order_first and the hop arrays, the refusals before the context is touched, the refreshed host mirror); csrc/swap_order_waves.h
built for the host -- loaded with ctypes and held to a Python restatement of the planner's rule on random batches, and as a
stand-alone program under the sanitizers; and csrc/order_checks.h, every refusal with its text, as a stand-alone program under
the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from test_swap_cpu import RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "swap_order_host.cpp")
CSRC = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")
NAMES = ("ORDER_APPLIED", "ORDER_LIMIT", "ORDER_REFUSED", "ORDER_UNOBTAINABLE", "ORDER_PATH_HELD")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


# ---- the header, the kernel's spelling, the Python binding and the Julia file agree ------------------------------------------------
def test_header_python_and_julia_agree_on_constants_and_arguments():
    raw = read("include", "cfmm_amd_order.h")
    values = {name: int(re.search(r"#define\s+CFMM_" + name + r"\s+(\d+)\b", raw).group(1)) for name in NAMES}
    assert values == {"ORDER_APPLIED": 0, "ORDER_LIMIT": 1, "ORDER_REFUSED": 2, "ORDER_UNOBTAINABLE": 3, "ORDER_PATH_HELD": 4}
    base = read("include", "cfmm_amd.h")
    path_codes = {int(re.search(r"#define\s+" + n + r"\s+(\d+)\b", base).group(1)) for n in ("CFMM_PATH_APPLIED", "CFMM_PATH_REFUSED", "CFMM_SWAP_UNOBTAINABLE")}
    assert values["ORDER_PATH_HELD"] not in path_codes                     # path_status tells the four apart
    for name, v in values.items():
        assert getattr(_lib, name) == v and getattr(cr, name) == v and name in cr.__all__
    sweep_h = read("cfmmrouter.jl_amd", "csrc", "sweep.h")
    assert "kOrderApplied = 0, kOrderLimit = 1, kOrderRefused = 2, kOrderUnobtainable = 3" in sweep_h and "kOrderPathHeld = 4" in sweep_h
    jl = read("julia", "src", "swap_order.jl")
    for name, v in values.items():
        assert re.search(r"^const " + name + r" = Int32\(" + str(v) + r"\)", jl, flags=re.M), name
    for phrase in ("THE CONTRACT IS THE SERIAL EXECUTION", "refused > unobtainable > limit", "STILL HOLDS ITS POOLS FOR ITS WAVE", "Host pointers only",
                   "CFMM_ERR_UNSUPPORTED", "order_max_blocks", "OUT OF SCOPE", "share pool"):
        assert phrase in raw, phrase
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    want_c = ["cfmm_ctx*", "int64_t", "int64_t*", "int64_t", "int32_t", "int32_t*", "int32_t*", "int64_t*", "int32_t*", "int32_t*", "double*", "double*",
              "double*", "double*", "double*", "int32_t*", "int32_t*"]
    lists = {}
    for entry in ("cfmm_swap_order", "cfmm_swap_order_out"):
        params = re.search(r"int\s+" + entry + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
        parts = [p.strip() for p in params.replace("\n", " ").split(",")]
        assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == want_c, entry
        assert [p.startswith("const") for p in parts[2:]] == [True, False, False] + [True] * 7 + [False] * 5, entry
        lists[entry] = [p.split()[-1] for p in parts]
    assert lists["cfmm_swap_order"][1:] == ["count", "order_first", "n_paths", "max_hops", "n_hops", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out",
                                            "path_amount_in", "min_total_out", "path_amount_out", "hop_out", "total_out", "path_status", "status"]
    assert lists["cfmm_swap_order_out"][10:] == ["path_amount_out", "max_total_in", "path_amount_in", "hop_in", "total_in", "path_status", "status"]
    assert "cfmm_swap_order" not in base                                    # the addition lives in its own header
    py = read("cfmmrouter.jl_amd", "_lib.py")
    argtypes = [a.strip() for a in re.search(r"L\.cfmm_swap_order\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert argtypes == ["_ctx", "C.c_int64", "_i64p", "C.c_int64", "C.c_int32", "_i32p", "_i32p", "_i64p", "_i32p", "_i32p", "_f64p", "_f64p", "_f64p",
                        "_f64p", "_f64p", "_i32p", "_i32p"]
    assert "L.cfmm_swap_order_out.argtypes = L.cfmm_swap_order.argtypes" in py
    for name in ("swap_order", "swap_order_out"):
        assert hasattr(_lib.Context, name) and not hasattr(_lib.Context, name + "_dev")
    for name in ("swap_order_", "swap_order_out_", "route_order_", "route_order_out_"):
        assert name in cr.__all__ and hasattr(cr, name)
    mk = read("cfmmrouter.jl_amd", "csrc", "Makefile")
    for f in ("abi_swap_order.cpp", "swap_order_kernels.h", "swap_order_waves.h", "order_checks.h", "cfmm_amd_order.h"):
        assert f in mk, f
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "cfmm_swap_order" in read(doc) and "swap_order_" in read(doc), doc
    # what the split headers said was out of scope no longer is: they point at the new calls
    for header in ("cfmm_amd_split.h", "cfmm_amd_split_out.h"):
        text = read("include", header)
        assert "executing inside the same call" not in text and "cfmm_swap_order" in text, header


def test_the_kernels_sit_behind_every_other_kernel_and_launcher():
    chain_end = read("cfmmrouter.jl_amd", "csrc", "split_paths_out_kernels.h").rstrip().splitlines()[-1]
    assert chain_end == '#include "swap_order_kernels.h"'
    kernels = read("cfmmrouter.jl_amd", "csrc", "swap_order_kernels.h")
    assert "__shared__" not in kernels and "atomic" not in kernels.replace("no atomic", "") and "__syncthreads" not in kernels
    assert "hop_try<false>(a.p" in kernels and "hop_try<true>(a.p" in kernels and "apply_hop(a.p" in kernels   # the existing bodies, unchanged
    hip = read("cfmmrouter.jl_amd", "csrc", "sweep_kernels.hip")
    launchers = re.findall(r"^hipError_t (launch_\w+)\(", hip, flags=re.M)
    assert launchers[-1] == "launch_swap_order"


# ---- swap_order_ on a recording context ---------------------------------------------------------------------------------------------
class RecordingOrderContext(RecordingContext):
    """answers every path with 1000 + the amount given, every order with the sum, statuses by number % 3, and records what it
    was sent; the state it serves to the host mirror counts the visits each row has had"""

    def swap_order(self, first, n_hops, seg, row, ci, co, amount, limit=None, hops=False):
        self.calls.append(("swap_order", np.array(first), np.array(n_hops), np.array(seg), np.array(row), np.array(ci), np.array(co), np.array(amount),
                           None if limit is None else np.array(limit), hops))
        for p, nh in enumerate(n_hops):
            for k in range(nh):
                key = (int(seg[p, k]), int(row[p, k]))
                self.swapped[key] = self.swapped.get(key, 0) + 1
        out = 1000.0 + np.asarray(amount)
        g = len(first) - 1
        total = np.array([out[first[i]:first[i + 1]].sum() for i in range(g)])
        res = (out, total, (np.arange(g) % 3).astype(np.int32), (np.arange(len(n_hops)) % 3).astype(np.int32))
        return res + (np.full((np.shape(seg)[1], len(n_hops)), 7.0),) if hops else res

    swap_order_out = swap_order

    def swap_path(self, *a, **k):
        raise AssertionError("an order call went to the path entry")


def order_router():
    r, pools = mixed_router()
    r._backend.ctx.__class__ = RecordingOrderContext
    return r, pools


def two_disjoint_paths(r, pools):
    """two single-pool paths between the same two tokens over different device pools, found in the router's own market"""
    L = r._layout
    by_pair = {}
    for i, p in enumerate(pools):
        if L.locate(i)[0] == "host":
            continue
        Ai = list(p.Ai)
        for a in Ai:
            for b in Ai:
                if a != b:
                    by_pair.setdefault((a, b), []).append(i)
    for (a, b), idx in sorted(by_pair.items()):
        if len(idx) >= 2:
            return [[idx[0]], [idx[1]]], [[a, b], [a, b]]
    return None


def test_router_builds_order_first_and_the_hop_arrays_and_refuses_before_the_context():
    r, pools = order_router()
    ctx = r._backend.ctx
    single = [[[0]], [[5]]]
    tokens = [[[2, 1]], [[1, 4]]]
    out, total, st, pst = cr.swap_order_(r, single, tokens, [np.array([1.0]), np.array([2.0])], min_total_out=[0.5, 0.25])
    assert len(ctx.calls) == 1
    verb, first, n_hops, seg, row, ci, co, a, lim, hops = ctx.calls[0]
    assert verb == "swap_order" and first.tolist() == [0, 1, 2] and first.dtype == np.int64 and n_hops.tolist() == [1, 1] and hops is False
    assert a.tolist() == [1.0, 2.0] and lim.tolist() == [0.5, 0.25]
    assert [o.tolist() for o in out] == [[1001.0], [1002.0]] and total.tolist() == [1001.0, 1002.0] and st.tolist() == [0, 1]
    assert [p.tolist() for p in pst] == [[0], [1]]
    assert pools[0].R[0] == 101.0 and pools[5].R[0] == 101.0                    # the host mirror of the touched rows follows the device
    assert not r._trades_stale
    pair = two_disjoint_paths(r, pools)
    if pair is not None:
        ctx.calls.clear()
        res = cr.swap_order_out_(r, [pair[0]], [pair[1]], 3.0, max_total_in=9.0, hops=True, sync_host=False)
        assert len(res) == 5 and ctx.calls[0][1].tolist() == [0, 2] and ctx.calls[0][7].tolist() == [3.0, 3.0] and ctx.calls[0][8].tolist() == [9.0]
        assert [o.tolist() for o in res[0]] == [[1003.0, 1003.0]] and res[1].tolist() == [2006.0]
    ctx.calls.clear()

    def refused(match, pools_, tokens_, amount=1.0, **kw):
        with pytest.raises(cr.ArgumentError, match=match):
            cr.swap_order_(r, pools_, tokens_, amount, **kw)
        assert ctx.calls == []

    refused(r"order 0: paths 0 and 1 share pool 0", [[[0], [0]]], [[[2, 1], [2, 1]]])
    refused(r"order 0: its paths must all start at the same token and end at the same token", [[[0], [5]]], [[[2, 1], [1, 4]]])
    refused(r"order 1: 9 paths \(an order has 1 to 8\)", [[[0]], [[0]] * 9], [[[2, 1]], [[2, 1]] * 9])
    refused(r"order 0: 0 paths", [[]], [[]])
    refused(r"path 1, hop 0: token 3 is not a coin of pool 0", [[[5]], [[0]]], [[[1, 4]], [[3, 1]]])
    refused(r"tokens must have one list of paths per order", [[[0]]], [])
    refused(r"path_amount_in must be a scalar or have one entry per path", single, tokens, amount=[np.ones(1), np.ones(2)])
    refused(r"min_total_out must be a scalar or have one entry per order", single, tokens, min_total_out=[1.0, 2.0, 3.0])
    with pytest.raises(cr.ArgumentError, match="path_amount_out must be a scalar or have one entry per path"):
        cr.swap_order_out_(r, single, tokens, [np.ones(1)])
    with pytest.raises(cr.ArgumentError, match="max_total_in must be a scalar or have one entry per order"):
        cr.swap_order_out_(r, single, tokens, 1.0, max_total_in=[1.0, 2.0, 3.0])
    assert ctx.calls == []


def test_context_wrapper_checks_shapes_before_the_library():
    ctx = object.__new__(cr.Context)
    ctx._h = None
    z = np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(cr.ArgumentError, match="n_hops"):
        ctx.swap_order([0, 2], [1], z, z, z, z, [1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="hop_row"):
        ctx.swap_order([0, 2], [1, 1], z, np.zeros((2, 2)), z, z, [1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="min_total_out"):
        ctx.swap_order([0, 2], [1, 1], z, z, z, z, [1.0, 2.0], min_total_out=[1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="max_total_in"):
        ctx.swap_order_out([0, 1, 2], [1, 1], z, z, z, z, [1.0, 2.0], max_total_in=[1.0, 2.0, 3.0])


# ---- the planner on the host ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the header built for the host (it needs no HIP header), loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("swap_order_host") / "swap_order_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip, lp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.swap_order_host_waves.argtypes = [ctypes.c_int64, lp, ctypes.c_int64, ip, ip, lp, lp]
    lib.swap_order_host_waves.restype = ctypes.c_int64
    lib.swap_order_host_plan.argtypes = [ctypes.c_int64, lp, ctypes.c_int64, ip, ip, lp, lp, lp]
    lib.swap_order_host_plan.restype = ctypes.c_int64
    lib.swap_order_host_path_plan.argtypes = [ctypes.c_int64, ip, ip, lp, lp, lp]
    lib.swap_order_host_path_plan.restype = ctypes.c_int64
    return lib


def test_headers_need_no_hip():
    for name in ("swap_order_waves.h", "order_checks.h"):
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', read("cfmmrouter.jl_amd", "csrc", name))
        assert includes and not any("hip" in i or i in ("ctx.h", "sweep.h", "devbuf.h", "hostres.h") for i in includes), (name, includes)


def p_(a, t):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(t))


def order_arrays(orders):
    """orders as lists of paths, paths as lists of (segment, row) -> order_first, n_hops and hop-major [H, n_paths] segment / row
    arrays (garbage in the unused slots)"""
    flat = [p for o in orders for p in o]
    first = np.concatenate(([0], np.cumsum([len(o) for o in orders]))).astype(np.int64)
    n, H = len(flat), max([len(p) for p in flat] + [1])
    n_hops = np.array([len(p) for p in flat], dtype=np.int32)
    seg, row = np.full((H, max(n, 1)), -5, dtype=np.int32), np.full((H, max(n, 1)), 1 << 40, dtype=np.int64)
    seg, row = seg[:, :n], row[:, :n]
    for q, path in enumerate(flat):
        for k, (s, r) in enumerate(path):
            seg[k, q], row[k, q] = s, r
    return first, n_hops, np.ascontiguousarray(seg), np.ascontiguousarray(row)


def plan_of(host, orders):
    first, n_hops, seg, row = order_arrays(orders)
    g, n = len(orders), int(first[-1])
    args = (g, p_(first, ctypes.c_int64), n, p_(n_hops, ctypes.c_int32), p_(seg, ctypes.c_int32), p_(row, ctypes.c_int64))
    wave = np.full(g, -1, dtype=np.int64)
    waves = host.swap_order_host_waves(*args, p_(wave, ctypes.c_int64))
    perm, off = np.full(g, -1, dtype=np.int64), np.full(g + 1, -1, dtype=np.int64)
    assert host.swap_order_host_plan(*args, p_(perm, ctypes.c_int64), p_(off, ctypes.c_int64)) == waves
    return wave, int(waves), perm, off[:waves + 1]


def test_case_list(host):
    assert host.swap_order_host_cases() == 0


def test_the_worked_case(host):
    A, B, C, D, E, F = (0, 5), (1, 5), (1, 6), (2, 0), (2, 1), (0, 6)
    wave, n, perm, off = plan_of(host, [[[A], [B]], [[C], [D, B]], [[E]], [[C, A], [F]]])
    assert wave.tolist() == [0, 1, 0, 2] and n == 3
    assert perm.tolist() == [0, 2, 1, 3] and off.tolist() == [0, 2, 3, 4]     # wave after wave, the caller's order inside a wave


def random_orders(rng, count, rows, max_k=8):
    """orders of 1 .. max_k paths of 1 .. 3 pools drawn over 3 segments of `rows` rows, no pool twice in an order; rows None:
    every hop of the batch gets a row of its own (pool-disjoint orders)"""
    orders, fresh = [], iter(rng.permutation(8 * 3 * count + 8).tolist())
    for _ in range(count):
        K = int(rng.integers(1, max_k + 1))
        taken, order = set(), []
        for _ in range(K):
            nh = int(rng.integers(1, 4))
            path = []
            while len(path) < nh and (rows is None or len(taken) < 3 * rows):
                pool = (int(rng.integers(0, 3)), next(fresh) if rows is None else int(rng.integers(0, rows)))
                if pool not in taken:
                    taken.add(pool)
                    path.append(pool)
            if path:
                order.append(path)
        orders.append(order)
    return orders


@pytest.mark.parametrize("rows,count", [(8, 60), (48, 300), (None, 300)])
def test_the_planners_four_properties_on_random_batches(host, rows, count):
    rng = np.random.default_rng(count + (rows or 0))
    orders = random_orders(rng, count, rows)
    wave, n, perm, off = plan_of(host, orders)
    pools_of = [[pool for path in o for pool in path] for o in orders]
    assert all(len(set(p)) == len(p) for p in pools_of)
    assert n == wave.max() + 1 and sorted(perm.tolist()) == list(range(count))
    # the restatement: an order's wave is the maximum of free_from over all pools of all its paths; afterwards each of those
    # pools is free from that wave + 1 -- whether or not the order will turn out to be applied
    free = {}
    for g, named in enumerate(pools_of):
        need = max([free.get(pool, 0) for pool in named] + [0])
        assert wave[g] == need, g                                          # (all paths of an order: one wave number)
        for pool in named:
            free[pool] = need + 1
    # inside a wave no two orders share a pool, and the wave is in the caller's order
    for w in range(n):
        members = perm[off[w]:off[w + 1]]
        assert np.all(wave[members] == w) and np.all(np.diff(members) > 0)
        named = [pool for g in members for pool in pools_of[g]]
        assert len(named) == len(set(named)), w
    if rows is None:
        assert n == 1 and perm.tolist() == list(range(count))             # pool-disjoint orders: one wave
    else:
        assert n > 1


def test_one_path_per_order_is_the_path_planner(host):
    rng = np.random.default_rng(11)
    orders = random_orders(rng, 200, 16, max_k=1)
    wave, n, perm, off = plan_of(host, orders)
    first, n_hops, seg, row = order_arrays(orders)
    count = len(orders)
    assert first.tolist() == list(range(count + 1))
    p_perm, p_off = np.full(count, -1, dtype=np.int64), np.full(count + 1, -1, dtype=np.int64)
    waves = host.swap_order_host_path_plan(count, p_(n_hops, ctypes.c_int32), p_(seg, ctypes.c_int32), p_(row, ctypes.c_int64),
                                           p_(p_perm, ctypes.c_int64), p_(p_off, ctypes.c_int64))
    assert waves == n > 1 and p_perm.tolist() == perm.tolist() and p_off[:waves + 1].tolist() == off.tolist()


def test_stand_alone_planner_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with -fsanitize=address,undefined, run as a program on the same case list.
    (Nothing loaded into Python is sanitized.)"""
    exe = str(tmp_path / "swap_order_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSWAP_ORDER_HOST_MAIN", SHIM, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "SWAP_ORDER_HOST_OK" in r.stdout and r.stderr == ""


def test_every_refusal_of_the_checks_header_with_its_text(tmp_path):
    """tests/native/order_checks_host.cpp: compiled without HIP, under the sanitizers, run as a program"""
    exe = str(tmp_path / "order_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "native", "order_checks_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "ORDER_CHECKS_OK" in r.stdout and r.stderr == ""
