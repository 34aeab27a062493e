"""cfmm_swap_path, the parts that need no device: the argument list across the header, the Python argtypes and the Julia ccall;
the CFMM_PATH_* values; swap_path_ on a recording context -- quote_path's mapping of (pools, tokens) to the hop arrays, its
refusals (which come before the context is touched), the refreshed host mirror and the reset trades; and
csrc/swap_path_waves.h + csrc/swap_path_checks.h built for the host -- loaded with ctypes, and as a stand-alone program under
the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from test_quote_path_cpu import PATHS
from test_swap_cpu import RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "swap_path_host.cpp")
CSRC = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")


def test_header_python_and_julia_agree_on_the_arguments():
    raw = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    for value, name in enumerate(("CFMM_PATH_APPLIED", "CFMM_PATH_BELOW_LIMIT", "CFMM_PATH_REFUSED")):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", raw), name
    assert (_lib.PATH_APPLIED, _lib.PATH_BELOW_LIMIT, _lib.PATH_REFUSED) == (0, 1, 2)
    sweep_h = open(os.path.join(CSRC, "sweep.h")).read()
    assert re.search(r"kPathApplied = 0, kPathBelowLimit = 1, kPathRefused = 2", sweep_h)        # the kernel's spelling of the same
    assert "A POOL MAY APPEAR ONLY ONCE IN A PATH" in raw and "ALL OR NOTHING" in raw and "NO cfmm_swap_path_dev" in raw
    assert "no state advances between hops" in raw                      # cfmm_quote_path keeps its own wording
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert "cfmm_swap_path_dev" not in h and "cfmm_swap_path_out" not in h
    params = re.search(r"int\s+cfmm_swap_path\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
    parts = [p.strip() for p in params.replace("\n", " ").split(",")]
    assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == [
        "cfmm_ctx*", "int64_t", "int32_t", "int32_t*", "int32_t*", "int64_t*", "int32_t*", "int32_t*", "double*", "double*", "double*", "double*",
        "int32_t*"]
    assert [p.split()[-1] for p in parts][1:] == ["count", "max_hops", "n_hops", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out", "amount_in",
                                                 "min_amount_out", "amount_out", "hop_out", "status"]
    assert [p.startswith("const") for p in parts[3:]] == [True] * 7 + [False] * 3       # seven inputs, three outputs
    # the path arguments are exactly cfmm_quote_path's
    qp = re.search(r"int\s+cfmm_quote_path\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
    assert [p.strip() for p in qp.replace("\n", " ").split(",")][:9] == parts[:9]
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    argtypes = [a.strip() for a in re.search(r"L\.cfmm_swap_path\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert argtypes == ["_ctx", "C.c_int64", "C.c_int32", "_i32p", "_i32p", "_i64p", "_i32p", "_i32p", "_f64p", "_f64p", "_f64p", "_f64p", "_i32p"]
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_swap_path,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == ["Ptr{Cvoid}", "Int64", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int64}", "Ptr{Int32}",
                                                    "Ptr{Int32}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Int32}"]
    assert "function swap_paths!(" in jl and "swap_paths!" in re.search(r"^export (.*)$", jl, flags=re.M).group(1)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "cfmm_swap_path" in open(os.path.join(ROOT, doc)).read(), doc
    assert hasattr(_lib.Context, "swap_path") and not hasattr(_lib.Context, "swap_path_dev")
    assert "swap_path_" in cr.__all__
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("abi_swap_path.cpp", "swap_path_kernels.h", "swap_path_waves.h", "swap_path_checks.h"):
        assert f in mk, f


# ---- swap_path_ on a recording context ----------------------------------------------------------------------------------------
class RecordingPathContext(RecordingContext):
    """answers every path with 1000·(segment of its last hop) + the amount given, status = path number % 3, and records the
    arrays it was sent; the state it serves to the host mirror counts the visits each row has had"""

    def swap_path(self, n_hops, seg, row, ci, co, amount_in, min_out=None, hops=False):
        self.calls.append(("swap_path", np.array(n_hops), np.array(seg), np.array(row), np.array(ci), np.array(co), np.array(amount_in),
                           None if min_out is None else np.array(min_out), hops))
        for p, nh in enumerate(n_hops):
            for k in range(nh):
                key = (int(seg[p, k]), int(row[p, k]))
                self.swapped[key] = self.swapped.get(key, 0) + 1
        last = np.array(seg)[np.arange(len(n_hops)), np.array(n_hops) - 1]
        out = 1000.0 * last + np.asarray(amount_in)
        st = (np.arange(len(n_hops)) % 3).astype(np.int32)
        return (out, st, np.full((np.shape(seg)[1], len(n_hops)), 7.0)) if hops else (out, st)

    def swap(self, *a, **k):
        raise AssertionError("a path call went to the single-pool entry")

    def quote_path(self, *a, **k):
        raise AssertionError("an execution went to the read-only entry")


def path_router():
    r, pools = mixed_router()
    r._backend.ctx.__class__ = RecordingPathContext
    return r, pools


def test_router_builds_the_hop_arrays_and_refreshes_the_mirror():
    r, pools = path_router()
    L, ctx = r._layout, r._backend.ctx
    cr.find_arb_(r, np.ones(4))
    assert r._trades_stale
    amt = np.array([1.0, 2.0, 3.0, 4.0])
    out, st = cr.swap_path_(r, [p for p, _ in PATHS], [t for _, t in PATHS], amt, min_out=[0.5, 0.0, 1.0, 2.0])
    assert len(ctx.calls) == 1                                     # ONE call for all paths, whatever segments they touch
    verb, n_hops, seg, row, ci, co, a, lim, hops = ctx.calls[0]
    assert verb == "swap_path" and hops is False
    assert n_hops.tolist() == [3, 1, 4, 2] and n_hops.dtype == np.int32
    assert seg.shape == row.shape == ci.shape == co.shape == (4, 4)
    assert seg.dtype == ci.dtype == co.dtype == np.int32 and row.dtype == np.int64
    np.testing.assert_array_equal(a, amt)
    assert lim.dtype == np.float64 and lim.tolist() == [0.5, 0.0, 1.0, 2.0]
    for p, (pl, tk) in enumerate(PATHS):                           # quote_path's mapping
        for k, i in enumerate(pl):
            _, b, want_row = L.locate(i)
            Ai = list(pools[i].Ai)
            assert (seg[p, k], row[p, k], ci[p, k], co[p, k]) == (L.seg_of[b], want_row, Ai.index(tk[k]), Ai.index(tk[k + 1])), (p, k)
    assert st.tolist() == [0, 1, 2, 0] and st.dtype == np.int32
    for p, (pl, _) in enumerate(PATHS):
        assert out[p] == 1000.0 * L.seg_of[L.locate(pl[-1])[1]] + amt[p]
    # the host mirror of the touched rows follows the device: pool 0 is visited once, pool 3 three times, pool 5 twice
    assert pools[0].R[0] == 101.0 and pools[3].R[0] == 103.0 and pools[5].R[0] == 102.0 and pools[4].R[0] == 102.0
    assert not r._trades_stale and all(np.all(np.asarray(x) == 0) for x in r.Δs)       # the old trades are gone
    # no limit, a scalar limit, hops=True, sync_host=False
    ctx.calls.clear()
    res = cr.swap_path_(r, [[0]], [[2, 1]], 2.5, hops=True, sync_host=False)
    assert len(res) == 3 and res[2].shape == (1, 1) and ctx.calls[0][7] is None and ctx.calls[0][8] is True
    assert (ctx.calls[0][4][0, 0], ctx.calls[0][5][0, 0]) == (1, 0) and pools[0].R[0] == 101.0   # (the mirror was not refreshed)
    cr.swap_path_(r, [[0], [5]], [[2, 1], [1, 4]], [1.0, 2.0], min_out=0.25, sync_host=False)
    assert ctx.calls[1][7].tolist() == [0.25, 0.25]


def test_router_refuses_before_the_context_is_touched():
    r, _ = path_router()

    def refused(match, pools, tokens, amount=1.0, **kw):
        with pytest.raises(cr.ArgumentError, match=match):
            cr.swap_path_(r, pools, tokens, amount, **kw)
        assert r._backend.ctx.calls == []

    good = ([0, 1], [1, 2, 3])
    refused(r"path 1, hop 1: token 4 is not a coin of pool 1", [good[0], [0, 1]], [good[1], [1, 2, 4]])
    refused(r"path 1, hop 0: token 2 on both sides of pool 0", [good[0], [0]], [good[1], [2, 2]])
    refused(r"path 0, hop 2: pool 0 appears twice", [[0, 5, 0]], [[2, 1, 4, 1]])
    refused(r"path 1, hop 1: pool 2: FixedTrade is evaluated on the host", [good[0], [0, 2]], [good[1], [2, 1, 3]])
    refused(r"path 0: 9 pools \(a path has 1 to 8\)", [[0, 1, 3, 5, 4, 0, 1, 3, 5]], [[1] * 10])
    refused(r"path 0: 0 pools", [[]], [[1]])
    refused(r"pool 6 out of range", [[6]], [[1, 2]])
    refused(r"amount_in must be a scalar or have one entry per path", [[0], [0]], [[1, 2], [2, 1]], amount=[1.0, 2.0, 3.0])
    refused(r"min_out must be a scalar or have one entry per path", [[0], [5]], [[1, 2], [1, 4]], min_out=[1.0, 2.0, 3.0])


def test_context_wrapper_checks_shapes_before_the_library():
    ctx = object.__new__(cr.Context)
    ctx._h = None
    z = np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(cr.ArgumentError, match="n_hops"):
        ctx.swap_path([1], z, z, z, z, [1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="hop_row"):
        ctx.swap_path([1, 1], z, np.zeros((2, 2)), z, z, [1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="min_out"):
        ctx.swap_path([1, 1], z, z, z, z, [1.0, 2.0], min_out=[1.0, 2.0, 3.0])


# ---- the wave numbering and the checks on the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the two headers built for the host (they need no HIP header), loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("swap_path_host") / "swap_path_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip, lp, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    lib.swap_path_host_waves.argtypes = [ctypes.c_int64, ip, ip, lp, lp]
    lib.swap_path_host_waves.restype = ctypes.c_int64
    lib.swap_path_host_plan.argtypes = [ctypes.c_int64, ip, ip, lp, lp, lp]
    lib.swap_path_host_plan.restype = ctypes.c_int64
    lib.swap_path_host_check.argtypes = [ctypes.c_int64, ip, ip, lp, dp, ctypes.c_char_p, ctypes.c_int64]
    return lib


def test_headers_need_no_hip():
    for name in ("swap_path_waves.h", "swap_path_checks.h"):
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(os.path.join(CSRC, name)).read())
        assert includes and not any("hip" in i or i in ("ctx.h", "sweep.h", "devbuf.h", "hostres.h") for i in includes), (name, includes)


def hop_arrays(paths):
    """paths as lists of (segment, row) -> n_hops, and hop-major [H, count] segment / row arrays (garbage in the unused slots)"""
    count, H = len(paths), max([len(p) for p in paths] + [1])
    n_hops = np.array([len(p) for p in paths], dtype=np.int32)
    seg, row = np.full((H, count), -5, dtype=np.int32), np.full((H, count), 1 << 40, dtype=np.int64)
    for p, path in enumerate(paths):
        for k, (s, r) in enumerate(path):
            seg[k, p], row[k, p] = s, r
    return n_hops, seg, row


def p_(a, t):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(t))


def waves_of(host, paths):
    n_hops, seg, row = hop_arrays(paths)
    wave = np.full(len(paths), -1, dtype=np.int64)
    n = host.swap_path_host_waves(len(paths), p_(n_hops, ctypes.c_int32), p_(seg, ctypes.c_int32), p_(row, ctypes.c_int64), p_(wave, ctypes.c_int64))
    perm, off = np.full(len(paths), -1, dtype=np.int64), np.full(len(paths) + 1, -1, dtype=np.int64)
    assert host.swap_path_host_plan(len(paths), p_(n_hops, ctypes.c_int32), p_(seg, ctypes.c_int32), p_(row, ctypes.c_int64),
                                    p_(perm, ctypes.c_int64), p_(off, ctypes.c_int64)) == n
    return wave, int(n), perm, off[:n + 1]


def test_case_list(host):
    assert host.swap_path_host_cases() == 0


def test_the_worked_case(host):
    A, B, C, D = (0, 5), (1, 5), (1, 6), (2, 0)
    wave, n, perm, off = waves_of(host, [[A, B], [B, C], [D], [C, A]])
    assert wave.tolist() == [0, 1, 0, 2] and n == 3
    assert perm.tolist() == [0, 2, 1, 3] and off.tolist() == [0, 2, 3, 4]     # wave after wave, query order inside a wave


@pytest.mark.parametrize("rows,count", [(4, 60), (32, 300), (None, 300)])
def test_wave_properties_on_random_batches(host, rows, count):
    """paths of 1..8 distinct pools drawn over 3 segments of `rows` rows, so that most paths conflict; rows None: every hop of
    the batch gets a row of its own (pool-disjoint paths)"""
    rng = np.random.default_rng(count + (rows or 0))
    paths, fresh = [], iter(rng.permutation(8 * count).tolist())
    for _ in range(count):
        nh = int(rng.integers(1, 9))
        pools = set()
        while len(pools) < (nh if rows is None else min(nh, 3 * rows)):
            pools.add((int(rng.integers(0, 3)), next(fresh) if rows is None else int(rng.integers(0, rows))))
        paths.append(sorted(pools, key=lambda _: rng.random()))
    wave, n, perm, off = waves_of(host, paths)
    assert n == wave.max() + 1 and sorted(perm.tolist()) == list(range(count))
    # every wave is pool-disjoint
    for w in range(n):
        members = perm[off[w]:off[w + 1]]
        assert np.all(wave[members] == w) and np.all(np.diff(members) > 0)        # ... and in query order
        named = [pool for p in members for pool in paths[p]]
        assert len(named) == len(set(named)), w
    # for every pool the paths naming it have strictly increasing waves in query order; and the numbering is minimal: each
    # path sits in the smallest wave that is behind the previous path of each of its pools
    last = {}
    for p, path in enumerate(paths):
        need = max([last[pool] + 1 for pool in path if pool in last] + [0])
        assert wave[p] == need, p
        for pool in path:
            last[pool] = int(wave[p])
    if rows is None:
        assert n == 1 and perm.tolist() == list(range(count))             # pool-disjoint: one wave, in query order
    else:
        assert n > 1


def test_refusals_name_path_and_hops(host):
    def check(paths, lim=None):
        n_hops, seg, row = hop_arrays(paths)
        msg = ctypes.create_string_buffer(256)
        rc = host.swap_path_host_check(len(paths), p_(n_hops, ctypes.c_int32), p_(seg, ctypes.c_int32), p_(row, ctypes.c_int64),
                                       None if lim is None else p_(np.asarray(lim, dtype=np.float64), ctypes.c_double), msg, 256)
        return rc, msg.value.decode()

    A, B, C = (0, 1), (1, 1), (1, 2)
    good = [[A, B], [B, C, A], [C]]
    assert check(good) == (0, "") and check(good, [0.0, 1.0, 1e308]) == (0, "")
    assert check([[A, B], [B, C, B]]) == (-1, "cfmm_swap_path: path 1, hops 0 and 2: row 1 of segment 1 appears twice (a pool may appear only once in a path)")
    assert check([[A, A]])[1].startswith("cfmm_swap_path: path 0, hops 0 and 1: row 1 of segment 0")
    assert check(good, [0.0, -1.0, 0.0]) == (-1, "cfmm_swap_path: path 1, hop 2: min_amount_out must be finite and >= 0")
    assert check(good, [np.nan, 0.0, 0.0]) == (-1, "cfmm_swap_path: path 0, hop 1: min_amount_out must be finite and >= 0")
    assert check(good, [0.0, 0.0, np.inf])[1].startswith("cfmm_swap_path: path 2, hop 0: min_amount_out")


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with -fsanitize=address,undefined, run as a program on the same case list.
    (The only sanitizer run of the feature; nothing loaded into Python is sanitized.)"""
    exe = str(tmp_path / "swap_path_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSWAP_PATH_HOST_MAIN", SHIM, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "SWAP_PATH_HOST_OK" in r.stdout and r.stderr == ""
