"""cfmm_quote_path / cfmm_quote_path_out and their _dev forms, the parts that need no device: the argument lists across the
header, the Python argtypes and the Julia ccall; the router's mapping of (pools, tokens) to the hop arrays on a mixed market
with a host-evaluated pool, on a recording context; the router's refusals, which come before the context is touched; and
csrc/path_checks.h built for the host -- loaded with ctypes, and as a stand-alone program under the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from test_quote_cpu import RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "path_checks_host.cpp")
ENTRIES = ("cfmm_quote_path", "cfmm_quote_path_out", "cfmm_quote_path_dev", "cfmm_quote_path_out_dev")


def test_header_python_and_julia_agree_on_the_arguments():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    assert re.search(r"#define\s+CFMM_MAX_PATH_HOPS\s+8\b", h) and _lib.MAX_PATH_HOPS == 8
    assert "no state advances between hops" in h                       # the limit is stated where the caller reads it
    h = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    want_c = ["cfmm_ctx*", "int64_t", "int32_t", "int32_t*", "int32_t*", "int64_t*", "int32_t*", "int32_t*", "double*", "double*", "double*"]
    want_py = ["_ctx", "C.c_int64", "C.c_int32", "_i32p", "_i32p", "_i64p", "_i32p", "_i32p", "_f64p", "_f64p", "_f64p"]
    want_jl = ["Ptr{Cvoid}", "Int64", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Float64}",
               "Ptr{Float64}", "Ptr{Float64}"]
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    names = {}
    for entry in ENTRIES:
        params = re.search(r"int\s+" + entry + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
        parts = [p.strip() for p in params.replace("\n", " ").split(",")]
        assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == want_c, entry
        names[entry] = [p.split()[-1] for p in parts]
        # the eight inputs are const, the three outputs are not
        assert [p.startswith("const") for p in parts[3:]] == [True] * 6 + [False] * 2, entry
        argtypes = [a.strip() for a in re.search(r"L\." + entry + r"\.argtypes = \[(.*?)\]", py).group(1).split(",")]
        assert argtypes == (want_py if not entry.endswith("_dev") else want_py[:3] + ["C.c_void_p"] * 8), entry
    assert names["cfmm_quote_path"][3:] == ["n_hops", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out", "amount_in", "amount_out", "hop_out"]
    assert names["cfmm_quote_path_out"][3:] == ["n_hops", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out", "amount_out", "amount_in", "hop_in"]
    assert names["cfmm_quote_path_dev"][3:] == ["d_" + n for n in names["cfmm_quote_path"][3:]]
    assert names["cfmm_quote_path_out_dev"][3:] == ["d_" + n for n in names["cfmm_quote_path_out"][3:]]
    for entry in ENTRIES[:2]:
        call = re.search(r"ccall\(\(:" + entry + r",\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
        assert [a.strip() for a in call.split(",")] == want_jl, entry
    assert "function quote_paths(" in jl and "function quote_paths_out(" in jl
    exported = re.search(r"^export (.*)$", jl, flags=re.M).group(1)
    assert "quote_paths" in exported.replace("quote_paths_out", "") and "quote_paths_out" in exported
    tests = open(os.path.join(ROOT, "julia", "test", "runtests.jl")).read()
    assert "quote_paths(" in tests and "quote_paths_out(" in tests
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry in ENTRIES:
        assert re.search(r"\b" + entry + r"\b", integration), entry
    for name in ("quote_path", "quote_path_out", "quote_path_dev", "quote_path_out_dev"):
        assert hasattr(_lib.Context, name), name
    assert "quote_path" in cr.__all__ and "quote_path_out" in cr.__all__


# ---- the router-level calls on a recording context --------------------------------------------------------------------------
class RecordingPathContext(RecordingContext):
    """answers every path with 1000·(segment of its last hop) + the amount given, and records the arrays it was sent"""

    def _record(self, verb, n_hops, seg, row, ci, co, amount, hops):
        self.calls.append((verb, np.array(n_hops), np.array(seg), np.array(row), np.array(ci), np.array(co), np.array(amount), hops))
        last = np.array(seg)[np.arange(len(n_hops)), np.array(n_hops) - 1]
        out = 1000.0 * last + np.asarray(amount)
        return (out, np.full((np.shape(seg)[1], len(n_hops)), 7.0)) if hops else out

    def quote_path(self, n_hops, seg, row, ci, co, amount_in, hops=False):
        return self._record("quote_path", n_hops, seg, row, ci, co, amount_in, hops)

    def quote_path_out(self, n_hops, seg, row, ci, co, amount_out, hops=False):
        return self._record("quote_path_out", n_hops, seg, row, ci, co, amount_out, hops)

    def quote(self, *a, **k):
        raise AssertionError("a path call went to the single-pool entry")


def path_router():
    r, pools = mixed_router()
    r._backend.ctx.__class__ = RecordingPathContext
    return r, pools


# mixed_router: 0 product {1,2}, 1 geomean {2,3}, 2 host {1,3}, 3 product {3,4}, 4 weighted {1,2,4}, 5 product {1,4}
PATHS = [([0, 1, 3], [1, 2, 3, 4]),          # 1 -> 2 -> 3 -> 4
         ([4], [4, 2]),                      # the weighted pool: coin 2 in, coin 1 out
         ([5, 4, 1, 3], [4, 1, 2, 3, 4]),    # four hops, a cycle in tokens
         ([3, 5], [3, 4, 1])]


@pytest.mark.parametrize("verb", ("quote_path", "quote_path_out"))
def test_router_builds_the_hop_arrays(verb):
    r, pools = path_router()
    L, ctx = r._layout, r._backend.ctx
    amt = np.array([1.0, 2.0, 3.0, 4.0])
    out = getattr(cr, verb)(r, [p for p, _ in PATHS], [t for _, t in PATHS], amt)
    assert len(ctx.calls) == 1                                     # ONE call for all paths, whatever segments they touch
    got_verb, n_hops, seg, row, ci, co, a, hops = ctx.calls[0]
    assert got_verb == verb and hops is False
    assert n_hops.tolist() == [3, 1, 4, 2] and n_hops.dtype == np.int32
    assert seg.shape == row.shape == ci.shape == co.shape == (4, 4)  # [count, max_hops], max_hops = the longest path
    assert seg.dtype == ci.dtype == co.dtype == np.int32 and row.dtype == np.int64
    np.testing.assert_array_equal(a, amt)
    for p, (pl, tk) in enumerate(PATHS):
        for k, i in enumerate(pl):
            _, b, want_row = L.locate(i)
            Ai = list(pools[i].Ai)
            assert (seg[p, k], row[p, k], ci[p, k], co[p, k]) == (L.seg_of[b], want_row, Ai.index(tk[k]), Ai.index(tk[k + 1])), (p, k)
    # the weighted pool's coins are positions among its three
    assert (ci[1, 0], co[1, 0]) == (2, 1)
    # the answers come back in the caller's order
    for p, (pl, _) in enumerate(PATHS):
        assert out[p] == 1000.0 * L.seg_of[L.locate(pl[-1])[1]] + amt[p]
    # hops=True is passed on and the hop amounts come back with the answers; a scalar amount serves every path
    ctx.calls.clear()
    out2, hv = getattr(cr, verb)(r, [[0]], [[2, 1]], 2.5, hops=True)
    assert ctx.calls[0][7] is True and hv.shape == (1, 1) and out2.shape == (1,)
    assert ctx.calls[0][6].tolist() == [2.5] and (ctx.calls[0][4][0, 0], ctx.calls[0][5][0, 0]) == (1, 0)


@pytest.mark.parametrize("verb", ("quote_path", "quote_path_out"))
def test_router_refuses_before_the_context_is_touched(verb):
    r, _ = path_router()
    call = getattr(cr, verb)

    def refused(match, pools, tokens, amount=1.0):
        with pytest.raises(cr.ArgumentError, match=match):
            call(r, pools, tokens, amount)
        assert r._backend.ctx.calls == []

    good = ([0, 1], [1, 2, 3])
    refused(r"path 1, hop 1: token 4 is not a coin of pool 1", [good[0], [0, 1]], [good[1], [1, 2, 4]])
    refused(r"path 0, hop 0: token 3 is not a coin of pool 0", [[0]], [[3, 1]])
    refused(r"path 1, hop 0: token 2 on both sides of pool 0", [good[0], [0]], [good[1], [2, 2]])
    refused(r"path 0, hop 2: pool 0 appears twice", [[0, 5, 0]], [[2, 1, 4, 1]])
    refused(r"path 1, hop 1: pool 2: FixedTrade is evaluated on the host", [good[0], [0, 2]], [good[1], [2, 1, 3]])
    refused(r"path 0: 9 pools \(a path has 1 to 8\)", [[0, 1, 3, 5, 4, 0, 1, 3, 5]], [[1] * 10])
    refused(r"path 0: 0 pools", [[]], [[1]])
    refused(r"path 0: 2 tokens for 2 pools", [[0, 1]], [[1, 2]])
    refused(r"pool 6 out of range", [[6]], [[1, 2]])
    refused(r"one sequence per path", [[0]], [[1, 2], [2, 1]])
    refused(r"one entry per path", [[0], [0]], [[1, 2], [2, 1]], amount=[1.0, 2.0, 3.0])


class NoContextBackend:
    """a backend that evaluates but holds no device context"""

    def __init__(self, n):
        self.n = n

    def eval(self, v):
        return np.zeros(self.n), 0.0

    find_arb = eval


def test_a_backend_without_a_context_is_not_implemented():
    _, pools = mixed_router()
    r = cr.Router(cr.LinearNonnegative(np.ones(4)), pools, 4, _backend=NoContextBackend(4))
    with pytest.raises(NotImplementedError, match="no device context"):
        cr.quote_path(r, [[0]], [[1, 2]], 1.0)
    with pytest.raises(NotImplementedError, match="no device context"):
        cr.quote_path_out(r, [[0]], [[1, 2]], 1.0)
    with pytest.raises(cr.ArgumentError, match="token 3"):              # ... but the arguments are judged first
        cr.quote_path(r, [[0]], [[1, 3]], 1.0)


def test_context_wrapper_checks_shapes_before_the_library():
    ctx = object.__new__(cr.Context)
    ctx._h = None
    z = np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(cr.ArgumentError, match="n_hops"):
        ctx.quote_path([1], z, z, z, z, [1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="hop_row"):
        ctx.quote_path([1, 1], z, np.zeros((2, 2)), z, z, [1.0, 2.0])
    with pytest.raises(cr.ArgumentError, match="hop_coin_out"):
        ctx.quote_path_out([1, 1], z, z, z, np.zeros((3, 3)), [1.0, 2.0])
    # count == 0 returns empty without the library
    e = np.zeros((0, 3), dtype=np.int32)
    assert ctx.quote_path([], e, e, e, e, []).size == 0
    out, hv = ctx.quote_path_out([], e, e, e, e, [], hops=True)
    assert out.size == 0 and hv.shape == (3, 0)


# ---- csrc/path_checks.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """path_checks.h built for the host (it needs no HIP header), loaded with ctypes"""
    so = str(tmp_path_factory.mktemp("path_checks_host") / "path_checks_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip, lp, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    lib.path_checks_host.argtypes = [ctypes.c_int64, ip, lp, ip, ctypes.c_int, ctypes.c_int64, ctypes.c_int32, ip, ip, lp, ip, ip, dp,
                                     ctypes.c_char_p, ctypes.c_int64]
    return lib


def test_path_checks_header_needs_no_hip():
    src = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "path_checks.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert includes and not any("hip" in i or i in ("ctx.h", "sweep.h", "devbuf.h", "hostres.h") for i in includes), includes


def test_path_checks_case_list(host):
    assert host.path_checks_host_cases() == 0


def test_path_checks_name_path_and_hop(host):
    """the same function driven from here: a market of two segments, the hop-major layout as the ABI passes it"""
    kind, m, nc = np.array([0, 4], dtype=np.int32), np.array([10, 6], dtype=np.int64), np.array([2, 3], dtype=np.int32)
    count, H = 5, 3
    n_hops = np.array([1, 2, 3, 2, 1], dtype=np.int32)
    seg = np.zeros((H, count), dtype=np.int32)
    seg[1] = 1
    row = np.tile(np.arange(count, dtype=np.int64), (H, 1))
    ci = np.zeros((H, count), dtype=np.int32)
    co = np.ones((H, count), dtype=np.int32)
    co[1] = 2
    amt = np.ones(count)

    def check(exact_out=0, seg=seg, row=row, ci=ci, co=co, amt=amt, n_hops=n_hops):
        msg = ctypes.create_string_buffer(256)
        p = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(t))
        rc = host.path_checks_host(2, p(kind, ctypes.c_int32), p(m, ctypes.c_int64), p(nc, ctypes.c_int32), exact_out, count, H,
                                   p(n_hops, ctypes.c_int32), p(seg, ctypes.c_int32), p(row, ctypes.c_int64), p(ci, ctypes.c_int32),
                                   p(co, ctypes.c_int32), p(amt, ctypes.c_double), msg, 256)
        return rc, msg.value.decode()

    assert check() == (0, "") and check(1) == (0, "")

    def edit(a, k, p, value):
        a = a.copy()
        a[k, p] = value
        return a
    assert check(row=edit(row, 1, 2, 6)) == (-1, "cfmm_quote_path: path 2, hop 1: row 6 out of range (segment 1 has 6 pools)")
    assert check(1, row=edit(row, 1, 2, 6))[1].startswith("cfmm_quote_path_out: path 2, hop 1: row 6")
    assert check(row=edit(row, 2, 0, 99)) == (0, "")                   # hop 2 of path 0 is not a hop: ignored
    assert check(seg=edit(seg, 0, 4, 2)) == (-1, "cfmm_quote_path: path 4, hop 0: segment 2 out of range (the context has 2)")
    assert check(ci=edit(ci, 2, 2, 2)) == (-1, "cfmm_quote_path: path 2, hop 2: coin_in 2 out of range (pool has 2 coins)")
    assert check(co=edit(co, 1, 3, 3)) == (-1, "cfmm_quote_path: path 3, hop 1: coin_out 3 out of range (pool has 3 coins)")
    assert check(co=edit(co, 1, 1, 0)) == (-1, "cfmm_quote_path: path 1, hop 1: coin_in and coin_out are both 0")
    bad = amt.copy()
    bad[2] = np.nan
    assert check(amt=bad) == (-1, "cfmm_quote_path: path 2, hop 0: amount_in must be finite and >= 0")
    assert check(1, amt=bad) == (-1, "cfmm_quote_path_out: path 2, hop 2: amount_out must be finite and >= 0")
    nh = n_hops.copy()
    nh[3] = 4
    assert check(n_hops=nh) == (-1, "cfmm_quote_path: path 3: n_hops 4 out of range (1 .. 3)")


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with -fsanitize=address,undefined, run as a program on the same case list.
    (The only sanitizer run of the feature; nothing loaded into Python is sanitized.)"""
    exe = str(tmp_path / "path_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DPATH_CHECKS_HOST_MAIN", SHIM, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "PATH_CHECKS_HOST_OK" in r.stdout and r.stderr == ""
