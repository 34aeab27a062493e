"""cfmm_find_path, the parts that need no device: the argument list across the header, the Python argtypes and the Julia ccall;
the router-level call on a recording context (1-based <-> 0-based tokens, the hop arrays turned back into (pools, tokens) on a
mixed market with a host-evaluated pool); the host reference of the layered search (tests/find_path_ref.py) against brute-force
enumeration on an exactly monotone quote function with built-in exact ties; and csrc/find_checks.h built for the host -- loaded
with ctypes, and as a stand-alone program under the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from find_path_ref import FOUND, FOUND_NONE, FOUND_REPEATS, brute_force_walks, find_path_ref, layers
from test_quote_cpu import RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "find_checks_host.cpp")


def test_header_python_and_julia_agree_on_the_arguments():
    raw = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    doc = raw[raw.index("The best swap path between two tokens"):raw.index("int cfmm_find_path(")]
    for phrase in ("The reference has no such function", "LAYERED", "FEWEST", "SMALLEST (segment, row, coin_in, coin_out)", "WALK",
                   "EVERY HOP IS QUOTED AGAINST THE POOL AS IT STANDS", "CFMM_FOUND_NONE", "CFMM_FOUND_REPEATS", "simple paths",
                   "CFMM_ERR_UNSUPPORTED", "256 MiB"):
        assert phrase in doc, phrase                                       # the contract is stated where the caller reads it
    for value, name in enumerate(("CFMM_FOUND", "CFMM_FOUND_NONE", "CFMM_FOUND_REPEATS")):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", raw), name
    assert (_lib.FOUND, _lib.FOUND_NONE, _lib.FOUND_REPEATS) == (0, 1, 2) == (cr.FOUND, cr.FOUND_NONE, cr.FOUND_REPEATS)
    assert (FOUND, FOUND_NONE, FOUND_REPEATS) == (0, 1, 2)
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    params = re.search(r"int\s+cfmm_find_path\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
    parts = [p.strip() for p in params.replace("\n", " ").split(",")]
    want_c = ["cfmm_ctx*", "int64_t", "int32_t", "int32_t*", "int32_t*", "double*", "double*", "int32_t*", "int32_t*", "int64_t*", "int32_t*",
              "int32_t*", "int32_t*"]
    want_py = ["_ctx", "C.c_int64", "C.c_int32", "_i32p", "_i32p", "_f64p", "_f64p", "_i32p", "_i32p", "_i64p", "_i32p", "_i32p", "_i32p"]
    want_jl = ["Ptr{Cvoid}", "Int64", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Int32}", "Ptr{Int32}",
               "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int32}"]
    assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == want_c
    assert [p.split()[-1] for p in parts] == ["ctx", "count", "max_hops", "token_in", "token_out", "amount_in", "amount_out", "n_hops", "hop_seg",
                                              "hop_row", "hop_coin_in", "hop_coin_out", "status"]
    assert [p.startswith("const") for p in parts[3:]] == [True] * 3 + [False] * 7      # three inputs, seven outputs
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    argtypes = [a.strip() for a in re.search(r"L\.cfmm_find_path\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert argtypes == want_py
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_find_path,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == want_jl
    assert "function find_paths(" in jl and "find_paths" in re.search(r"^export (.*)$", jl, flags=re.M).group(1)
    assert "find_paths(" in open(os.path.join(ROOT, "julia", "test", "runtests.jl")).read()
    assert re.search(r"\bcfmm_find_path\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert hasattr(_lib.Context, "find_path") and "find_path" in cr.__all__ and callable(cr.find_path)
    for name in ("FOUND", "FOUND_NONE", "FOUND_REPEATS"):
        assert name in cr.__all__


def test_device_header_is_included_behind_every_other_one():
    hip = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "sweep_kernels.hip")).read()
    includes = re.findall(r'#include "([^"]+)"', hip)
    assert includes[-1] == "find_path_kernels.h"                            # new templates are emitted behind the existing kernels
    src = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "find_path_kernels.h")).read()
    assert '#include "find_dir_kernels.h"' in src                           # the kernels' text, part of the search header
    src += open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "find_dir_kernels.h")).read()
    assert "atomicMax" in src and "atomicMin" in src and "__ballot" in src and "atomicAdd" not in src
    # the one dispatch on a kind lives in kind_switch.h: no query header spells the cases out again
    csrc = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")
    for header in ("query_read.h", "quote_kernels.h", "quote_path_kernels.h", "swap_kernels.h", "swap_out_kernels.h", "swap_path_kernels.h",
                   "find_path_kernels.h", "find_dir_kernels.h", "size_path_kernels.h"):
        assert "case CFMM_KIND_" not in open(os.path.join(csrc, header)).read(), header
    assert open(os.path.join(csrc, "kind_switch.h")).read().count("case CFMM_KIND_") == 6
    assert "kFindScratchBudget = 256ll << 20" in open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "find_checks.h")).read()


# ---- the router-level call on a recording context ---------------------------------------------------------------------------
class RecordingFindContext(RecordingContext):
    """answers every query with a fixed two-hop path through device pools, and records what it was sent"""

    def find_path(self, token_in, token_out, amount_in, max_hops=3):
        self.calls.append((np.array(token_in), np.array(token_out), np.array(amount_in), max_hops))
        n = len(self.calls[-1][2])
        seg, ci, co = (np.full((n, max_hops), -1, dtype=np.int32) for _ in range(3))
        row = np.full((n, max_hops), -1, dtype=np.int64)
        n_hops, status = np.zeros(n, dtype=np.int32), np.full(n, FOUND_NONE, dtype=np.int32)
        out = np.zeros(n)
        for q, (hops, st) in enumerate(self.answers[:n]):
            n_hops[q], status[q], out[q] = len(hops), st, (100.0 + q if hops else 0.0)
            for k, hop in enumerate(hops):
                seg[q, k], row[q, k], ci[q, k], co[q, k] = hop
        return out, n_hops, seg, row, ci, co, status


def test_router_maps_tokens_and_turns_hops_back_into_pools_and_tokens():
    # mixed_router: 0 product {1,2}, 1 geomean {2,3}, 2 host {1,3}, 3 product {3,4}, 4 weighted {1,2,4}, 5 product {1,4}
    r, pools = mixed_router()
    L, ctx = r._layout, r._backend.ctx
    ctx.__class__ = RecordingFindContext
    where = {i: (L.seg_of[L.locate(i)[1]], L.locate(i)[2]) for i in (0, 1, 3, 4, 5)}
    hop = lambda i, t_in, t_out: (*where[i], list(pools[i].Ai).index(t_in), list(pools[i].Ai).index(t_out))
    ctx.answers = [([hop(0, 1, 2), hop(1, 2, 3), hop(3, 3, 4)], FOUND),     # 1 -> 2 -> 3 -> 4
                   ([hop(4, 4, 2)], FOUND),                                 # the weighted pool: coin 2 in, coin 1 out
                   ([], FOUND_NONE),
                   ([hop(5, 4, 1), hop(4, 1, 4), hop(5, 4, 1)], FOUND_REPEATS)]
    out, pl, tk, status = cr.find_path(r, [1, 4, 3, 4], [4, 2, 3, 1], [1.0, 2.0, 3.0, 4.0], max_hops=3)
    assert len(ctx.calls) == 1
    tin, tout, amt, H = ctx.calls[0]
    assert tin.tolist() == [0, 3, 2, 3] and tout.tolist() == [3, 1, 2, 0] and amt.tolist() == [1.0, 2.0, 3.0, 4.0] and H == 3   # 0-based
    assert pl == [[0, 1, 3], [4], [], [5, 4, 5]]                           # positions in r.cfmms, the host pool's slot skipped
    assert tk == [[1, 2, 3, 4], [4, 2], [], [4, 1, 4, 1]]                  # 1-based, one more than the pools
    assert out.tolist() == [100.0, 101.0, 0.0, 103.0] and status.tolist() == [FOUND, FOUND, FOUND_NONE, FOUND_REPEATS]
    # what comes back is what quote_path takes
    from test_quote_path_cpu import RecordingPathContext
    ctx.__class__ = RecordingPathContext
    ctx.calls.clear()
    cr.quote_path(r, pl[:2], tk[:2], [1.0, 2.0])
    _, n_hops, seg, row, ci, co, _, _ = ctx.calls[0]
    assert n_hops.tolist() == [3, 1] and (seg[1, 0], row[1, 0], ci[1, 0], co[1, 0]) == hop(4, 4, 2)
    # scalars broadcast; the refusals come before the context is touched
    ctx.__class__ = RecordingFindContext
    ctx.calls.clear()
    cr.find_path(r, 1, [2, 3], 5.0)
    assert ctx.calls[0][0].tolist() == [0, 0] and ctx.calls[0][1].tolist() == [1, 2] and ctx.calls[0][2].tolist() == [5.0, 5.0] and ctx.calls[0][3] == 3
    ctx.calls.clear()
    for bad_in, bad_out, match in ((0, 1, "query 0: token_in 0 out of range 1:4"), ([1, 5], 1, "query 1: token_in 5"), (1, [1, 2, 9], "query 2: token_out 9")):
        with pytest.raises(cr.ArgumentError, match=match):
            cr.find_path(r, bad_in, bad_out, 1.0)
    with pytest.raises(cr.ArgumentError, match="one entry per query"):
        cr.find_path(r, [1, 2], [1, 2, 3], 1.0)
    assert ctx.calls == []
    assert "not searched" in cr.find_path.__doc__.replace("NOT", "not")


# ---- the reference against brute force, on integers ---------------------------------------------------------------------------
def integer_market():
    """three segments of 2-, 2- and 3-coin pools on 5 tokens; a quote is floor(amount * num / den) with small integer num, den per
    (pool, coin pair): non-decreasing in the amount and exact in doubles.  Segment 1's rows 0 and 1 are twins of segment 0's
    rows 0 and 1, and segment 0's row 4 is a twin of its row 0: exact ties by construction."""
    rng = np.random.default_rng(5)
    tok = [np.array([[0, 1], [1, 2], [2, 3], [3, 4], [0, 1], [4, 0]]),
           np.array([[0, 1], [1, 2], [0, 2], [1, 3]]),
           np.array([[0, 1, 2], [2, 3, 4], [4, 0, 2]])]
    rate = []
    for T in tok:
        m, nc = T.shape
        rate.append((rng.integers(5, 14, size=(m, nc, nc)), rng.integers(6, 12, size=(m, nc, nc))))
    for a, b in (((0, 4), (0, 0)), ((1, 0), (0, 0)), ((1, 1), (0, 1))):    # (segment, row) <- a copy of (segment, row)
        for part in (0, 1):
            rate[a[0]][part][a[1]] = rate[b[0]][part][b[1]]

    def quote(seg, amounts, ci, co, rows):
        num, den = rate[seg]
        rows, ci, co = np.asarray(rows), np.asarray(ci), np.asarray(co)
        return np.floor(np.asarray(amounts) * num[rows, ci, co] / den[rows, ci, co])
    return tok, quote


def every_walk(tok, quote, source, amount, max_hops):
    """every walk of 1 .. max_hops hops from `source`: (hops, the token each hop reaches, the amount leaving each hop)"""
    edges = {}
    for s, T in enumerate(tok):
        for row in range(T.shape[0]):
            for i in range(T.shape[1]):
                for j in range(T.shape[1]):
                    if i != j:
                        edges.setdefault(int(T[row, i]), []).append(((s, row, i, j), int(T[row, j])))
    out, frontier = [], [((), (), (), source, amount)]
    for _ in range(max_hops):
        nxt = []
        for hops, toks, vals, t, y in frontier:
            for e, to in edges.get(t, ()):
                z = float(quote(e[0], [y], [e[2]], [e[3]], [e[1]])[0]) if y > 0 else 0.0
                nxt.append((hops + (e,), toks + (to,), vals + (z,), to, z))
        out += nxt
        frontier = nxt
    return [(h, t, v) for h, t, v, _, _ in out]


def test_reference_equals_brute_force_on_an_exactly_monotone_market():
    tok, quote = integer_market()
    n, H = 5, 3
    sources = [(a, amt) for a in range(n) for amt in (1000.0, 7.0)]
    queries = [(a, b, amt) for a, amt in sources for b in range(n)] + [(0, 1, 0.0), (0, 1, 1.0)]
    walks = {src: every_walk(tok, quote, src[0], src[1], H) for src in set((a, x) for a, _, x in queries)}
    assert walks == {src: [(tuple(w), t, v) for w, t, v in every_walk(tok, quote, src[0], src[1], H)] for src in walks}
    assert {tuple(map(tuple, w)) for w in brute_force_walks(tok, 0, 3, H)} == {h for h, t, _ in walks[(0, 1000.0)] if t[-1] == 3}
    tin, tout, amt = (np.array(x) for x in zip(*queries))
    best = layers(tok, quote, n, tin, amt, H)
    ties = repeats = 0
    for max_hops in (1, 2, 3):
        out, n_hops, seg, row, ci, co, status = find_path_ref(tok, quote, n, tin, tout, amt, max_hops, best=best)
        direct = find_path_ref(tok, quote, n, tin, tout, amt, max_hops)   # layers computed for exactly max_hops: the same
        for x, y in zip(direct, (out, n_hops, seg, row, ci, co, status)):
            np.testing.assert_array_equal(x, y)
        for q, (a, b, x) in enumerate(queries):
            mine = [w for w in walks[(a, x)] if len(w[0]) <= max_hops]
            layer = {}                                                     # (hops, token) -> the best amount of any walk
            for _, toks, vals in mine:
                layer[(len(toks), toks[-1])] = max(layer.get((len(toks), toks[-1]), 0.0), vals[-1])
            top = max((vals[-1] for _, toks, vals in mine if toks[-1] == b), default=0.0)
            assert out[q] == top, (max_hops, q)                            # exactly monotone: the layered maximum IS the maximum
            if top <= 0:
                assert status[q] == FOUND_NONE and n_hops[q] == 0 and np.all(seg[q] == -1) and np.all(row[q] == -1)
                continue
            # the contract's path: the fewest hops; then, walking back from the end, the smallest hop among the walks that
            # attain the layer's best at every hop and whose later hops are the ones already chosen
            fewest = min(len(toks) for _, toks, vals in mine if toks[-1] == b and vals[-1] == top)
            cands = [hops for hops, toks, vals in mine if len(toks) == fewest and toks[-1] == b and
                     all(vals[k] == layer[(k + 1, toks[k])] for k in range(fewest))]
            ties += len(cands) > 1
            for k in reversed(range(fewest)):
                pick = min(w[k] for w in cands)
                cands = [w for w in cands if w[k] == pick]
            got = [(seg[q, k], row[q, k], ci[q, k], co[q, k]) for k in range(n_hops[q])]
            assert got == list(cands[0]), (max_hops, q)
            assert np.all(seg[q, n_hops[q]:] == -1)
            pools_on_it = [(s, r_) for s, r_, _, _ in got]
            assert status[q] == (FOUND_REPEATS if len(set(pools_on_it)) < len(pools_on_it) else FOUND)
            repeats += status[q] == FOUND_REPEATS
    print(f"integer market: {ties} answers with exact ties, {repeats} walks that re-enter a pool")
    assert ties > 5 and repeats > 0                                        # the built-in twins do tie


# ---- csrc/find_checks.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("find_checks_host") / "find_checks_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    lib.find_checks_host.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ip, ip, dp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
    lib.find_checks_host_chunk.argtypes = [ctypes.c_int64, ctypes.c_int32]
    lib.find_checks_host_chunk.restype = ctypes.c_int64
    return lib


def test_find_checks_header_needs_no_hip():
    src = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "find_checks.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert includes and not any("hip" in i or i in ("ctx.h", "sweep.h", "devbuf.h", "hostres.h") for i in includes), includes


def test_find_checks_case_list(host):
    assert host.find_checks_host_cases() == 0


def test_find_checks_every_refusal_text(host):
    n_tokens, count = 10, 5
    tin = np.array([0, 1, 2, 3, 9], dtype=np.int32)
    tout = np.array([9, 0, 2, 1, 4], dtype=np.int32)
    amt = np.array([0.0, 1.0, 2.0, 3.0, 4.0])

    def check(tin=tin, tout=tout, amt=amt, max_hops=3, count=count, outputs=1):
        msg = ctypes.create_string_buffer(256)
        p = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(t))
        rc = host.find_checks_host(n_tokens, count, max_hops, p(tin, ctypes.c_int32), p(tout, ctypes.c_int32), p(amt, ctypes.c_double),
                                   outputs, msg, 256)
        return rc, msg.value.decode()

    def edit(a, q, value):
        a = a.copy()
        a[q] = value
        return a
    assert check() == (0, "") and check(max_hops=1) == (0, "") and check(max_hops=8) == (0, "")
    assert check(count=-1) == (-1, "cfmm_find_path: count must be >= 0")
    assert check(max_hops=0) == (-1, "cfmm_find_path: max_hops must be 1 .. 8 (got 0)")
    assert check(max_hops=9) == (-1, "cfmm_find_path: max_hops must be 1 .. 8 (got 9)")
    assert check(outputs=0) == (-1, "cfmm_find_path: null query array")
    assert check(count=0, outputs=0) == (0, "")
    assert check(tin=edit(tin, 3, 10)) == (-1, "cfmm_find_path: query 3: token_in 10 out of range (the market has 10 tokens)")
    assert check(tin=edit(tin, 0, -1)) == (-1, "cfmm_find_path: query 0: token_in -1 out of range (the market has 10 tokens)")
    assert check(tout=edit(tout, 4, 10)) == (-1, "cfmm_find_path: query 4: token_out 10 out of range (the market has 10 tokens)")
    assert check(tout=edit(tout, 1, -7)) == (-1, "cfmm_find_path: query 1: token_out -7 out of range (the market has 10 tokens)")
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert check(amt=edit(amt, 2, bad)) == (-1, "cfmm_find_path: query 2: amount_in must be finite and >= 0")
    assert check(tin=edit(tin, 4, 10), amt=edit(amt, 1, -1.0))[1].startswith("cfmm_find_path: query 1: amount_in")   # the first bad query
    # the chunking rule
    assert host.find_checks_host_chunk(65536, 8) == 56 and host.find_checks_host_chunk(65536, 3) == 128
    assert host.find_checks_host_chunk(1 << 30, 8) == 1


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with -fsanitize=address,undefined, run as a program on the same case list.
    (The only sanitizer run of the feature; nothing loaded into Python is sanitized.)"""
    exe = str(tmp_path / "find_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DFIND_CHECKS_HOST_MAIN", SHIM, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "FIND_CHECKS_HOST_OK" in r.stdout and r.stderr == ""
