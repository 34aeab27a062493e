"""cfmm_find_path_out, the parts that need no device: the argument list across its header, the Python argtypes and the Julia
ccall; the contract's key phrases in the header; the router-level call on a recording context; the host reference of the
layered min-search (tests/find_path_out_ref.py) against brute-force enumeration of every walk on an exactly monotone integer
market with built-in twins; and csrc/find_checks.h as the entry calls it -- loaded with ctypes, and as a stand-alone program under
the sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from find_path_out_ref import FOUND, FOUND_NONE, FOUND_REPEATS, find_path_out_ref, layers_out
from test_find_path_cpu import integer_market
from test_quote_cpu import RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "find_out_checks_host.cpp")


def read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_header_python_and_julia_agree_on_the_arguments():
    raw = read("include", "cfmm_amd_find_out.h")
    assert '#include "cfmm_amd.h"' in raw and "cfmm_find_path_out" not in read("include", "cfmm_amd.h")
    doc = raw[raw.index("The cheapest swap path that BUYS an exact amount"):raw.index("int cfmm_find_path_out(")]
    for phrase in ("LAYERED", "FEWEST", "SMALLEST (segment, row, coin_in, coin_out)", "forward walk", "+inf", "+0.0", "MINIMUM", "WALK",
                   "EVERY HOP IS QUOTED AGAINST THE POOL AS IT", "CFMM_FOUND_NONE", "CFMM_FOUND_REPEATS", "CFMM_ERR_UNSUPPORTED",
                   "cfmm_quote_path_out on the returned arrays answers amount_in bit for bit", "path order", "256 MiB"):
        assert phrase in doc, phrase                                       # the contract is stated where the caller reads it
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    params = re.search(r"int\s+cfmm_find_path_out\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
    parts = [p.strip() for p in params.replace("\n", " ").split(",")]
    want_c = ["cfmm_ctx*", "int64_t", "int32_t", "int32_t*", "int32_t*", "double*", "double*", "int32_t*", "int32_t*", "int64_t*", "int32_t*",
              "int32_t*", "int32_t*"]
    want_py = ["_ctx", "C.c_int64", "C.c_int32", "_i32p", "_i32p", "_f64p", "_f64p", "_i32p", "_i32p", "_i64p", "_i32p", "_i32p", "_i32p"]
    want_jl = ["Ptr{Cvoid}", "Int64", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Int32}", "Ptr{Int32}",
               "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int32}"]
    assert len(parts) == 13
    assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == want_c
    assert [p.split()[-1] for p in parts] == ["ctx", "count", "max_hops", "token_in", "token_out", "amount_out", "amount_in", "n_hops", "hop_seg",
                                              "hop_row", "hop_coin_in", "hop_coin_out", "status"]      # cfmm_find_path's, the amounts exchanged
    assert [p.startswith("const") for p in parts[3:]] == [True] * 3 + [False] * 7      # three inputs, seven outputs
    # the same types, position by position, as cfmm_find_path
    h0 = re.sub(r"/\*.*?\*/", " ", read("include", "cfmm_amd.h"), flags=re.S)
    parts0 = [p.strip() for p in re.search(r"int\s+cfmm_find_path\s*\(([^;]*?)\)\s*;", h0, flags=re.S).group(1).replace("\n", " ").split(",")]
    assert [p.rsplit(None, 1)[0] for p in parts] == [p.rsplit(None, 1)[0] for p in parts0]
    py = read("cfmmrouter.jl_amd", "_lib.py")
    argtypes = [a.strip() for a in re.search(r"L\.cfmm_find_path_out\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert argtypes == want_py
    jl = read("julia", "src", "find_paths_out.jl")
    call = re.search(r"ccall\(\(:cfmm_find_path_out,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == want_jl
    module = read("julia", "src", "CFMMRouterAMD.jl")
    assert 'include("find_paths_out.jl")' in module and ":cfmm_find_path_out" not in module   # the ccall lives in the verb's own file
    assert "function find_paths_out(" in jl and "find_paths_out" in re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(",")
    assert "token_in[q] - 1" in jl and "token_out[q] - 1" in jl and "segment_rows(r)" in jl and "co[q, k] + 1" in jl
    tests = read("julia", "test", "runtests.jl")
    assert "find_paths_out(" in tests and "quote_paths_out(r, paths[found]" in tests and "swap_paths_out!(" in tests
    assert re.search(r"\bcfmm_find_path_out\b", read("INTEGRATION.md")) and "find_path_out" in read("README.md")
    assert "cfmm_find_path_out" in read("DESIGN.md")
    assert hasattr(_lib.Context, "find_path_out") and "find_path_out" in cr.__all__ and callable(cr.find_path_out)


def test_device_code_sits_below_the_existing_kernels_and_has_no_float_atomic():
    hip = read("cfmmrouter.jl_amd", "csrc", "sweep_kernels.hip")
    assert re.findall(r'#include "([^"]+)"', hip)[-1] == "find_path_kernels.h"
    src = read("cfmmrouter.jl_amd", "csrc", "find_path_kernels.h")
    launch = hip[hip.index("hipError_t launch_find("):hip.index("hipError_t launch_size_path(")]
    # both directions are ONE search: every entry keeps its name and template arguments, is defined in the header and is
    # what launch_find launches
    kernels = read("cfmmrouter.jl_amd", "csrc", "find_dir_kernels.h")     # the six kernels' one text, included once per direction
    assert src.count('#include "find_dir_kernels.h"') == 2
    for prefix, out in (("find_", "false"), ("find_out_", "true")):
        assert f'#define CFMM_FIND_OUT {out}\n#define CFMM_FIND(role) {prefix}##role\n#include "find_dir_kernels.h"' in src
    for role in ("init", "relax", "select", "claim", "advance", "finish"):
        args = "template <int BLOCK, bool LDS>" if role == "relax" else "template <int BLOCK>"
        assert kernels.count(f"{args}\n__global__ __launch_bounds__(BLOCK) void CFMM_FIND({role})(FindArgs a)") == 1, role
        for prefix in ("find_", "find_out_"):
            assert f"&{prefix}{role}<kFindBlock" in launch, prefix + role
    assert kernels.count("\n__global__ ") == 6
    src += kernels
    # the search reuses the quotes and the one kind dispatch, and copies neither: no kind is named here
    for reused in ("find_segment<true>", "find_tokens(", "find_decode(", "find_clamp_token(", "with_kind(", "path_hop<decltype(K)::value, OUT>"):
        assert reused in src, reused
    assert "CFMM_KIND_" not in src and "switch (" not in src
    assert src.count("__ballot(") == 1                                     # one relax text, one early-out
    # both integer folds, and no float atomic in any query header
    assert "atomicMax(word, bits)" in src and "atomicMin(word, bits)" in src
    for header in ("kind_switch.h", "query_read.h", "quote_kernels.h", "quote_path_kernels.h", "swap_kernels.h", "swap_out_kernels.h",
                   "swap_path_kernels.h", "find_path_kernels.h", "find_dir_kernels.h", "size_path_kernels.h", "swap_pool.h"):
        assert "atomicAdd" not in read("cfmmrouter.jl_amd", "csrc", header), header
    assert "template <bool TILE>" in src


# ---- the router-level call on a recording context ---------------------------------------------------------------------------
class RecordingFindOutContext(RecordingContext):
    """answers every query with a fixed path through device pools, and records what it was sent"""

    def find_path_out(self, token_in, token_out, amount_out, max_hops=3):
        self.calls.append((np.array(token_in), np.array(token_out), np.array(amount_out), max_hops))
        n = len(self.calls[-1][2])
        seg, ci, co = (np.full((n, max_hops), -1, dtype=np.int32) for _ in range(3))
        row = np.full((n, max_hops), -1, dtype=np.int64)
        n_hops, status = np.zeros(n, dtype=np.int32), np.full(n, FOUND_NONE, dtype=np.int32)
        cost = np.full(n, np.inf)
        for q, (hops, st) in enumerate(self.answers[:n]):
            n_hops[q], status[q], cost[q] = len(hops), st, (100.0 + q if hops else np.inf)
            for k, hop in enumerate(hops):
                seg[q, k], row[q, k], ci[q, k], co[q, k] = hop
        return cost, n_hops, seg, row, ci, co, status

    def find_path(self, *a, **k):
        raise AssertionError("an exact-output search went to the exact-input entry")


def test_router_maps_tokens_and_turns_hops_back_into_pools_and_tokens():
    # mixed_router: 0 product {1,2}, 1 geomean {2,3}, 2 host {1,3}, 3 product {3,4}, 4 weighted {1,2,4}, 5 product {1,4}
    r, pools = mixed_router()
    L, ctx = r._layout, r._backend.ctx
    ctx.__class__ = RecordingFindOutContext
    where = {i: (L.seg_of[L.locate(i)[1]], L.locate(i)[2]) for i in (0, 1, 3, 4, 5)}
    hop = lambda i, t_in, t_out: (*where[i], list(pools[i].Ai).index(t_in), list(pools[i].Ai).index(t_out))
    ctx.answers = [([hop(0, 1, 2), hop(1, 2, 3), hop(3, 3, 4)], FOUND),     # 1 -> 2 -> 3 -> 4, in path order
                   ([hop(4, 4, 2)], FOUND),                                 # the weighted pool: coin 2 in, coin 1 out
                   ([], FOUND_NONE),
                   ([hop(5, 4, 1), hop(4, 1, 4), hop(5, 4, 1)], FOUND_REPEATS)]
    cost, pl, tk, status = cr.find_path_out(r, [1, 4, 3, 4], [4, 2, 3, 1], [1.0, 2.0, 3.0, 4.0], max_hops=3)
    assert len(ctx.calls) == 1
    tin, tout, amt, H = ctx.calls[0]
    assert tin.tolist() == [0, 3, 2, 3] and tout.tolist() == [3, 1, 2, 0] and amt.tolist() == [1.0, 2.0, 3.0, 4.0] and H == 3   # 0-based
    assert pl == [[0, 1, 3], [4], [], [5, 4, 5]]                           # positions in r.cfmms, the host pool's slot skipped
    assert tk == [[1, 2, 3, 4], [4, 2], [], [4, 1, 4, 1]]                  # 1-based, one more than the pools
    assert cost.tolist() == [100.0, 101.0, np.inf, 103.0] and status.tolist() == [FOUND, FOUND, FOUND_NONE, FOUND_REPEATS]
    # what comes back is what quote_path_out takes
    from test_quote_path_cpu import RecordingPathContext
    ctx.__class__ = RecordingPathContext
    ctx.calls.clear()
    cr.quote_path_out(r, pl[:2], tk[:2], [1.0, 2.0])
    verb, n_hops, seg, row, ci, co, _, _ = ctx.calls[0]
    assert verb == "quote_path_out" and n_hops.tolist() == [3, 1] and (seg[1, 0], row[1, 0], ci[1, 0], co[1, 0]) == hop(4, 4, 2)
    assert (seg[0, 0], row[0, 0], ci[0, 0], co[0, 0]) == hop(0, 1, 2) and (seg[0, 2], row[0, 2], ci[0, 2], co[0, 2]) == hop(3, 3, 4)
    # scalars broadcast; the refusals come before the context is touched
    ctx.__class__ = RecordingFindOutContext
    ctx.calls.clear()
    cr.find_path_out(r, 1, [2, 3], 5.0)
    assert ctx.calls[0][0].tolist() == [0, 0] and ctx.calls[0][1].tolist() == [1, 2] and ctx.calls[0][2].tolist() == [5.0, 5.0] and ctx.calls[0][3] == 3
    ctx.calls.clear()
    for bad_in, bad_out, match in ((0, 1, "query 0: token_in 0 out of range 1:4"), ([1, 5], 1, "query 1: token_in 5"), (1, [1, 2, 9], "query 2: token_out 9")):
        with pytest.raises(cr.ArgumentError, match=match):
            cr.find_path_out(r, bad_in, bad_out, 1.0)
    with pytest.raises(cr.ArgumentError, match="token_in, token_out and amount_out must be scalars or have one entry per query"):
        cr.find_path_out(r, [1, 2], [1, 2, 3], 1.0)
    assert ctx.calls == []
    assert "not searched" in cr.find_path_out.__doc__.replace("NOT", "not")


# ---- the reference against brute force, on integers ---------------------------------------------------------------------------
def integer_market_out():
    """test_find_path_cpu.integer_market() -- three segments of 2-, 2- and 3-coin pools on 5 tokens, quote = floor(x * num / den)
    with small integer num, den per (pool, coin pair), segment 1's rows 0 and 1 twins of segment 0's rows 0 and 1 and segment 0's
    row 4 a twin of its row 0 -- with the EXACT INVERSE of that quote: quote_out(y) = ceil(y * den / num), the smallest integer
    x with quote(x) >= y.  Non-decreasing in y and exact in doubles.  The rates are drawn the way integer_market draws them; that
    they are the same ones is asserted against its quote."""
    tok, quote = integer_market()
    rng = np.random.default_rng(5)
    rate = []
    for T in tok:
        m, nc = T.shape
        rate.append((rng.integers(5, 14, size=(m, nc, nc)), rng.integers(6, 12, size=(m, nc, nc))))
    for a, b in (((0, 4), (0, 0)), ((1, 0), (0, 0)), ((1, 1), (0, 1))):
        for part in (0, 1):
            rate[a[0]][part][a[1]] = rate[b[0]][part][b[1]]

    def quote_out(seg, amounts, ci, co, rows):
        num, den = rate[seg]
        rows, ci, co = np.asarray(rows), np.asarray(ci), np.asarray(co)
        y = np.asarray(amounts, dtype=np.float64).astype(np.int64)
        assert np.all(y == np.asarray(amounts))                            # integers in, integers out
        return (-((-y * den[rows, ci, co]) // num[rows, ci, co])).astype(np.float64)

    for s, T in enumerate(tok):                                            # the exact inverse, on every edge
        for row in range(T.shape[0]):
            for i in range(T.shape[1]):
                for j in range(T.shape[1]):
                    if i != j:
                        y = np.array([1.0, 7.0, 1000.0, 123457.0])
                        x = quote_out(s, y, [i] * 4, [j] * 4, [row] * 4)
                        assert np.all(quote(s, x, [i] * 4, [j] * 4, [row] * 4) >= y) and np.all(quote(s, x - 1, [i] * 4, [j] * 4, [row] * 4) < y)
    return tok, quote_out


def every_walk_into(tok, quote_out, dest, amount, max_hops):
    """every walk of 1 .. max_hops hops that ENDS at `dest`: (hops in path order, the token each hop STARTS from, the amount to
    tender to each hop), grown from the last hop backwards"""
    edges = {}
    for s, T in enumerate(tok):
        for row in range(T.shape[0]):
            for i in range(T.shape[1]):
                for j in range(T.shape[1]):
                    if i != j:
                        edges.setdefault(int(T[row, j]), []).append(((s, row, i, j), int(T[row, i])))
    out, frontier = [], [((), (), (), dest, amount)]
    for _ in range(max_hops):
        nxt = []
        for hops, toks, vals, t, y in frontier:
            for e, frm in edges.get(t, ()):
                z = float(quote_out(e[0], [y], [e[2]], [e[3]], [e[1]])[0]) if y > 0 else 0.0
                nxt.append(((e,) + hops, (frm,) + toks, (z,) + vals, frm, z))
        out += nxt
        frontier = nxt
    return [(h, t, v) for h, t, v, _, _ in out]


def test_reference_equals_brute_force_on_an_exactly_monotone_market():
    tok, quote_out = integer_market_out()
    n, H = 5, 3
    dests = [(b, amt) for b in range(n) for amt in (1000.0, 7.0)]
    queries = [(a, b, amt) for b, amt in dests for a in range(n)] + [(0, 1, 0.0), (0, 1, 1.0)]
    walks = {d: every_walk_into(tok, quote_out, d[0], d[1], H) for d in set((b, y) for _, b, y in queries)}
    tin, tout, amt = (np.array(x) for x in zip(*queries))
    need = layers_out(tok, quote_out, n, tout, amt, H)
    ties = repeats = 0
    for max_hops in (1, 2, 3):
        cost, n_hops, seg, row, ci, co, status = find_path_out_ref(tok, quote_out, n, tin, tout, amt, max_hops, need=need)
        direct = find_path_out_ref(tok, quote_out, n, tin, tout, amt, max_hops)   # layers computed for exactly max_hops: the same
        for x, y in zip(direct, (cost, n_hops, seg, row, ci, co, status)):
            np.testing.assert_array_equal(x, y)
        for q, (a, b, y) in enumerate(queries):
            mine = [w for w in walks[(b, y)] if len(w[0]) <= max_hops and w[2][0] > 0]
            layer = {}                                                     # (hops still to go, token) -> the cheapest of any walk
            for _, toks, vals in mine:
                layer[(len(toks), toks[0])] = min(layer.get((len(toks), toks[0]), np.inf), vals[0])
            low = min((vals[0] for _, toks, vals in mine if toks[0] == a), default=np.inf)
            if y == 0:
                assert not mine and cost[q] == 0.0 and not np.signbit(cost[q]) and status[q] == FOUND_NONE and n_hops[q] == 0
                continue
            assert cost[q] == low, (max_hops, q)                           # exactly monotone: the layered minimum IS the minimum
            if not np.isfinite(low):
                assert status[q] == FOUND_NONE and n_hops[q] == 0 and np.all(seg[q] == -1) and np.all(row[q] == -1)
                continue
            # the contract's path: the fewest hops; then, walking forward from the start, the smallest hop among the walks whose
            # every suffix attains its layer's cheapest and whose earlier hops are the ones already chosen
            fewest = min(len(toks) for _, toks, vals in mine if toks[0] == a and vals[0] == low)
            cands = [hops for hops, toks, vals in mine if len(toks) == fewest and toks[0] == a and
                     all(vals[k] == layer[(fewest - k, toks[k])] for k in range(fewest))]
            ties += len(cands) > 1
            for k in range(fewest):
                pick = min(w[k] for w in cands)
                cands = [w for w in cands if w[k] == pick]
            got = [(seg[q, k], row[q, k], ci[q, k], co[q, k]) for k in range(n_hops[q])]
            assert got == list(cands[0]), (max_hops, q)
            assert np.all(seg[q, n_hops[q]:] == -1)
            assert tok[got[0][0]][got[0][1], got[0][2]] == a and tok[got[-1][0]][got[-1][1], got[-1][3]] == b
            pools_on_it = [(s, r_) for s, r_, _, _ in got]
            assert status[q] == (FOUND_REPEATS if len(set(pools_on_it)) < len(pools_on_it) else FOUND)
            repeats += status[q] == FOUND_REPEATS
    print(f"integer market: {ties} answers with exact ties, {repeats} walks that re-enter a pool")
    assert ties > 5 and repeats > 0                                        # the built-in twins do tie; some cheapest walk re-enters a pool


# ---- csrc/find_checks.h as cfmm_find_path_out calls it --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("find_out_checks_host") / "find_out_checks_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    lib.find_out_checks_host.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ip, ip, dp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
    return lib


def test_find_checks_case_list(host):
    assert host.find_out_checks_host_cases() == 0


def test_find_checks_every_refusal_text(host):
    n_tokens, count = 10, 5
    tin = np.array([0, 1, 2, 3, 9], dtype=np.int32)
    tout = np.array([9, 0, 2, 1, 4], dtype=np.int32)
    amt = np.array([0.0, 1.0, 2.0, 3.0, 4.0])

    def check(tin=tin, tout=tout, amt=amt, max_hops=3, count=count, outputs=1):
        msg = ctypes.create_string_buffer(256)
        p = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(t))
        rc = host.find_out_checks_host(n_tokens, count, max_hops, p(tin, ctypes.c_int32), p(tout, ctypes.c_int32), p(amt, ctypes.c_double),
                                       outputs, msg, 256)
        return rc, msg.value.decode()

    def edit(a, q, value):
        a = a.copy()
        a[q] = value
        return a
    assert check() == (0, "") and check(max_hops=1) == (0, "") and check(max_hops=8) == (0, "")
    assert check(count=-1) == (-1, "cfmm_find_path_out: count must be >= 0")
    assert check(max_hops=0) == (-1, "cfmm_find_path_out: max_hops must be 1 .. 8 (got 0)")
    assert check(max_hops=9) == (-1, "cfmm_find_path_out: max_hops must be 1 .. 8 (got 9)")
    assert check(outputs=0) == (-1, "cfmm_find_path_out: null query array")
    assert check(count=0, outputs=0) == (0, "")
    assert check(tin=edit(tin, 3, 10)) == (-1, "cfmm_find_path_out: query 3: token_in 10 out of range (the market has 10 tokens)")
    assert check(tin=edit(tin, 0, -1)) == (-1, "cfmm_find_path_out: query 0: token_in -1 out of range (the market has 10 tokens)")
    assert check(tout=edit(tout, 4, 10)) == (-1, "cfmm_find_path_out: query 4: token_out 10 out of range (the market has 10 tokens)")
    assert check(tout=edit(tout, 1, -7)) == (-1, "cfmm_find_path_out: query 1: token_out -7 out of range (the market has 10 tokens)")
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert check(amt=edit(amt, 2, bad)) == (-1, "cfmm_find_path_out: query 2: amount_out must be finite and >= 0")
    assert check(tin=edit(tin, 4, 10), amt=edit(amt, 1, -1.0))[1].startswith("cfmm_find_path_out: query 1: amount_out")   # the first bad query


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same file with its own main, built with -fsanitize=address,undefined, run as a program on the same case list.
    (The only sanitizer run of the feature; nothing loaded into Python is sanitized.)"""
    exe = str(tmp_path / "find_out_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DFIND_OUT_CHECKS_HOST_MAIN", SHIM, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "FIND_OUT_CHECKS_HOST_OK" in r.stdout and r.stderr == ""


# ---- the GPU test's amounts, checked where no device is needed ---------------------------------------------------------------
def test_the_gpu_tests_amounts_are_within_what_the_median_pool_gives():
    """tests/test_gpu_find_path_out.py asks for 10^u of the median reserve of token_out, u in [U_LO, U_HI], and requires that
    more than half of its 1025 queries find a path.  Here, on the CPU: the largest such amount is below the reserve of at least
    half the pools that hold the token (every non-UniV3 form answers +inf only at amount >= reserve); tests/quote_precise_ref.py's
    restatement of the Product form turns the inverse's answer back into the amount; and counting only DIRECT pools whose
    reserve exceeds the amount, more than half of the queries are already answerable within one hop."""
    import quote_precise_ref as P
    import test_gpu_find_path_out as G
    batches = G.market()
    scale = G.reserve_scale(batches, G.NT)
    top = scale * 10.0 ** G.U_HI
    holders = {}
    for s, b in enumerate(batches):
        if b.kind == _lib.KIND_UNIV3:
            continue
        for c in range(b.Ai.shape[1]):
            for t, x in zip((b.Ai[:, c] - 1).tolist(), b.R[:, c].tolist()):
                holders.setdefault(t, []).append(x)
    assert sorted(holders) == list(range(G.N))                             # every token but the unheld one
    for t, R in holders.items():
        assert np.sum(np.array(R) > top[t]) * 2 >= len(R), t
    b = batches[0]                                                         # Product: the inverse, then the restatement of the quote
    assert b.kind == _lib.KIND_PRODUCT
    Ri, Ro, g = b.R[:, 0], b.R[:, 1], np.asarray(b.γ, dtype=np.float64)
    o = top[b.Ai[:, 1] - 1]
    ok = o < Ro
    x = (Ri * o) / ((Ro - o) * g)
    assert np.sum(ok) * 2 >= len(ok) and np.all(np.isfinite(x[ok]) & (x[ok] > 0))
    np.testing.assert_allclose(P.q_product(Ri[ok], Ro[ok], g[ok], x[ok]), o[ok], rtol=1e-12)
    tin, tout, amt = G.make_queries(batches, G.NT, G.COUNT)
    direct = np.zeros(G.COUNT, dtype=bool)
    for b in batches:
        if b.kind == _lib.KIND_UNIV3:
            continue
        T = b.Ai - 1
        for ci in range(T.shape[1]):
            for co in range(T.shape[1]):
                if ci != co:
                    hit = (T[None, :, ci] == tin[:, None]) & (T[None, :, co] == tout[:, None]) & (b.R[None, :, co] > amt[:, None])
                    direct |= hit.any(axis=1)
    direct &= amt > 0
    print(f"queries answerable by one direct pool: {int(direct.sum())} of {G.COUNT}")
    assert direct.sum() > G.COUNT // 2
