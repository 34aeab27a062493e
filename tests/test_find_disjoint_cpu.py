"""cfmm_find_disjoint_paths, the parts that need no device: the host reference (tests/find_disjoint_ref.py) against
find_path_ref.py with one round and against brute force on the exactly monotone integer market; the chunking rule and every
refusal text through a stand-alone host program over csrc/find_checks.h (built plainly and under the sanitizers, run as a
program); the argument list across the header, the Python argtypes and the Julia ccall; the router-level mapping and
route_order on a recording context."""
import os
import re
import subprocess

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from find_disjoint_ref import find_disjoint_ref, first_pools, masked_find
from find_path_ref import FOUND, FOUND_NONE, FOUND_REPEATS, find_path_ref
from test_find_path_cpu import every_walk, integer_market
from test_quote_cpu import RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "native", "find_disjoint_checks_host.cpp")


# ---- the reference ----------------------------------------------------------------------------------------------------------
def integer_queries():
    n = 5
    queries = [(a, b, amt) for a in range(n) for amt in (1000.0, 7.0) for b in range(n)] + [(0, 1, 0.0), (0, 1, 1.0)]
    return n, queries, tuple(np.array(x) for x in zip(*queries))


def test_one_round_is_find_path_ref_bit_for_bit():
    tok, quote = integer_market()
    n, _, (tin, tout, amt) = integer_queries()
    for H in (1, 2, 3):
        want = find_path_ref(tok, quote, n, tin, tout, amt, H)
        got = find_disjoint_ref(tok, quote, n, tin, tout, amt, 1, H)
        nothing = np.zeros((tin.size, int(first_pools(tok)[-1])), dtype=bool)
        for a, b in zip(masked_find(tok, quote, n, tin, tout, amt, H, nothing), want):
            np.testing.assert_array_equal(a, b)
        assert got[1].shape == (tin.size, 1) and got[3].shape == (tin.size, 1, H)
        np.testing.assert_array_equal(got[1][:, 0].view(np.uint64), want[0].view(np.uint64))
        for k, j in ((2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6)):
            np.testing.assert_array_equal(got[k][:, 0], want[j])
        np.testing.assert_array_equal(got[0], (want[6] != FOUND_NONE).astype(np.int32))
        # ... and slot 0 is that answer whatever max_paths is; smaller max_paths are the leading slots
        more = find_disjoint_ref(tok, quote, n, tin, tout, amt, 4, H)
        for k in range(1, 8):
            np.testing.assert_array_equal(more[k][:, :1], got[k])
        two = find_disjoint_ref(tok, quote, n, tin, tout, amt, 2, H)
        for k in range(1, 8):
            np.testing.assert_array_equal(more[k][:, :2], two[k])


def test_reference_equals_brute_force_round_by_round():
    """Each round takes the best remaining walk of the enumeration that avoids the banned pools, with the contract's tie-break:
    the fewest hops; then, walking back from the end, the smallest hop among the walks that attain the layer's best AMONG THE
    WALKS THAT AVOID THE BAN at every hop.  On this market a quote is exact and non-decreasing, so the layered maximum is the
    maximum over the walks."""
    tok, quote = integer_market()
    n, queries, (tin, tout, amt) = integer_queries()
    H, K = 3, 8
    walks = {src: every_walk(tok, quote, src[0], src[1], H) for src in set((a, x) for a, _, x in queries)}
    n_paths, out, n_hops, seg, row, ci, co, status = find_disjoint_ref(tok, quote, n, tin, tout, amt, K, H)
    several = repeats = exhausted = 0
    for q, (a, b, x) in enumerate(queries):
        banned = set()
        for r in range(K):
            mine = [w for w in walks[(a, x)] if not any((s, r_) in banned for s, r_, _, _ in w[0])]
            layer = {}
            for _, toks, vals in mine:
                layer[(len(toks), toks[-1])] = max(layer.get((len(toks), toks[-1]), 0.0), vals[-1])
            top = max((vals[-1] for _, toks, vals in mine if toks[-1] == b), default=0.0)
            assert out[q, r] == top, (q, r)
            if top <= 0:
                assert status[q, r] == FOUND_NONE and n_hops[q, r] == 0 and np.all(seg[q, r] == -1) and np.all(row[q, r] == -1)
                assert np.all(status[q, r:] == FOUND_NONE) and np.all(out[q, r:] == 0.0) and n_paths[q] == r   # nothing ever after
                exhausted += 1
                break
            fewest = min(len(toks) for _, toks, vals in mine if toks[-1] == b and vals[-1] == top)
            cands = [hops for hops, toks, vals in mine if len(toks) == fewest and toks[-1] == b and
                     all(vals[k] == layer[(k + 1, toks[k])] for k in range(fewest))]
            for k in reversed(range(fewest)):
                pick = min(w[k] for w in cands)
                cands = [w for w in cands if w[k] == pick]
            got = [(seg[q, r, k], row[q, r, k], ci[q, r, k], co[q, r, k]) for k in range(n_hops[q, r])]
            assert got == list(cands[0]), (q, r)
            on_it = [(s, r_) for s, r_, _, _ in got]
            assert status[q, r] == (FOUND_REPEATS if len(set(on_it)) < len(on_it) else FOUND)
            repeats += status[q, r] == FOUND_REPEATS
            assert not banned & set(on_it)                                 # no pool occurs in two paths of a query
            banned |= set(on_it)
            if r:
                assert out[q, r] <= out[q, r - 1]
        else:
            assert n_paths[q] == K
        several += n_paths[q] >= 2
    print(f"integer market: {several} of {len(queries)} queries with two or more paths, {exhausted} ran out of paths, "
          f"{repeats} paths that re-enter a pool; n_paths histogram {np.bincount(n_paths, minlength=K + 1).tolist()}")
    assert several > len(queries) // 2 and exhausted > 5 and repeats > 0


# ---- csrc/find_checks.h through a stand-alone program -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("find_disjoint_checks_host")
    plain, sanitized = str(d / "plain"), str(d / "sanitized")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", HOST, "-o", plain], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", HOST, "-o", sanitized],
                   check=True)
    return plain, sanitized


def test_every_refusal_text_plainly_and_under_the_sanitizers(programs):
    """the case list of tests/native/find_disjoint_checks_host.cpp compares every refusal's whole text; run as a program, twice.
    (The only sanitizer run of the feature; nothing loaded into Python is sanitized.)"""
    for exe in programs:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr[-2000:])
        assert r.returncode == 0 and "FIND_DISJOINT_CHECKS_HOST_OK" in r.stdout and r.stderr == ""
    src = open(HOST).read()
    for text in ("count must be >= 0", "max_paths must be 1 .. 8 (got 0)", "max_paths must be 1 .. 8 (got 9)", "max_hops must be 1 .. 8 (got 0)",
                 "max_hops must be 1 .. 8 (got 9)", "null query array", "token_in 10 out of range (the market has 10 tokens)",
                 "token_out 77 out of range (the market has 10 tokens)", "amount_in must be finite and >= 0"):
        assert "cfmm_find_disjoint_paths: " in src and text in src, text


def test_the_chunk_rule(programs):
    """monotone (more tokens, hops or pools never allow more queries; a larger budget never fewer), never less than 1, and the
    layers plus the ban rows of a chunk within the budget whenever one query fits"""
    outs = [subprocess.run([exe, "chunks"], capture_output=True, text=True, timeout=120) for exe in programs]
    assert all(o.returncode == 0 and o.stderr == "" for o in outs) and outs[0].stdout == outs[1].stdout
    table = {}
    for line in outs[0].stdout.split("\n"):
        if line:
            t, h, p, b, chunk = (int(v) for v in line.split())
            table[(t, h, p, b)] = chunk
    assert len(table) == 7 * 8 * 8 * 4
    per_query = lambda t, h, p: ((h + 1) * max(t, 1) + max((p + 63) // 64, 1)) * 8
    fits = over = 0
    for (t, h, p, b), chunk in table.items():
        assert 1 <= chunk <= 1 << 20
        if per_query(t, h, p) <= b:
            assert chunk * per_query(t, h, p) <= b and (chunk == 1 << 20 or (chunk + 1) * per_query(t, h, p) > b)   # within, and no smaller than need be
            fits += 1
        else:
            assert chunk == 1                                              # one query still runs, over the budget
            over += 1
    keys = sorted(table)
    axis = lambda k: sorted({key[k] for key in keys})
    for (t, h, p, b), chunk in table.items():
        for k, values in enumerate((axis(0), axis(1), axis(2), axis(3))):
            i = values.index((t, h, p, b)[k])
            if i + 1 < len(values):
                nxt = list((t, h, p, b))
                nxt[k] = values[i + 1]
                assert (table[tuple(nxt)] >= chunk) if k == 3 else (table[tuple(nxt)] <= chunk), ((t, h, p, b), k)
    assert fits > 100 and over > 100
    # with few pools the ban costs nothing against find_path's rule; a million pools on few tokens is what it costs
    assert table[(65536, 8, 2056, 256 << 20)] == 56 and table[(65, 3, 1000000, 256 << 20)] == (256 << 20) // ((4 * 65 + 15625) * 8)


def test_find_checks_header_still_needs_no_hip():
    src = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "find_checks.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert not any("hip" in i or i in ("ctx.h", "sweep.h", "devbuf.h", "hostres.h") for i in includes), includes
    assert "check_find_disjoint" in src and "find_disjoint_chunk_queries" in src


# ---- the header, the Python argtypes and the Julia ccall ------------------------------------------------------------------------
def test_header_python_and_julia_agree_on_the_arguments():
    raw = open(os.path.join(ROOT, "include", "cfmm_amd_find_disjoint.h")).read()
    for phrase in ("SUCCESSIVE LAYERED SEARCH WITH A GROWING BAN SET", "OF THE\n *     SAME QUERY", "bit for bit", "A / K", "GREEDY successive-best",
                   "CFMM_FOUND_NONE", "CFMM_FOUND_REPEATS", "r*count + q", "(r*max_hops + k)*count + q", "CFMM_ERR_UNSUPPORTED", "256 MiB",
                   "find_lds", "OUT OF SCOPE"):
        assert phrase in raw, phrase                                       # the contract is stated where the caller reads it
    assert "cfmm_find_disjoint_paths" not in open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()   # the addition lives in its own header
    h = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    params = re.search(r"int\s+cfmm_find_disjoint_paths\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
    parts = [p.strip() for p in params.replace("\n", " ").split(",")]
    want_c = ["cfmm_ctx*", "int64_t", "int32_t", "int32_t", "int32_t*", "int32_t*", "double*", "int32_t*", "double*", "int32_t*", "int32_t*",
              "int32_t*", "int64_t*", "int32_t*", "int32_t*"]
    want_py = ["_ctx", "C.c_int64", "C.c_int32", "C.c_int32", "_i32p", "_i32p", "_f64p", "_i32p", "_f64p", "_i32p", "_i32p", "_i32p", "_i64p",
               "_i32p", "_i32p"]
    want_jl = ["Ptr{Cvoid}", "Int64", "Int32", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Ptr{Float64}", "Ptr{Int32}", "Ptr{Float64}", "Ptr{Int32}",
               "Ptr{Int32}", "Ptr{Int32}", "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}"]
    assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == want_c
    assert [p.split()[-1] for p in parts] == ["ctx", "count", "max_paths", "max_hops", "token_in", "token_out", "amount_in", "n_paths", "amount_out",
                                              "n_hops", "status", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out"]
    assert [p.startswith("const") for p in parts[4:]] == [True] * 3 + [False] * 8       # three inputs, eight outputs
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    argtypes = [a.strip() for a in re.search(r"L\.cfmm_find_disjoint_paths\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert argtypes == want_py
    module = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    jl = open(os.path.join(ROOT, "julia", "src", "find_disjoint_paths.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_find_disjoint_paths,\s*LIB\),\s*Cint,\s*\((.*?)\),\s*r\.ctx", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.replace("\n", " ").split(",")] == want_jl
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    assert "find_disjoint_paths" in exported and 'include("find_disjoint_paths.jl")' in module and "function find_disjoint_paths(" in jl
    assert "find_paths" in exported                                        # the batch form of cfmm_find_path keeps its name
    tests = open(os.path.join(ROOT, "julia", "test", "find_disjoint_paths.jl")).read()
    assert "find_disjoint_paths(" in tests and "split_paths(" in tests and "swap_paths!(" in tests
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "find_disjoint_paths" in open(os.path.join(ROOT, doc)).read(), doc
    assert hasattr(_lib.Context, "find_disjoint_paths")
    for name in ("find_disjoint_paths", "route_order"):
        assert name in cr.__all__ and callable(getattr(cr, name))
    names = re.findall(r"#define (CFMM_\w+)", raw)
    assert names == ["CFMM_AMD_FIND_DISJOINT_H"]                           # no new codes: CFMM_FOUND* and CFMM_MAX_SPLIT_PATHS serve


def test_device_text_keeps_the_search_headers_rules():
    csrc = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")
    src = open(os.path.join(csrc, "find_disjoint_kernels.h")).read()
    assert "atomicAdd" not in src and "case CFMM_KIND_" not in src and "__ballot" in src and "atomicMin" in src
    assert '#include "find_disjoint_kernels.h"' in open(os.path.join(csrc, "split_paths_kernels.h")).read().rstrip().split("\n")[-1]
    assert "FindBanArgs" in open(os.path.join(csrc, "sweep.h")).read()


# ---- the router-level calls on a recording context -------------------------------------------------------------------------
class RecordingDisjointContext(RecordingContext):
    """answers query q with the paths of self.answers[q], a list of (hops, status), and records what it was sent"""

    def find_disjoint_paths(self, token_in, token_out, amount_in, max_paths=4, max_hops=3):
        self.calls.append(("find", np.array(token_in), np.array(token_out), np.array(amount_in), max_paths, max_hops))
        n = len(self.calls[-1][3])
        K, H = max_paths, max_hops
        seg, ci, co = (np.full((n, K, H), -1, dtype=np.int32) for _ in range(3))
        row = np.full((n, K, H), -1, dtype=np.int64)
        n_hops, status = np.zeros((n, K), dtype=np.int32), np.full((n, K), FOUND_NONE, dtype=np.int32)
        out, n_paths = np.zeros((n, K)), np.zeros(n, dtype=np.int32)
        for q, paths in enumerate(self.answers[:n]):
            n_paths[q] = len(paths)
            for r, (hops, st) in enumerate(paths):
                n_hops[q, r], status[q, r], out[q, r] = len(hops), st, 100.0 * (q + 1) - r
                for k, hop in enumerate(hops):
                    seg[q, r, k], row[q, r, k], ci[q, r, k], co[q, r, k] = hop
        return n_paths, out, n_hops, seg, row, ci, co, status

    def split_paths(self, order_first, amount_in, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, rounds=5):
        self.calls.append(("split", np.array(order_first), np.array(amount_in), np.array(n_hops), np.array(hop_seg), np.array(hop_row), rounds))
        n, g = len(n_hops), len(amount_in)
        return np.arange(n) + 0.5, np.arange(n) + 0.25, 10.0 + np.arange(g), np.zeros(g, dtype=np.int32)


def disjoint_router():
    # mixed_router: 0 product {1,2}, 1 geomean {2,3}, 2 host {1,3}, 3 product {3,4}, 4 weighted {1,2,4}, 5 product {1,4}
    r, pools = mixed_router()
    L, ctx = r._layout, r._backend.ctx
    ctx.__class__ = RecordingDisjointContext
    where = {i: (L.seg_of[L.locate(i)[1]], L.locate(i)[2]) for i in (0, 1, 3, 4, 5)}
    hop = lambda i, t_in, t_out: (*where[i], list(pools[i].Ai).index(t_in), list(pools[i].Ai).index(t_out))
    ctx.answers = [[([hop(5, 1, 4)], FOUND), ([hop(4, 1, 4)], FOUND), ([hop(0, 1, 2), hop(1, 2, 3), hop(3, 3, 4)], FOUND)],   # 1 -> 4, three ways
                   [],                                                                                                # nothing
                   [([hop(4, 4, 2)], FOUND), ([hop(5, 4, 1), hop(0, 1, 2)], FOUND)],                                   # 4 -> 2, two ways
                   [([hop(5, 4, 1), hop(4, 1, 4), hop(5, 4, 1)], FOUND_REPEATS), ([hop(4, 4, 1)], FOUND)]]             # a walk that repeats, then a path
    return r, ctx


def test_router_maps_tokens_and_lists_the_paths_the_way_split_paths_takes_them():
    r, ctx = disjoint_router()
    out, pl, tk, status = cr.find_disjoint_paths(r, [1, 3, 4, 4], [4, 3, 2, 1], [1.0, 2.0, 3.0, 4.0], max_paths=3, max_hops=3)
    assert len(ctx.calls) == 1
    _, tin, tout, amt, K, H = ctx.calls[0]
    assert tin.tolist() == [0, 2, 3, 3] and tout.tolist() == [3, 2, 1, 0] and amt.tolist() == [1.0, 2.0, 3.0, 4.0] and (K, H) == (3, 3)   # 0-based
    assert pl == [[[5], [4], [0, 1, 3]], [], [[4], [5, 0]], [[4]]]         # positions in r.cfmms; the repeating walk is left out
    assert tk == [[[1, 4], [1, 4], [1, 2, 3, 4]], [], [[4, 2], [4, 1, 2]], [[4, 1]]]
    assert [o.tolist() for o in out] == [[100.0, 99.0, 98.0], [], [300.0, 299.0], [399.0]]
    assert [s.tolist() for s in status] == [[FOUND] * 3, [], [FOUND] * 2, [FOUND]]
    # usable_only=False lists the walk with its status
    out, pl, tk, status = cr.find_disjoint_paths(r, [1, 3, 4, 4], [4, 3, 2, 1], [1.0, 2.0, 3.0, 4.0], max_paths=3, usable_only=False)
    assert pl[3] == [[5, 4, 5], [4]] and tk[3] == [[4, 1, 4, 1], [4, 1]] and status[3].tolist() == [FOUND_REPEATS, FOUND] and out[3].tolist() == [400.0, 399.0]
    assert pl[:3] == [[[5], [4], [0, 1, 3]], [], [[4], [5, 0]]]
    # what comes back is what split_paths takes
    ctx.calls.clear()
    cr.split_paths(r, [pl[0], pl[2]], [tk[0], tk[2]], [1.0, 3.0])
    _, first, amt, n_hops, seg, row, rounds = ctx.calls[0]
    assert first.tolist() == [0, 3, 5] and n_hops.tolist() == [1, 1, 3, 1, 2] and rounds == 5
    # defaults, scalars broadcast, and the refusals come before the context is touched
    ctx.calls.clear()
    cr.find_disjoint_paths(r, 1, [2, 3], 5.0)
    assert ctx.calls[0][1].tolist() == [0, 0] and ctx.calls[0][2].tolist() == [1, 2] and ctx.calls[0][3].tolist() == [5.0, 5.0] and ctx.calls[0][4:] == (4, 3)
    ctx.calls.clear()
    for bad_in, bad_out, match in ((0, 1, "query 0: token_in 0 out of range 1:4"), ([1, 5], 1, "query 1: token_in 5"), (1, [1, 2, 9], "query 2: token_out 9")):
        with pytest.raises(cr.ArgumentError, match=match):
            cr.find_disjoint_paths(r, bad_in, bad_out, 1.0)
    with pytest.raises(cr.ArgumentError, match="one entry per query"):
        cr.find_disjoint_paths(r, [1, 2], [1, 2, 3], 1.0)
    assert ctx.calls == []


def test_route_order_composes_find_and_split():
    r, ctx = disjoint_router()
    pools, tokens, x, y, total, status = cr.route_order(r, [1, 3, 4, 4], [4, 3, 2, 1], [10.0, 20.0, 30.0, 40.0], max_paths=3, rounds=7)
    assert [c[0] for c in ctx.calls] == ["find", "split"]
    assert ctx.calls[0][3].tolist() == [10.0, 20.0, 30.0, 40.0] and ctx.calls[0][4:] == (3, 3)        # the probe defaults to the amount
    _, first, amt, n_hops, seg, row, rounds = ctx.calls[1]
    assert first.tolist() == [0, 3, 5, 6] and amt.tolist() == [10.0, 30.0, 40.0] and rounds == 7      # the empty order is not sent
    assert n_hops.tolist() == [1, 1, 3, 1, 2, 1]                                                      # ... nor the walk that repeats
    assert pools == [[[5], [4], [0, 1, 3]], [], [[4], [5, 0]], [[4]]] and tokens[3] == [[4, 1]]
    assert [v.tolist() for v in x] == [[0.5, 1.5, 2.5], [], [3.5, 4.5], [5.5]] and [v.tolist() for v in y] == [[0.25, 1.25, 2.25], [], [3.25, 4.25], [5.25]]
    assert total.tolist() == [10.0, 0.0, 11.0, 12.0] and status.tolist() == [cr.SPLIT_OK, cr.SPLIT_NONE, cr.SPLIT_OK, cr.SPLIT_OK]
    # a probe of its own goes to the search, the amounts to the split
    ctx.calls.clear()
    cr.route_order(r, 1, 4, 100.0, probe=25.0)
    assert ctx.calls[0][3].tolist() == [25.0] and ctx.calls[0][4:] == (4, 3) and ctx.calls[1][2].tolist() == [100.0] and ctx.calls[1][6] == 5
    # nothing found anywhere: split_paths is not called at all
    ctx.calls.clear()
    ctx.answers = [[], []]
    pools, tokens, x, y, total, status = cr.route_order(r, [1, 2], [2, 3], 5.0)
    assert [c[0] for c in ctx.calls] == ["find"] and pools == [[], []] and tokens == [[], []]
    assert total.tolist() == [0.0, 0.0] and status.tolist() == [cr.SPLIT_NONE] * 2 and all(v.size == 0 for v in x + y)
    with pytest.raises(cr.ArgumentError, match="one entry per order"):
        cr.route_order(r, [1, 2], [2, 3], [1.0, 2.0, 3.0])
