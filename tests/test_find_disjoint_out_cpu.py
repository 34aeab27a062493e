"""cfmm_find_disjoint_paths_out, the parts that need no device: the host reference (tests/find_disjoint_out_ref.py) against
find_path_out_ref.py with one round and against a round-by-round brute force over every walk on the exactly monotone integer
market of test_find_path_out_cpu.py; the contract's consequences on the reference; the argument list across the header and the
Python argtypes; the checks' texts under the entry's name."""
import os
import re
import subprocess

import numpy as np

from find_disjoint_out_ref import find_disjoint_out_ref, masked_find_out
from find_disjoint_ref import first_pools
from find_path_out_ref import FOUND, FOUND_NONE, FOUND_REPEATS, find_path_out_ref
from test_find_path_out_cpu import every_walk_into, integer_market_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def integer_queries():
    n = 5
    queries = [(a, b, amt) for b in range(n) for amt in (1000.0, 7.0) for a in range(n)] + [(0, 1, 0.0), (0, 1, 1.0)]
    return n, queries, tuple(np.array(x) for x in zip(*queries))


def test_one_round_is_find_path_out_ref_bit_for_bit():
    tok, quote_out = integer_market_out()
    n, _, (tin, tout, amt) = integer_queries()
    for H in (1, 2, 3):
        want = find_path_out_ref(tok, quote_out, n, tin, tout, amt, H)
        got = find_disjoint_out_ref(tok, quote_out, n, tin, tout, amt, 1, H)
        nothing = np.zeros((tin.size, int(first_pools(tok)[-1])), dtype=bool)
        masked = masked_find_out(tok, quote_out, n, tin, tout, amt, H, nothing)
        for a, b in zip(masked[1:], want[1:]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(got[1][:, 0].view(np.uint64), want[0].view(np.uint64))   # the none values included: +inf, +0.0
        for k, j in ((2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6)):
            np.testing.assert_array_equal(got[k][:, 0], want[j])
        np.testing.assert_array_equal(got[0], (want[6] != FOUND_NONE).astype(np.int32))
        # slot 0 is that answer whatever max_paths is; smaller max_paths are the leading slots
        more = find_disjoint_out_ref(tok, quote_out, n, tin, tout, amt, 4, H)
        two = find_disjoint_out_ref(tok, quote_out, n, tin, tout, amt, 2, H)
        for k in range(1, 8):
            np.testing.assert_array_equal(more[k][:, :1], got[k])
            np.testing.assert_array_equal(more[k][:, :2], two[k])


def test_reference_equals_brute_force_round_by_round():
    """Each round's amount is the cheapest walk of the enumeration that avoids the banned pools, with the fewest hops among
    those that attain it.  On this market a cost is exact and non-decreasing, so the layered minimum is the minimum over walks."""
    tok, quote_out = integer_market_out()
    n, queries, (tin, tout, amt) = integer_queries()
    H, K = 3, 8
    walks = {d: every_walk_into(tok, quote_out, d[0], d[1], H) for d in set((b, y) for _, b, y in queries)}
    n_paths, cost, n_hops, seg, row, ci, co, status = find_disjoint_out_ref(tok, quote_out, n, tin, tout, amt, K, H)
    several = exhausted = repeats = 0
    for q, (a, b, y) in enumerate(queries):
        banned = set()
        for r in range(K):
            mine = [w for w in walks[(b, y)] if w[1][0] == a and w[2][0] > 0 and not any((s, r_) in banned for s, r_, _, _ in w[0])]
            if not mine or y == 0:
                assert status[q, r] == FOUND_NONE and n_hops[q, r] == 0 and np.all(seg[q, r] == -1) and np.all(row[q, r] == -1)
                assert np.all(status[q, r:] == FOUND_NONE) and n_paths[q] == r                   # nothing ever after
                assert np.all(cost[q, r:] == (0.0 if y == 0 else np.inf))
                exhausted += 1
                break
            top = min(w[2][0] for w in mine)
            assert cost[q, r] == top, (q, r)
            assert n_hops[q, r] == min(len(w[0]) for w in mine if w[2][0] == top)
            hops = [(int(seg[q, r, k]), int(row[q, r, k]), int(ci[q, r, k]), int(co[q, r, k])) for k in range(n_hops[q, r])]
            assert any(list(w[0]) == hops for w in mine if w[2][0] == top)                       # the answer is one of the cheapest walks
            visited = [(s, r_) for s, r_, _, _ in hops]
            assert (status[q, r] == FOUND_REPEATS) == (len(set(visited)) < len(visited))
            repeats += status[q, r] == FOUND_REPEATS
            assert not banned & set(visited)
            banned |= set(visited)
            several += r > 0
        if r > 0:
            assert np.all(cost[q, 1:n_paths[q]] >= cost[q, :n_paths[q] - 1])                     # each round minimises over a subset
    assert several > 50 and exhausted > 20
    found = status != FOUND_NONE
    np.testing.assert_array_equal(n_paths, found.sum(axis=1))
    assert np.all(found == (np.arange(K)[None, :] < n_paths[:, None]))                           # the found slots are the leading ones


def test_header_and_python_agree_on_the_arguments_and_the_checks_take_the_entrys_names(tmp_path):
    from cfmmrouter_amd import _lib
    import inspect
    h = open(os.path.join(ROOT, "include", "cfmm_amd_find_disjoint_out.h")).read()
    fwd = open(os.path.join(ROOT, "include", "cfmm_amd_find_disjoint.h")).read()
    args = lambda text, name: [re.sub(r"\s+", " ", a.strip()) for a in re.search(name + r"\((.*?)\);", text, flags=re.S).group(1).split(",")]
    out, into = args(h, "int cfmm_find_disjoint_paths_out"), args(fwd, "int cfmm_find_disjoint_paths")
    assert len(out) == len(into) == 15
    assert [a.rsplit(" ", 1)[0] for a in out] == [a.rsplit(" ", 1)[0] for a in into]             # the same types in the same order
    assert out[6] == "const double* amount_out" and out[8] == "double* amount_in"                # the two amounts exchanged
    assert "L.cfmm_find_disjoint_paths_out.argtypes = L.cfmm_find_disjoint_paths.argtypes" in inspect.getsource(_lib)
    # find_checks.h under the entry's name, as a stand-alone program
    src = tmp_path / "names.cpp"
    src.write_text('#include "find_checks.h"\n#include <cstdio>\n#include <cstring>\nusing namespace cfmm;\nint main() {\n'
                   '    char msg[256];\n    const int32_t tin[2] = {0, 1}, tout[2] = {1, 0};\n    const double amt[2] = {1.0, -1.0};\n    int x = 0;\n    const void* p = &x;\n'
                   '    int rc = check_find_disjoint("cfmm_find_disjoint_paths_out", 4, 2, 3, 3, tin, tout, amt, p, p, p, p, p, p, p, p, msg, sizeof msg, "amount_out");\n'
                   '    std::printf("%d %s\\n", rc, msg);\n'
                   '    rc = check_find_disjoint("cfmm_find_disjoint_paths", 4, 2, 3, 3, tin, tout, amt, p, p, p, p, p, p, p, p, msg, sizeof msg);\n'
                   '    std::printf("%d %s\\n", rc, msg);\n'
                   '    rc = check_find_disjoint("cfmm_find_disjoint_paths_out", 4, 2, 9, 3, tin, tout, amt, p, p, p, p, p, p, p, p, msg, sizeof msg, "amount_out");\n'
                   '    std::printf("%d %s\\n", rc, msg);\n    return 0;\n}\n')
    exe = str(tmp_path / "names")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"), str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-1500:]
    lines = r.stdout.strip().split("\n")
    assert lines[0].endswith("cfmm_find_disjoint_paths_out: query 1: amount_out must be finite and >= 0"), lines
    assert lines[1].endswith("cfmm_find_disjoint_paths: query 1: amount_in must be finite and >= 0"), lines
    assert lines[2].endswith("cfmm_find_disjoint_paths_out: max_paths must be 1 .. 8 (got 9)"), lines
