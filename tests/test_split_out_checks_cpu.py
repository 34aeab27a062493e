"""csrc/split_out_grid.h (what cfmm_split_paths_out's search has of its own: the arg-min order, the greedy with the
first-bad-step rule, the status and the written values -- the ONE text the kernel and the multi-device parent compile) and
csrc/split_checks.h under the entry's name, driven by tests/native/split_out_checks_host.cpp, a stand-alone program built with
the address and undefined-behaviour sanitizers and run as a program.  The program asserts the refusals' texts itself; its greedy
rounds and statuses are compared here with the numpy statement of the contract (tests/split_paths_out_ref.py) -- the other
tests run that statement, so this is where the two are tied together."""
import os
import subprocess

import numpy as np
import pytest

import split_paths_out_ref as ref
from split_paths_ref import MAX_PATHS, POINTS, SPLIT_NAN, SPLIT_NONE, SPLIT_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hx(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def unhx(s):
    return np.array([int(t, 16) for t in s], dtype=np.uint64).view(np.float64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_out_checks") / "split_out_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "split_out_checks_host.cpp"), "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        print(r.stdout[-600:], r.stderr[-2000:])
        assert r.returncode == 0 and r.stderr == "" and "SPLIT_OUT_CHECKS_OK" in r.stdout and "SPLIT_OUT_GRID_OK" in r.stdout
        out = r.stdout.split("\n")
        return out[out.index("SPLIT_OUT_CHECKS_OK") + 1:out.index("SPLIT_OUT_GRID_OK")]
    return ask


def rounds_of_costs():
    """[K, 64] tables of costs: convex ones, ties, NaN paths, NaN tails, +inf tails (a path's capacity), free stretches"""
    j = np.arange(POINTS, dtype=np.float64)
    nan, inf = np.nan, np.inf
    conv = lambda b, cap: np.where(j < cap, b * j / np.where(j < cap, cap - j, 1.0), inf)
    out = [np.array([conv(50.0, 100.0)]),                                                # one path: every slice
           np.array([conv(50.0, 100.0), conv(50.0, 100.0)]),                             # a tie at every step: 32 and 31
           np.array([conv(50.0, 100.0)] * 8),
           np.array([conv(50.0, 100.0), np.full(POINTS, nan), conv(20.0, 80.0)]),        # a NaN path gets nothing
           np.array([np.full(POINTS, nan), np.full(POINTS, nan)]),                       # no number anywhere
           np.array([conv(50.0, 40.0), conv(50.0, 30.0)]),                               # 39 + 29 slices of room: all 63 fit
           np.array([conv(50.0, 30.0), conv(50.0, 30.0)]),                               # 29 + 29: the 59th step takes +inf
           np.array([np.full(POINTS, nan), conv(50.0, 10.0)]),                           # +inf beats the NaN path, then inf - inf
           np.array([np.maximum(j - 10.0, 0.0), j, np.zeros(POINTS) * -1.0])]            # free slices: +0.0 and -0.0 are equal
    t = conv(50.0, 100.0).copy(); t[10:] = nan
    out.append(np.array([t, conv(5.0, 100.0)]))                                          # a path that is NaN beyond a size
    t = j.copy(); t[5] = nan; t[20:] = inf
    out.append(np.array([t]))                                                            # NaN before +inf
    t = j.copy(); t[5:] = inf; t[30:] = nan
    out.append(np.array([t]))                                                            # +inf before NaN
    rng = np.random.default_rng(6)
    for _ in range(120):
        K = int(rng.integers(1, 9))
        c = np.cumsum(np.round(rng.exponential(size=(K, POINTS)), 1) * (rng.random((K, POINTS)) < 0.8), axis=1)   # many ties and free slices
        cap = rng.integers(5, 90, K)
        c[j[None, :] >= cap[:, None]] = inf
        c[rng.random((K, POINTS)) < 0.02] = nan
        out.append(c)
    return out


def test_the_greedy_is_the_references(program):
    tables = rounds_of_costs()
    rng = np.random.default_rng(9)
    before = [int(b) for b in rng.choice([ref.CLEAN, ref.CLEAN, ref.CLEAN, ref.BAD_INF, ref.BAD_NAN], len(tables))]
    before[:12] = [ref.CLEAN] * 12
    got = program([f"G {b} {c.shape[0]} " + " ".join(hx(v) for v in c.ravel()) for b, c in zip(before, tables)])
    assert len(got) == len(tables)
    seen = set()
    for b, c, line in zip(before, tables, got):
        K = c.shape[0]
        full = np.full((1, MAX_PATHS, POINTS), np.nan)
        full[0, :K] = c
        n, bad = ref.greedy_out(full, np.array([K]), bad=np.array([b]))
        t = [int(v) for v in line.split()[1:]]
        assert t[1:] == n[0].tolist(), (K, line, n[0])
        assert t[0] == int(bad[0]), (K, line)
        assert sum(t[1:]) == POINTS - 1 and all(v == 0 for v in t[1 + K:])
        if b != ref.CLEAN:
            assert t[0] == b                                              # what an earlier round reported stays
        else:
            seen.add(t[0])
    assert seen == {ref.CLEAN, ref.BAD_INF, ref.BAD_NAN}
    first = lambda i: got[i].split()[1:]
    assert first(1)[:3] == ["0", "32", "31"] and first(2)[1:] == ["8"] * 7 + ["7"]
    assert first(3)[0] == "0" and first(3)[2] == "0" and first(4)[:2] == [str(ref.BAD_NAN), "63"]   # (no number: every slice to path 0)
    assert first(5)[0] == str(ref.CLEAN) and first(6)[0] == str(ref.BAD_INF) and first(7)[0] == str(ref.BAD_INF)
    assert first(8)[:4] == ["0", "10", "0", "53"]                          # the free slices first, the smaller path among equals
    assert first(10)[0] == str(ref.BAD_NAN) and first(11)[0] == str(ref.BAD_INF)


def test_statuses_and_written_values(program):
    nan, inf = np.nan, np.inf
    cases = [(ref.CLEAN, 10.0, 5.0, 3.0, SPLIT_OK, 3.0, 3.0), (ref.CLEAN, 0.0, 0.0, 0.0, SPLIT_NONE, 0.0, 0.0),
             (ref.CLEAN, 0.0, 7.0, 7.0, SPLIT_NONE, 0.0, 0.0), (ref.CLEAN, 10.0, 0.0, -0.0, SPLIT_OK, -0.0, -0.0),
             (ref.CLEAN, 10.0, nan, 3.0, SPLIT_NAN, nan, nan), (ref.BAD_NAN, 10.0, 5.0, 3.0, SPLIT_NAN, nan, nan),
             (ref.BAD_INF, 10.0, inf, 3.0, ref.SPLIT_UNOBTAINABLE, 0.0, inf), (ref.BAD_INF, 10.0, nan, nan, ref.SPLIT_UNOBTAINABLE, 0.0, inf),
             (ref.BAD_INF, 0.0, 5.0, 3.0, ref.SPLIT_UNOBTAINABLE, 0.0, inf), (ref.BAD_NAN, nan, nan, nan, SPLIT_NAN, nan, nan),
             (ref.CLEAN, 10.0, inf, inf, SPLIT_OK, inf, inf)]
    got = program([f"A {b} {hx(B)} {hx(t)} {hx(v)}" for b, B, t, v, _, _, _ in cases])
    for line, case in zip(got, cases):
        st, share, cost = int(line.split()[1]), unhx([line.split()[2]])[0], unhx([line.split()[3]])[0]
        assert st == case[4], (line, case)
        want_st = ref.answer_status(np.array([case[0]]), np.array([case[1]]), np.array([case[2]]))
        assert want_st[0] == st, (line, case)
        for have, want, is_cost in ((share, case[5], False), (cost, case[6], True)):
            w = ref.written(np.array([case[3]]), want_st, cost=is_cost)[0]
            if np.isnan(want):
                assert np.isnan(have) and np.isnan(w)
            else:
                assert hx(have) == hx(want) == hx(w), (line, case)
