"""csrc/split_checks.h (the checks of cfmm_split_paths: scalars, arrays, the orders' path ranges and amounts, the paths named by
order, and no pool twice in an order) and csrc/split_grid.h (the search's arithmetic: the ONE text the kernel and the multi-device
parent compile) driven by tests/native/split_checks_host.cpp, a stand-alone program built with the address and
undefined-behaviour sanitizers and run as a program.  The program asserts every refusal's text itself; its grid points, greedy
rounds, remainders and statuses are compared here, bit for bit, with the numpy statement of the contract
(tests/split_paths_ref.py) -- the other tests run that statement, so this is where the two are tied together."""
import os
import subprocess

import numpy as np
import pytest

import split_paths_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hx(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def unhx(s):
    return np.array([int(t, 16) for t in s], dtype=np.uint64).view(np.float64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_checks") / "split_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "split_checks_host.cpp"), "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        print(r.stdout[-600:], r.stderr[-2000:])
        assert r.returncode == 0 and r.stderr == "" and "SPLIT_CHECKS_OK" in r.stdout and "SPLIT_GRID_OK" in r.stdout
        out = r.stdout.split("\n")
        return out[out.index("SPLIT_CHECKS_OK") + 1:out.index("SPLIT_GRID_OK")]
    return ask


def test_the_checks_pass_and_the_grid_points_are_the_references_bits(program):
    up = lambda x, k: np.float64(x) + k * np.spacing(np.float64(x))
    cases = [(0.0, 1.0), (0.0, 1e6), (0.0, 123456.789), (3.0, 0.0), (0.0, 0.0), (1e-300, 3e-300), (0.0, 5e-324), (0.0, 1.7e308),
             (1.0, 3 * np.spacing(1.0)), (1e9, 63.0), (7.25, up(1.0, 5)), (np.nan, 1.0), (1.0, np.nan)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        cases.append((10.0 ** rng.uniform(-3, 12) * rng.integers(0, 2), 10.0 ** rng.uniform(-12, 12)))
    b = np.array(cases)
    got = program([f"P {hx(base)} {hx(rem)}" for base, rem in b])
    with np.errstate(invalid="ignore"):
        want = ref.grid_points(b[:, 0], b[:, 1])
    assert len(got) == len(b)
    for k, line in enumerate(got):
        x = unhx(line.split()[1:])
        np.testing.assert_array_equal(np.isnan(x), np.isnan(want[k]))
        np.testing.assert_array_equal(x.view(np.uint64)[~np.isnan(x)], want[k].view(np.uint64)[~np.isnan(want[k])], err_msg=str(b[k]))
        if not np.any(np.isnan(b[k])):                                # monotone, from the share so far to the share plus the rest
            assert np.all(np.diff(x) >= 0) and x[0] == b[k, 0] and x[-1] == b[k, 0] + b[k, 1]


def rounds_of_outputs():
    """[K, 64] tables of outputs: concave ones, ties, NaN paths, NaN tails, flat and falling stretches, -inf steps"""
    j = np.arange(64, dtype=np.float64)
    nan = np.nan
    out = []
    conc = lambda a, b: a * j / (b + j)
    out.append(np.array([conc(100.0, 50.0)]))                                           # one path: every slice
    out.append(np.array([conc(100.0, 50.0), conc(100.0, 50.0)]))                        # a tie at every step: 32 and 31
    out.append(np.array([conc(100.0, 50.0)] * 8))
    out.append(np.array([conc(100.0, 50.0), np.full(64, nan), conc(80.0, 20.0)]))       # a NaN path gets nothing
    out.append(np.array([np.full(64, nan), np.full(64, nan)]))                          # no number anywhere
    t = conc(100.0, 50.0).copy(); t[10:] = nan
    out.append(np.array([t, conc(10.0, 50.0)]))                                         # a path that is NaN beyond a size
    out.append(np.array([np.minimum(j, 10.0), np.minimum(j, 20.0), np.minimum(j, 5.0)]))   # saturating: zero increments taken
    out.append(np.array([np.zeros(64), -0.0 * j]))                                      # +0.0 and -0.0 are equal: the smaller path
    out.append(np.array([-j, -2.0 * j]))                                                # falling: negative increments, still numbers
    t = conc(5.0, 1.0).copy(); t[3:] = -np.inf
    out.append(np.array([np.full(64, nan), t]))                                         # a step to -inf beats a NaN; then inf - inf is no number
    rng = np.random.default_rng(6)
    for _ in range(120):
        K = int(rng.integers(1, 9))
        y = np.cumsum(np.round(rng.exponential(size=(K, 64)), 1) * (rng.random((K, 64)) < 0.8), axis=1)   # many ties and flats
        y[rng.random((K, 64)) < 0.03] = nan
        out.append(y)
    return out


def test_the_greedy_is_the_references(program):
    tables = rounds_of_outputs()
    got = program([f"G {y.shape[0]} " + " ".join(hx(v) for v in y.ravel()) for y in tables])
    assert len(got) == len(tables)
    seen = set()
    for y, line in zip(tables, got):
        K = y.shape[0]
        full = np.full((1, ref.MAX_PATHS, ref.POINTS), np.nan)
        full[0, :K] = y
        with np.errstate(invalid="ignore"):
            n, step_nan, step_flat = ref.greedy(full, np.array([K]))
        t = [int(v) for v in line.split()[1:]]
        assert t[1:] == n[0].tolist(), (K, line, n[0])
        assert t[0] == int(step_nan[0]) + 2 * int(step_flat[0]), (K, line)
        assert sum(t[1:]) == ref.POINTS - 1 and all(v == 0 for v in t[1 + K:])
        seen.add(t[0])
    assert seen >= {0, 1, 2}
    assert got[1].split()[1:4] == ["0", "32", "31"] and got[2].split()[2:] == ["8"] * 7 + ["7"]
    assert got[3].split()[3] == "0" and got[4].split()[1:3] == ["1", "63"]              # (no number: every slice to path 0)


def test_remainders_and_statuses(program):
    rng = np.random.default_rng(8)
    lines, want = [], []
    for _ in range(200):
        K = int(rng.integers(1, 9))
        A = 10.0 ** rng.uniform(-3, 9)
        base = rng.dirichlet(np.ones(K)) * A * rng.choice([0.5, 0.999, 1.0, 1.0 + 1e-15])
        total = base[0]
        for v in base[1:]:
            total = total + v
        lines.append(f"R {hx(A)} {K} " + " ".join(hx(v) for v in base))
        want.append(np.maximum(A - total, 0.0))
    lines.append(f"R {hx(np.nan)} 1 {hx(1.0)}")
    want.append(np.nan)
    got = program(lines)
    g = unhx([line.split()[1] for line in got])
    w = np.array(want)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    np.testing.assert_array_equal(g.view(np.uint64)[~np.isnan(w)], w.view(np.uint64)[~np.isnan(w)])
    nan = np.nan
    cases = [(0, 0, 10.0, 5.0, 3.0, ref.SPLIT_OK, 3.0), (0, 1, 10.0, 5.0, 3.0, ref.SPLIT_SATURATED, 3.0),
             (0, 1, 0.0, 0.0, 0.0, ref.SPLIT_NONE, 0.0), (0, 0, 10.0, 0.0, 3.0, ref.SPLIT_NONE, 0.0), (0, 1, 10.0, -1.0, 3.0, ref.SPLIT_NONE, 0.0),
             (0, 0, 10.0, -0.0, -0.0, ref.SPLIT_NONE, 0.0), (1, 0, 10.0, 5.0, 3.0, ref.SPLIT_NAN, nan), (0, 0, 10.0, nan, 3.0, ref.SPLIT_NAN, nan),
             (1, 1, nan, nan, nan, ref.SPLIT_NAN, nan)]
    got = program([f"A {a} {f} {hx(A)} {hx(t)} {hx(v)}" for a, f, A, t, v, _, _ in cases])
    for line, case in zip(got, cases):
        st, v = int(line.split()[1]), unhx([line.split()[2]])[0]
        assert st == case[5], (line, case)
        if np.isnan(case[6]):
            assert np.isnan(v)
        else:
            assert hx(v) == hx(case[6]), (line, case)                  # (NONE: +0.0)
