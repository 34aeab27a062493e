"""csrc/size_checks.h (the scalar, limit and value checks of cfmm_size_path) and csrc/size_grid.h (the search's arithmetic: the ONE
text the kernel and the multi-device parent compile) driven by tests/native/size_checks_host.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers and run as a program.  The program asserts the checks itself; its trial
sizes, gains, selections and answers are compared here, bit for bit, with the numpy statement of the contract
(tests/size_path_ref.py) -- the other CPU tests run that statement, so this is where the two are tied together."""
import os
import subprocess

import numpy as np
import pytest

import size_path_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hx(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def unhx(s):
    return np.array([int(t, 16) for t in s], dtype=np.uint64).view(np.float64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("size_checks") / "size_checks_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "size_checks_host.cpp"), "-o", exe], check=True)

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        print(r.stdout[-600:], r.stderr[-2000:])
        assert r.returncode == 0 and r.stderr == "" and "SIZE_CHECKS_OK" in r.stdout and "SIZE_GRID_OK" in r.stdout
        out = r.stdout.split("\n")
        return out[out.index("SIZE_CHECKS_OK") + 1:out.index("SIZE_GRID_OK")]
    return ask


def brackets():
    up = lambda x, k: np.float64(x) + k * np.spacing(np.float64(x))
    out = [(0.0, 1.0), (0.0, 1e6), (0.0, 123456.789), (3.0, 3.0), (0.0, 0.0), (1e-300, 3e-300), (0.0, 5e-324), (0.0, 1.7e308),
           (1.0, up(1.0, 3)), (1e9, up(1e9, 5)), (7.25, up(7.25, 1)), (0.1, up(0.1, 70)), (1e15, 1e15 + 63.0), (np.nan, np.nan)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        lo = 10.0 ** rng.uniform(-3, 12)
        out.append((lo, lo * (1.0 + 10.0 ** rng.uniform(-15.5, 2))))
    return np.array(out, dtype=np.float64)


def test_the_checks_pass_and_the_trial_sizes_are_the_references_bits(program):
    b = brackets()
    got = program([f"T {hx(lo)} {hx(hi)}" for lo, hi in b])
    with np.errstate(invalid="ignore"):
        want = ref.trial_sizes(b[:, 0], b[:, 1])
    assert len(got) == len(b)
    for k, line in enumerate(got):
        x = unhx(line.split()[1:])
        np.testing.assert_array_equal(x.view(np.uint64)[~np.isnan(x)], want[k].view(np.uint64)[~np.isnan(want[k])], err_msg=str(b[k]))
        np.testing.assert_array_equal(np.isnan(x), np.isnan(want[k]))
        if not np.isnan(b[k, 0]):                                  # monotone, inside the bracket, the ends exact
            assert np.all(np.diff(x) >= 0) and x[0] == b[k, 0] and x[-1] == b[k, 1]
    assert len({float(v) for v in unhx(got[8].split()[1:])}) == 4   # a bracket three ulps wide has four distinct sizes
    assert len(set(got[3].split()[1:])) == 1                        # lo == hi: one size


def test_gains_are_the_references_bits(program):
    rng = np.random.default_rng(4)
    n = 300
    vi, vo = 10.0 ** rng.uniform(-3, 3, n), 10.0 ** rng.uniform(-3, 3, n)
    x = 10.0 ** rng.uniform(-6, 12, n)
    y = x * vi / vo * (1.0 + 10.0 ** rng.uniform(-16, 0, n) * rng.choice([-1.0, 1.0], n))   # gains that cancel to a few ulps
    got = program([f"G {hx(a)} {hx(b)} {hx(c)} {hx(d)}" for a, b, c, d in zip(vi, vo, x, y)])
    want = ref.gains(vi, vo, x[:, None], y[:, None])[:, 0]
    np.testing.assert_array_equal(unhx([g.split()[1] for g in got]).view(np.uint64), want.view(np.uint64))


def selections():
    j = np.arange(64, dtype=np.float64)
    nan = np.nan
    rows = [-(j - 20.0) ** 2, np.ones(64), np.full(64, nan), np.full(64, -np.inf)]
    r = np.full(64, nan); r[40] = -5.0; rows.append(r)                                   # one number among NaNs
    r = np.zeros(64); r[3] = nan; r[7] = r[50] = 2.0; rows.append(r)                    # two equal maxima: the smaller j
    r = np.full(64, -1.0); r[5] = -0.0; r[10] = 0.0; rows.append(r)                     # -0.0 == +0.0 as numbers
    r = np.full(64, -np.inf); r[0] = nan; rows.append(r)                                # a true -inf beats the NaN in front of it
    r = -(j - 63.0) ** 2; rows.append(r)                                                # the last lane
    r = -(j - 0.0) ** 2; rows.append(r)                                                 # the first lane
    rng = np.random.default_rng(6)
    for _ in range(100):
        r = np.round(rng.normal(size=64), 1)                                             # many ties
        r[rng.random(64) < 0.2] = nan
        rows.append(r)
    return np.array(rows)


def test_selection_is_the_references_and_the_butterfly_agrees(program):
    g = selections()
    got = program(["S " + " ".join(hx(v) for v in row) for row in g])
    want = ref.select(g)
    for k, line in enumerate(got):
        j, left, right = (int(t) for t in line.split()[1:])
        assert (j, left, right) == (want[k], max(want[k] - 1, 0), min(want[k] + 1, 63)), (k, line)


def test_answers_and_statuses(program):
    nan = np.nan
    cases = [(0, 10.0, 4.0, 5.0, 1.0, (4.0, 5.0, 1.0, ref.SIZED)), (0, 10.0, 10.0, 12.0, 2.0, (10.0, 12.0, 2.0, ref.SIZED_AT_LIMIT)),
             (0, 10.0, 4.0, 4.0, 0.0, (0.0, 0.0, 0.0, ref.SIZED_NONE)), (0, 10.0, 4.0, 3.0, -1.0, (0.0, 0.0, 0.0, ref.SIZED_NONE)),
             (0, 10.0, 4.0, 4.0, -0.0, (0.0, 0.0, 0.0, ref.SIZED_NONE)), (0, 0.0, 0.0, 0.0, 0.0, (0.0, 0.0, 0.0, ref.SIZED_NONE)),
             (1, 10.0, 4.0, 5.0, 1.0, (nan, nan, nan, ref.SIZED_NAN)), (1, nan, nan, nan, nan, (nan, nan, nan, ref.SIZED_NAN))]
    got = program([f"A {a} {hx(m)} {hx(x)} {hx(y)} {hx(g)}" for a, m, x, y, g, _ in cases])
    for line, case in zip(got, cases):
        t = line.split()[1:]
        v, want = unhx(t[:3]), case[5]
        assert int(t[3]) == want[3], (line, case)
        if want[3] == ref.SIZED_NAN:
            assert np.all(np.isnan(v))
        else:
            np.testing.assert_array_equal(v.view(np.uint64), np.array(want[:3]).view(np.uint64))   # (NONE: three +0.0)
