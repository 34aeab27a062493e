"""The HIP-free parts of the path entries' host side -- csrc/stage_layout.h SwapPathStage (the one staging layout of
cfmm_swap_path / cfmm_swap_order and their exact-output forms), csrc/swap_fill.h (the UniV3 landing rule, the columns into launch
order and back), csrc/swap_path_waves.h and swap_order_waves.h (the planner and its two namings) and csrc/split_search.h (a parent's split search) -- driven by
tests/native/path_rig_host.cpp: a stand-alone program built with the address and undefined-behaviour sanitizers and run as a
program.  The search runs there over a closed-form quote (constant-product hops with a fee); its shares, costs, totals and
statuses are compared here, as 64-bit words, with tests/split_paths_ref.py and tests/split_paths_out_ref.py over the same
closed form in numpy."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_paths_out_ref import SPLIT_UNOBTAINABLE, split_paths_out_ref  # noqa: E402
from split_paths_ref import SPLIT_NAN, SPLIT_NONE, SPLIT_OK, split_paths_ref  # noqa: E402

# the market of tests/native/path_rig_host.cpp
FIRST = np.array([0, 1, 3, 6, 14, 22, 23], dtype=np.int64)      # K = 1, 2, 3, 8, 8, 1
AMOUNT = np.array([50.0, 0.0, 120.0, 400.0, 1.0e6, 10.0])
NAN_PATH, GAMMA = 4, np.float64(0.997)
hops_of = lambda p: 1 + p % 3
r_in = lambda p, k: 1000.0 + 37.0 * p + 11.0 * k
r_out = lambda p, k: 900.0 + 29.0 * p + 7.0 * k


def quote_forward(path, x):
    """every operation one rounded binary64 operation, in the program's order"""
    path, x = np.asarray(path), np.array(x, dtype=np.float64)
    for k in range(3):
        on = hops_of(path) > k
        g = GAMMA * x
        with np.errstate(invalid="ignore", divide="ignore"):
            y = (r_out(path, k) * g) / (r_in(path, k) + g)
        x = np.where(on, y, x)
    return np.where(path == NAN_PATH, np.nan, x)


def quote_inverse(path, y):
    path, y = np.asarray(path), np.array(y, dtype=np.float64)
    dead = np.zeros(y.shape, dtype=bool)
    for k in (2, 1, 0):
        on = (hops_of(path) > k) & ~dead
        dead |= on & ~(y < r_out(path, k))
        with np.errstate(invalid="ignore", divide="ignore"):
            t = ((r_in(path, k) * y) / (r_out(path, k) - y)) / GAMMA
        y = np.where(on & ~dead, t, y)
    return np.where(path == NAN_PATH, np.nan, np.where(dead, np.inf, y))


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("path_rig_host") / "path_rig_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "path_rig_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stderr == ""
    return r.stdout


def test_layout_landing_rule_and_launch_order_under_the_sanitizers(program_output):
    assert "FAILED" not in program_output and program_output.rstrip().endswith("PATH_RIG_HOST_OK")


def words(v):
    v = np.asarray(v)
    return (v.astype(np.int64) if v.dtype.kind == "i" else v.astype(np.float64)).view(np.uint64)


@pytest.mark.parametrize("direction", ["in", "out"])
def test_the_search_equals_the_reference_word_for_word(program_output, direction):
    got = {}
    for line in program_output.splitlines():
        f = line.split()
        if f and f[0] == "SEARCH" and f[1] == direction:
            got[(int(f[2]), f[3])] = np.array([int(w, 16) for w in f[4:]], dtype=np.uint64)
    assert sorted(got) == sorted((r, a) for r in (1, 3, 5) for a in ("x", "y", "total", "status"))
    seen = set()
    for rounds in (1, 3, 5):
        if direction == "in":
            x, y, total, status = split_paths_ref(quote_forward, FIRST, AMOUNT, rounds=rounds)
        else:
            x, y, total, status = split_paths_out_ref(quote_inverse, FIRST, AMOUNT, rounds=rounds)
        assert status.size == 6 and x.size == y.size == 23
        for name, want in (("x", x), ("y", y), ("total", total), ("status", status)):
            np.testing.assert_array_equal(got[(rounds, name)], words(want), err_msg=f"{direction} rounds {rounds} {name}")
        seen |= set(status.tolist())
        # the cases the comparison is about are there
        assert status[1] == SPLIT_NONE and status[2] == SPLIT_NAN and status[0] == SPLIT_OK
        assert np.isnan(total[2]) and total[1] == 0.0 and total[0] > 0
        if direction == "out":
            assert status[4] == SPLIT_UNOBTAINABLE and np.isinf(total[4]) and status[3] == SPLIT_OK
    assert {SPLIT_OK, SPLIT_NONE, SPLIT_NAN} <= seen
