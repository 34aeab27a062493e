"""cfmm_swap_out on the device against the 80-digit sequences of tests/golden/swap_out_precise.npz: every sequence is one pool
of a segment, every step of every sequence goes through ONE ctx.swap_out call per family (step j of all sequences, then step
j + 1: the rows repeat, so the call runs one wave per step), on a single context and on a multi-device parent
(device=[0, 0]).  Every step's answer and the state the sequence leaves are held to tests/swap_out_precise_ref.py's bounds at
the K the host build of csrc/swap_pool.h measured (tests/test_swap_out_precise_cpu.py).  Run with -s for the worst ratio per
class."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import swap_out_precise_ref as S
from cfmmrouter_amd._lib import SWAP_APPLIED
from test_gpu_swap_precise import batch_of

pytestmark = pytest.mark.gpu

FX = S.load()


def run_group(name, device):
    """-> run(name, g, s) for swap_out_precise_ref.worst_by_class: the device's answers and final state of sequence s"""
    g = S.group(FX, name)
    u3 = name == "univ3"
    m = len(g["cls"])
    rows, steps = [], []
    for j in range(int(np.max(g["nsteps"]))):
        live = np.flatnonzero(g["nsteps"] > j)
        rows.append(live)
        steps.append(np.full(live.size, j))
    rows, steps = np.concatenate(rows), np.concatenate(steps)
    be = cr.DeviceBackend(8, [batch_of(name, g)], device=device)
    try:
        a, st = be.ctx.swap_out(0, g["want"][rows, steps], g["cin"][rows, steps], None if u3 else g["cout"][rows, steps], rows, status=True)
        assert np.all(st == SWAP_APPLIED) and be.ctx.get_option("swap_refused") == 0
        final = be.ctx.prices(0, m) if u3 else be.ctx.reserves(0, m, g["R0"].shape[1])
    finally:
        be.close()
    table = np.full((m, 4), np.nan)
    table[rows, steps] = a
    return table, final


@pytest.mark.parametrize("device", (0, [0, 0]), ids=("single", "multi"))
def test_every_step_and_the_final_state_within_the_bounds(device):
    got = {name: run_group(name, device) for name in S.GROUPS}
    worst = S.worst_by_class(FX, lambda name, g, s: (got[name][0][s], got[name][1][s]))
    for key in sorted(worst):
        K = S.K_of(*key)
        print(f"device {device} {key[0]}/{key[1]}: worst {worst[key]:.3g} of K = {K} (host build: {S.K_MEASURED[key]:.3g})")
    for key, w in worst.items():
        assert w <= S.K_of(*key), (key, w)
    assert set(worst) == set(S.K_MEASURED)
