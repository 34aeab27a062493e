"""cfmm_swap on the device against the 80-digit sequences of tests/golden/swap_precise.npz: every sequence is one pool of a
segment, every step of every sequence goes through ONE ctx.swap call per family (step j of all sequences, then step j + 1:
the rows repeat, so the call runs one wave per step), on a single context and on a multi-device parent (device=[0, 0]).
Every step's answer and the state the sequence leaves are held to tests/swap_precise_ref.py's bounds at the K the host build
of csrc/swap_pool.h measured (tests/test_swap_precise_cpu.py).  Run with -s for the worst ratio per class; the measured
figures are recorded in profiles/swap_gpu_tests.log."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as Q
import swap_precise_ref as S

pytestmark = pytest.mark.gpu

FX = S.load()


def batch_of(name, g):
    fam = Q.family(name)
    m = len(g["cls"])
    if fam == "univ3":
        Ai = np.tile([1, 2], (m, 1))
        return cr.UniV3.batch(g["cp"], g["tick_off"], g["lower_ticks"], g["liquidity"], g["gamma"], Ai)
    n = g["R0"].shape[1]
    Ai = np.tile(np.arange(1, n + 1), (m, 1))
    if fam == "product":
        return cr.ProductTwoCoin.batch(g["R0"], g["gamma"], Ai)
    if fam == "solidly":
        return cr.SolidlyStableTwoCoin.batch(g["R0"], g["gamma"], Ai)
    if fam == "geomean":
        return cr.GeometricMeanTwoCoin.batch(g["R0"], g["w"], g["gamma"], Ai)
    if fam == "weighted":
        return cr.GeometricMean.batch(g["R0"], g["w"], g["gamma"], Ai)
    return cr.Curve.batch(g["R0"], g["gamma"], Ai, g["alpha"], g["beta"])


def run_group(name, device):
    """-> run(name, g, s) for swap_precise_ref.worst_by_class: the device's answers and final state of sequence s"""
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
        out = be.ctx.swap(0, g["a"][rows, steps], g["cin"][rows, steps], None if u3 else g["cout"][rows, steps], rows)
        assert be.ctx.get_option("swap_refused") == 0
        final = be.ctx.prices(0, m) if u3 else be.ctx.reserves(0, m, g["R0"].shape[1])
    finally:
        be.close()
    table = np.full((m, 4), np.nan)
    table[rows, steps] = out
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
