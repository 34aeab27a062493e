"""The 60-digit fixture tests/golden/precise.npz on the CPU: its truth re-derived at 80 digits, and the two CPU
references the GPU suite leans on (the C oracle for GeometricMeanTwoCoin, tests/weighted_ref.py for weighted pools)
held to the scale-aware bounds of tests/precise_ref.py.  The device paths are held to the same bounds in
tests/test_gpu_precise.py."""
import importlib.util
import os

import numpy as np
import pytest

import cfmmrouter_amd as cr
import precise_ref as P
import weighted_ref as wr
from helpers import oracle_sweep

GC, WC, GCLS, WCLS = P.load()

K_ORACLE = 4      # glibc pow in the reference's operation order: at most 1.8 observed
K_WREF = 16       # bisection on t to 4·eps·|t|: at most 8.8 observed (ties)


def _generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_precise_golden.py")
    spec = importlib.util.spec_from_file_location("make_precise_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_shape():
    assert os.path.getsize(P.PATH) <= 1 << 20
    assert sum(len(c["gamma"]) for c in GC.values()) >= 6000
    for name, c in WC.items():
        N = int(name.split("_")[1])
        assert c["R"].shape[1] == N and len(c["gamma"]) >= 300
        assert set(np.unique(c["cls"])) == set(range(len(WCLS)))
        band = c["cls"] == WCLS.index("band")
        assert np.all(c["D"][band] == 0) and np.all(c["L"][band] == 0)
        trades = np.any(c["D"] > 0, axis=1) & np.any(c["L"] > 0, axis=1)
        assert np.count_nonzero(trades[~band]) >= 0.8 * np.count_nonzero(~band)
    well = GC["g_well"]
    both = well["cls"] == GCLS.index("both_live")
    assert np.count_nonzero(np.all(well["D"][both] > 0, axis=1)) >= 300        # most γ > 1 pools trade both ways
    assert "v2" in well and "v2" in WC["w_3"]


def _sample(cases, rng, count):
    rows = [(name, i) for name, c in sorted(cases.items()) for i in range(len(c["gamma"]))]
    return [rows[j] for j in rng.choice(len(rows), count, replace=False)]


def test_truth_rederived_at_80_digits_is_bit_equal():
    """256 seeded rows per family: the stored float64 truth is the 80-digit value rounded once."""
    mp = pytest.importorskip("mpmath")
    gen = _generator()
    rng = np.random.default_rng(80)
    with mp.workdps(80):
        for name, i in _sample(GC, rng, 256):
            c = GC[name]
            d1, d2, l1, l2 = gen.geo_truth(c["R"][i], c["w"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
            got = [gen._f(x) for x in (d1, d2, l1, l2)]
            assert got == [c["D"][i, 0], c["D"][i, 1], c["L"][i, 0], c["L"][i, 1]], (name, i)
        for name, i in _sample(WC, rng, 256):
            c = WC[name]
            D, L = gen.weighted_truth(c["R"][i], c["w"][i], c["gamma"][i], c["v"][c["Ai"][i] - 1])
            assert [gen._f(x) for x in D] == list(c["D"][i]) and [gen._f(x) for x in L] == list(c["L"][i]), (name, i)


@pytest.mark.parametrize("name", sorted(GC))
def test_oracle_meets_the_two_coin_bound(name):
    """The C oracle (src/cfmms.jl:180-196 with glibc pow) within K_ORACLE·u·scale everywhere except where the reference's
    own powers leave float64; every pool it gets wrong is one of those, predicted from the inputs."""
    c = GC[name]
    b = cr.GeometricMeanTwoCoin.batch(c["R"], c["w"], c["gamma"], c["Ai"])
    with np.errstate(all="ignore"):
        D, L, _, _ = oracle_sweep([b], len(c["v"]), c["v"])
    vp = c["v"][c["Ai"] - 1]
    bD, bL = P.two_coin_scale(c["R"], c["w"], c["gamma"], vp, c["D"], c["L"])
    r = P.ratios(D, L, c["D"], c["L"], bD, bL)
    pred = P.pow_out_of_range(c["R"], c["w"], c["gamma"], vp)
    print(f"\n[oracle] {name}: max ratio by class (pow-range pools excluded) "
          f"{P.class_max(np.where(pred, 0.0, r), c['cls'], GCLS)}; {int(pred.sum())} predicted pow-range pools, "
          f"{int(np.count_nonzero(r[pred] > K_ORACLE))} of them off")
    assert np.all(r[~pred] <= K_ORACLE)
    assert np.all(pred[r > K_ORACLE])
    if name == "g_wide":
        overflow = c["cls"] == GCLS.index("overflow")
        assert np.count_nonzero(pred & overflow) >= 200 and np.count_nonzero(r[pred] > K_ORACLE) > 0


@pytest.mark.parametrize("name", sorted(WC))
def test_weighted_reference_meets_the_weighted_bound(name):
    c = WC[name]
    vl = c["v"][c["Ai"] - 1]
    D, L = wr.solve(c["R"], c["w"], c["gamma"], vl)
    bD, bL = P.weighted_scale(c["R"], c["w"], c["gamma"], vl, c["D"], c["L"])
    r = P.ratios(D, L, c["D"], c["L"], bD, bL)
    print(f"\n[weighted_ref] {name}: {P.class_max(r, c['cls'], WCLS)}")
    assert np.all(r <= K_WREF)
