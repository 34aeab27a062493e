"""The numpy closed form of tests/solidly_ref.py against the 60-digit truth of tests/golden/solidly_precise.npz: the
YARDSTICK of the device test (tests/test_gpu_solidly_precise.py), whose per-class K is the next power of two >= 2× the
worst ratio shown here, capped at 16 on well / gamma1 / band and 64 elsewhere.  Also the fixture's own consistency (the
truth meets the optimality predicate; the independent bisection solver agrees with it).  No GPU.

Bound (derivation in tests/solidly_precise_ref.py), u = 2⁻⁵³, κ = 4, x′* / y′* the exact new reserves:
    |Δ − Δ*| <= K·u·(κ·(x′* + r_a)/γ + cΔ),   |Λ − Λ*| <= K·u·(κ·(y′* + r_b) + cΛ).

Worst ratio of the numpy reference per class (printed with -s), and the K that follows:
    well 0.36 -> 1   balanced 0.29 -> 1   band_edge 0.32 -> 1   band 0 -> 1   gamma1 0.34 -> 1   low_gamma 0.46 -> 1
    wide 0.62 -> 2   range 0.47 -> 1   drain 0.62 -> 2
"""
import numpy as np

import solidly_precise_ref as P
import solidly_ref as sr

C, CLS = P.load()
CAP = {"well": 16, "gamma1": 16, "band": 16}
# recorded from this test (the numpy reference, float64, any host): the device test derives its K from these
REF_RATIO = {"well": 0.36, "balanced": 0.29, "band_edge": 0.32, "band": 0.0, "gamma1": 0.34, "low_gamma": 0.46, "wide": 0.62,
             "range": 0.47, "drain": 0.62}
K = {name: P.k_of(r, CAP.get(name, 64)) for name, r in REF_RATIO.items()}


def _local_v():
    return C["v"][C["Ai"] - 1]


def test_fixture_shape_and_classes():
    m = len(C["gamma"])
    assert 10_000 <= m <= 20_000 and set(CLS) == set(REF_RATIO)
    assert C["R"].shape == (m, 2) and C["D"].shape == (m, 2) and C["cL"].shape == (m, 2)
    for k, name in enumerate(CLS):
        assert np.count_nonzero(C["cls"] == k) >= 1000, name
    assert np.all(C["D"] >= 0) and np.all(C["L"] >= 0)
    assert np.all((C["D"] > 0).sum(axis=1) <= 1)
    band = C["cls"] == CLS.index("band")
    assert not C["D"][band].any() and not C["L"][band].any() and np.all(C["gamma"][band] < 1)
    bal = C["cls"] == CLS.index("balanced")
    assert np.count_nonzero(C["R"][bal, 0] == C["R"][bal, 1]) >= np.count_nonzero(bal) // 2
    assert np.all(np.abs(C["R"][bal, 1] / C["R"][bal, 0] - 1) <= 1e-9)
    assert np.all(C["gamma"][C["cls"] == CLS.index("gamma1")] == 1.0)
    lg = C["gamma"][C["cls"] == CLS.index("low_gamma")]
    assert lg.min() >= 0.5 and lg.max() <= 0.9
    rg = C["R"][C["cls"] == CLS.index("range")]
    assert rg.min() < 2.0 ** -149 and rg.max() >= 2.0 ** 149 and rg.min() >= 2.0 ** -150 and rg.max() < 2.0 ** 151
    wd = C["cls"] == CLS.index("wide")
    assert np.max(np.abs(np.log(C["R"][wd, 1] / C["R"][wd, 0]))) > 35
    dr = C["cls"] == CLS.index("drain")
    rb = np.where(C["dir"] == 1, C["R"][:, 1], C["R"][:, 0])
    assert np.all((rb - C["L"].max(axis=1))[dr] < 1e-12 * rb[dr])


def test_numpy_closed_form_against_the_truth():
    D, L = sr.solve(C["R"], C["gamma"], _local_v())
    bD, bL = P.scale(C)
    r = P.ratios(D, L, C["D"], C["L"], bD, bL)
    worst = P.class_max(r, C["cls"], CLS)
    print("\nnumpy closed form, worst ratio |err| / (u·scale) per class: " + "  ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    print("K per class: " + "  ".join(f"{k}={v:g}" for k, v in K.items()))
    for name, w in worst.items():
        assert w <= 1.05 * REF_RATIO[name] + 0.02, (name, w)       # the recorded figures still describe the reference
        assert w <= K[name], (name, w)
    band = C["cls"] == CLS.index("band")
    assert not D[band].any() and not L[band].any() and not np.signbit(D[band]).any() and not np.signbit(L[band]).any()


def test_truth_meets_the_optimality_predicate():
    v = _local_v()
    for i in range(0, len(C["gamma"]), 7):
        R = C["R"][i]
        if C["cls"][i] in (CLS.index("range"), CLS.index("wide"), CLS.index("drain")):
            continue       # (φ of degree 4 overflows float64 at the ends of the upload range; drained pools: below)
        assert sr.optimality_ok(v[i], C["D"][i], C["L"][i], R, C["gamma"][i]), (i, CLS[C["cls"][i]])


def test_bisection_solver_agrees_with_the_truth():
    """The float64 bisection of tests/solidly_ref.py, which shares no formula with the generator's closed-form check: on
    the well-conditioned classes, at 1e-11 of the larger reserve (its own stopping accuracy near balance)."""
    sel = np.isin(C["cls"], [CLS.index(n) for n in ("well", "gamma1", "low_gamma")])
    R, g, v = C["R"][sel], C["gamma"][sel], _local_v()[sel]
    Db, Lb = sr.solve_bisect(R, g, v)
    sc = R.max(axis=1, keepdims=True)
    assert np.max(np.abs(Db - C["D"][sel]) / sc) <= 1e-11 and np.max(np.abs(Lb - C["L"][sel]) / sc) <= 1e-11
