"""Do the contracts' searches reach the optimum?  tests/size_path_ref.py and tests/split_paths_ref.py (the numpy statements of
cfmm_size_path and cfmm_split_paths) over the numpy quotes of tests/quote_precise_ref.py, chained by tests/optimum_ref.py, against
the 80-digit optima of tests/golden/optimum_precise.npz (tests/golden/make_optimum_golden.py): every pool family alone and mixed,
1 .. 8 hops, optima on UniV3 tick boundaries and list ends, Solidly cycles far below the reserves' rounding, orders of 1 .. 8
paths.  No device.  Run with -s for the worst case per class (profiles/optimum_precise.txt).

Per case the fixture holds the optimum (g*, x* / T*, shares), a noise bound e of the quotes the search is given (the pinned bound
K·u·(R_o + out + cond) of every hop carried through the later hops' exact rates, plus the roundings of the gain / of the total) and
s_ref: what THE SAME search reaches when it is given exact quotes rounded once to double (optimum_ref.s_ref_size / s_ref_split;
the table in profiles/optimum_precise.txt).

SIZING.  gain is concave and its evaluations are off by at most e.  A round that picks a bracket without the maximiser took a
point whose evaluated gain was the largest; concavity then bounds the true slope beyond the bracket by 2e per grid step, the
maximiser is at most 63 steps away, and the winner itself is within 2e: such a round loses at most 2e·63 + 2e = 128e.  Hence
    g* − g  <=  s_ref + 128·rounds·e + e              (the last e: the reported gain against the true one at its own amount_in).

SPLITTING.  Σ_k q_k(x_k) over a grid is separable and concave, so for an allocation n of t slices and a best one n° of t + 1 there
is a path k with n_k < n°_k and V(n + e_k) + V(n° − e_k) >= V(n) + V(n°): the best increment from n is at least OPT_{t+1} − OPT_t.
A greedy step that compares increments each off by 2e_k takes one that is at most 2(e_k + e_k') <= 2e below the best (e = Σ_k e_k),
so the deficiency against the grid's optimum grows by at most 2e per step, 63 steps a round: 126e.  For two paths the one-slice
step back is a lower bound of the finer optimum, so rounds add up as they do for sizing: K·63·rounds·e with K = 2.  For K > 2
the documented stall (tests/test_split_paths_cpu.py) means a round can leave a restart point ABOVE the optimum and no such sum
can be derived; there the split is held to s_ref (exact quotes, the stall included) plus K·e per step taken:
    T* − T  <=  s_ref + 63·K·rounds·e + e             for every K.

THE CONDITION ON THE INPUTS, on the fixture alone: 128·16·e <= 1e-3·g* on every sizing class but `solidly_small`, and
63·K·16·e <= 1e-3·T* on every order: the noise term cannot hide a shortfall of a thousandth.  `solidly_small` has e of the size
of g* (the quote ends in R_o − u·x′: one ulp of the reserve whatever the amount); it is held to the noise bound alone and what it
reaches is printed.
"""
import numpy as np
import pytest

import optimum_ref as O
from size_path_ref import SIZED, size_path_ref
from split_paths_ref import SPLIT_OK, SPLIT_SATURATED, split_paths_ref

ROUNDS = O.ROUNDS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fx():
    return O.load()


@pytest.fixture(scope="module")
def sized(fx):
    """{rounds: (amount_in, amount_out, gain, status)} of the numpy-quote search, computed once and left unchanged"""
    q = O.quoter(fx, O.hops_of(fx, "size"))
    return {r: size_path_ref(q, fx["size_max_in"], fx["size_vi"], fx["size_vo"], r) for r in ROUNDS}


@pytest.fixture(scope="module")
def split(fx):
    q = O.quoter(fx, O.hops_of(fx, "split"))
    return {r: split_paths_ref(q, fx["split_first"], fx["split_A"], r) for r in ROUNDS}


def size_cls(fx):
    return O.names(fx, "size_classes", fx["size_cls"])


def order_kind(fx):
    return O.names(fx, "order_kinds", fx["split_kind"])


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_what_the_issue_asks_for(fx):
    cls, n_hops, seg = size_cls(fx), fx["size_n_hops"], fx["size_seg"]
    count = {c: int(np.sum(cls == c)) for c in ("interior", "kink", "plateau", "solidly_small", "hops8")}
    print(f"sizing cases: {cls.size} {count}")
    assert all(v >= 6 for v in count.values()) and cls.size >= 100
    assert set(n_hops) == {1, 2, 3, 8}
    used = np.arange(O.H)[None, :] < n_hops[:, None]
    families = [set(seg[p, used[p]]) for p in range(cls.size)]
    assert {next(iter(f)) for f in families if len(f) == 1} == set(range(len(O.SEGMENTS)))     # every family alone
    assert sum(len(f) > 1 for f in families) >= 30
    assert np.all((fx["size_x"] > 0) & (fx["size_x"] < fx["size_max_in"]) & (fx["size_g"] > 0))
    small = cls == "solidly_small"
    Ri = fx["solidly_R"][fx["size_row"][small, 0], fx["size_ci"][small, 0]]
    assert np.all(fx["size_x"][small] < 1e-4 * Ri)
    K, kind = np.diff(fx["split_first"]), order_kind(fx)
    print(f"orders: {K.size}, K {dict(zip(*np.unique(K, return_counts=True)))}, kinds {dict(zip(*np.unique(kind, return_counts=True)))}")
    assert set(K) == {1, 2, 3, 4, 8} and K.size >= 55
    assert {"stall", "empty", "kink"} <= set(kind)
    share, first, A = fx["split_share"], fx["split_first"], fx["split_A"]
    for g in range(K.size):
        s = share[first[g]:first[g + 1]]
        assert abs(np.sum(s.astype(np.longdouble)) - A[g]) <= 4e-16 * A[g]
        rows = [(int(a), int(b)) for p in range(first[g], first[g + 1]) for a, b in
                zip(fx["split_seg"][p, :fx["split_n_hops"][p]], fx["split_row"][p, :fx["split_n_hops"][p]])]
        assert len(set(rows)) == len(rows)                                   # pool-disjoint
        if kind[g] == "stall":
            print(f"stall order {g}: K = {K[g]}, the largest share is {s.max() / A[g]:.3f} of A")
            assert K[g] == 8 and s.max() >= 0.5 * A[g] and np.all(s > 0)
        if kind[g] == "empty":
            assert np.sum(s == 0.0) >= 1


def test_the_noise_cannot_hide_a_thousandth(fx):
    cls = size_cls(fx)
    ratio = 128.0 * 16 * fx["size_e"] / fx["size_g"]
    print("sizing, 128·16·e / g* worst per class:", {c: f"{v:.3g}" for c, v in O.worst_by(cls, ratio).items()})
    assert np.all(ratio[cls != "solidly_small"] <= 1e-3)
    K = np.diff(fx["split_first"])
    ratio = 63.0 * K * 16 * fx["split_e"] / fx["split_T"]
    print("splitting, 63·K·16·e / T* worst per kind:", {c: f"{v:.3g}" for c, v in O.worst_by(order_kind(fx), ratio).items()})
    assert np.all(ratio <= 1e-3)


def test_the_resolution_table(fx):
    """the search's own shortfall with a noise-free quote, per class and round (profiles/optimum_precise.txt is this output)"""
    lines = O.resolution_table(fx)
    print("\n".join(lines))
    assert np.all(np.isfinite(fx["size_g_ref"])) and np.all(np.isfinite(fx["split_T_ref"]))
    assert np.all(fx["size_g_ref"] <= (fx["size_g"] + fx["size_e"])[:, None])        # the optimum is one: nothing beats it by more than noise
    assert np.all(fx["split_T_ref"] <= (fx["split_T"] + fx["split_e"])[:, None])


# ---- sizing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", ROUNDS)
def test_sizing_reaches_the_optimum_within_resolution_and_noise(fx, sized, rounds):
    x, y, g, st = sized[rounds]
    cls = size_cls(fx)
    short, bound = fx["size_g"] - g, O.size_bound(fx, rounds)
    for c in np.unique(cls):
        sel = cls == c
        w = np.argmax(short[sel] / bound[sel])
        print(f"size_path numpy rounds {rounds:2d} {c:14s}: worst (g* - g)/g* {np.max(short[sel] / fx['size_g'][sel]):.3g}, worst (g* - g)/bound "
              f"{(short[sel] / bound[sel])[w]:.3g} (case {np.flatnonzero(sel)[w]}), s_ref/g* there {(O.s_ref_size(fx, rounds)[sel] / fx['size_g'][sel])[w]:.3g}")
    assert np.all(short <= bound)
    assert np.all(st == SIZED)                                               # never SIZED_AT_LIMIT: max_in >= 1.25 x*


@pytest.mark.parametrize("rounds", ROUNDS)
def test_amount_in_is_within_the_bracket_of_the_optimum(fx, sized, rounds):
    """the maximiser lies in every bracket: |amount_in − x*| <= max_in·(2/63)^rounds on `interior`, and a `plateau` answers the
    smallest x that reaches the plateau's gain (x*: where the list ends) to within the bracket -- plus the stretch that noise e
    cannot tell from x*, derived in optimum_ref.size_x_bound (at 16 rounds the bracket is below an ulp and that stretch is all
    there is; up to 3 rounds the bracket is all there is).  Paths with a Solidly hop are exempt (gain only)."""
    x = sized[rounds][0]
    cls = size_cls(fx)
    used = np.arange(O.H)[None, :] < fx["size_n_hops"][:, None]
    solidly = np.array([np.any(fx["size_seg"][p, used[p]] == O.SEGMENTS.index("solidly")) for p in range(x.size)])
    width = fx["size_max_in"] * (2.0 / 63.0) ** rounds
    bound = O.size_x_bound(fx, rounds)
    off = np.abs(x - fx["size_x"])
    off_ref = np.abs(fx["size_x_ref"][:, rounds - 1] - fx["size_x"])
    for c in ("interior", "plateau"):
        sel = (cls == c) & ~solidly
        print(f"size_path numpy rounds {rounds:2d} {c:9s}: worst |amount_in - x*| / bracket {np.max(off[sel] / width[sel]):.3g} (the exact-quote search "
              f"{np.max(off_ref[sel] / width[sel]):.3g}), / bound {np.max(off[sel] / bound[sel]):.3g}, / x* {np.max(off[sel] / fx['size_x'][sel]):.3g}; "
              f"the noise stretch is at most {np.max((bound - width)[sel] / fx['size_x'][sel]):.3g} of x*")
        assert np.all((bound - width)[sel] <= 0.1 * fx["size_x"][sel])          # the quadratic model's range (optimum_ref.FLAT_MARGIN)
        assert np.all(off[sel] <= bound[sel])


# ---- splitting --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", ROUNDS)
def test_splitting_reaches_the_optimum_within_resolution_and_noise(fx, split, rounds):
    path_in, path_out, total, st = split[rounds]
    kind, K = order_kind(fx), np.diff(fx["split_first"])
    short, bound = fx["split_T"] - total, O.split_bound(fx, rounds)
    for c in np.unique(kind):
        sel = kind == c
        w = np.argmax(short[sel] / bound[sel])
        print(f"split_paths numpy rounds {rounds:2d} {c:8s}: worst (T* - T)/T* {np.max(short[sel] / fx['split_T'][sel]):.3g}, worst (T* - T)/bound "
              f"{(short[sel] / bound[sel])[w]:.3g} (order {np.flatnonzero(sel)[w]}, K = {K[sel][w]}), s_ref/T* there "
              f"{(O.s_ref_split(fx, rounds)[sel] / fx['split_T'][sel])[w]:.3g}")
    assert np.all(short <= bound)
    assert np.all((st == SPLIT_OK) | (st == SPLIT_SATURATED))


@pytest.mark.parametrize("rounds", ROUNDS)
def test_shares_sum_to_the_amount_and_an_empty_path_gets_plus_zero(fx, split, rounds):
    path_in = split[rounds][0]
    first, A, kind = fx["split_first"], fx["split_A"], order_kind(fx)
    order_of = np.repeat(np.arange(A.size), np.diff(first))
    sums = np.array([np.sum(path_in[first[g]:first[g + 1]].astype(np.longdouble)) for g in range(A.size)])
    err = np.abs(sums - A.astype(np.longdouble)).astype(np.float64) / A
    print(f"split_paths numpy rounds {rounds:2d}: worst |sum of shares - A| / A {err.max():.3g}")
    assert np.all(err <= 3e-16)
    # the path the optimum leaves empty: +0.0 through the default 5 rounds.  MEASURED AT 16 ROUNDS (order 50, K = 3): 3.4e-13 -- once
    # a slice is below the rounding of the quotes the increments are noise and the greedy hands the path a slice; its base was 0
    # through round 5, so what it holds is at most the remainder of round 6, A·(K/63)^5
    empty = (fx["split_share"] == 0.0) & (kind[order_of] == "empty")
    assert empty.sum() >= 2
    if rounds <= 5:
        assert not np.any(bits(path_in[empty]))
    else:
        print(f"split_paths numpy rounds {rounds:2d}: the empty paths hold {path_in[empty]}")
        assert np.all(path_in[empty] <= (A * (np.diff(first) / 63.0) ** 5)[order_of][empty])


@pytest.mark.parametrize("rounds", ROUNDS)
def test_shares_are_within_the_last_slice_where_the_search_resolves(fx, split, rounds):
    """where the exact-quote search reaches the optimum (s_ref < 1e-9·T*) every share with a curvature to speak of is within its
    order's last slice of the truth, plus the stretch over which the total is flat (optimum_ref.share_bound: the optimum is flat
    in the shares, √ε of the scale, as tests/test_split_paths_cpu.py says of its own)."""
    path_in = split[rounds][0]
    first, A = fx["split_first"], fx["split_A"]
    K = np.diff(first)
    order_of = np.repeat(np.arange(A.size), K)
    sel = (O.s_ref_split(fx, rounds) < 1e-9 * fx["split_T"])[order_of] & (fx["split_curv"] > 0)
    bound = O.share_bound(fx, rounds)
    off = np.abs(path_in - fx["split_share"])
    off_ref = np.abs(fx["split_share_ref"][:, rounds - 1] - fx["split_share"])
    if sel.any():
        print(f"split_paths numpy rounds {rounds:2d}: {int(sel.sum())} of {sel.size} shares asserted; worst |share - truth| / bound "
              f"{np.max(off[sel] / bound[sel]):.3g} (the exact-quote search {np.max(off_ref[sel] / bound[sel]):.3g}), / A {np.max(off[sel] / A[order_of][sel]):.3g}")
    assert rounds < 5 or sel.sum() >= sel.size // 2
    assert np.all(off[sel] <= bound[sel])
