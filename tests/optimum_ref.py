"""The optimum fixture (tests/golden/make_optimum_golden.py -> tests/golden/optimum_precise.npz): its loader, its market as the
device takes it, and the numpy quote of a path -- the restatements of tests/quote_precise_ref.py chained hop by hop.  No quote
arithmetic of its own, no device, no library.

The market is seven segments in the order of SEGMENTS; a hop is (segment, row, coin_in, coin_out) as cfmm_quote_path takes it
(tests/test_gpu_quote_path.py make_paths), the hop arrays are [paths, 8]."""
import os

import numpy as np

import quote_precise_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "optimum_precise.npz")
SEGMENTS = ("product", "geomean", "solidly", "univ3", "weighted3", "curve2", "curve3")
N_COINS = {"product": 2, "geomean": 2, "solidly": 2, "univ3": 2, "weighted3": 3, "curve2": 2, "curve3": 3}
H = 8
ROUNDS = (1, 2, 3, 5, 16)
HOP_KEYS = ("n_hops", "seg", "row", "ci", "co")
FLAT_MARGIN = 1.1           # the quadratic model of a flat stretch is exact to a relative O(stretch / x*): the tests hold that below 0.1


def load():
    z = np.load(FIXTURE, allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    assert tuple(str(s) for s in fx["segments"]) == SEGMENTS
    return fx


def segment(fx, name):
    return {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")}


def hops_of(fx, what):
    """(n_hops, seg, row, ci, co) of the sizing cases ("size") or of all the orders' paths ("split")"""
    return tuple(fx[f"{what}_{k}"] for k in HOP_KEYS)


def names(fx, key, cls):
    """class / kind names per case"""
    table = [str(s) for s in fx[key]]
    return np.array([table[c] for c in cls])


def upload(ctx, fx):
    """the market on a context: segment s is SEGMENTS[s]; tokens 0 .. n-1 (the path entries address pools, not tokens)"""
    for name in SEGMENTS:
        g = segment(fx, name)
        if name == "univ3":
            p = g["current_price"].size
            ctx.add_univ3(g["current_price"], g["pool_gamma"], np.tile(np.array([0, 1], dtype=np.int32), (p, 1)), g["tick_off"],
                          g["lower_ticks"], g["liquidity"])
            continue
        m, n = g["R"].shape
        Ai0 = np.tile(np.arange(n, dtype=np.int32), (m, 1))
        if name == "product":
            ctx.add_product(g["R"], g["gamma"], Ai0)
        elif name == "solidly":
            ctx.add_solidly(g["R"], g["gamma"], Ai0)
        elif name == "geomean":
            ctx.add_geomean(g["R"], g["w"], g["gamma"], Ai0)
        elif name == "weighted3":
            ctx.add_weighted(g["R"], g["w"], g["gamma"], Ai0)
        else:
            ctx.add_curve(g["R"], g["gamma"], Ai0, g["alpha"], g["beta"])


def quoter(fx, hops):
    """quote_path(path_index_array, amounts) -> amounts over the numpy restatements of quote_precise_ref, hop level by hop level"""
    n_hops, seg, row, ci, co = hops
    segs = [segment(fx, name) for name in SEGMENTS]
    u = segs[SEGMENTS.index("univ3")]
    preps = [P.univ3_prepare(*P.univ3_pool(u, p)[:3]) for p in range(u["current_price"].size)]

    def hop(name, g, r, i, o, a):
        if name == "univ3":
            return np.array([P.q_univ3(preps[rr], float(g["pool_gamma"][rr]), int(ii), float(aa)) for rr, ii, aa in zip(r, i, a)])
        Ri, Ro, gm = g["R"][r, i], g["R"][r, o], g["gamma"][r]
        if name == "product":
            return P.q_product(Ri, Ro, gm, a)
        if name == "solidly":
            return P.q_solidly(Ri, Ro, gm, a)
        if name in ("geomean", "weighted3"):
            return P.q_weighted(Ri, Ro, g["w"][r, i], g["w"][r, o], gm, a)
        return P.q_curve(Ri, Ro, P.sum_logs(g["R"][r]), g["alpha"][r], np.log(g["beta"][r]), gm, a)

    def quote_path(idx, x):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        y = np.array(x, dtype=np.float64).reshape(-1)
        with np.errstate(all="ignore"):
            for k in range(H):
                act = n_hops[idx] > k
                for s, name in enumerate(SEGMENTS):
                    q = np.flatnonzero(act & (seg[idx, k] == s))
                    if q.size:
                        p = idx[q]
                        y[q] = hop(name, segs[s], row[p, k], ci[p, k], co[p, k], y[q])
        return y
    return quote_path


# ---- the bounds (derived in tests/test_optimum_precise_cpu.py) --------------------------------------------------------------------
def s_ref_size(fx, rounds):
    """what the search reaches with exact quotes: g* − g_ref after `rounds` rounds (below 0: the rounding of the stored gain, taken as 0)"""
    return np.maximum(fx["size_g"] - fx["size_g_ref"][:, rounds - 1], 0.0)


def size_bound(fx, rounds):
    return s_ref_size(fx, rounds) + (128.0 * rounds + 1.0) * fx["size_e"]


def s_ref_split(fx, rounds):
    return np.maximum(fx["split_T"] - fx["split_T_ref"][:, rounds - 1], 0.0)


def split_bound(fx, rounds):
    K = np.diff(fx["split_first"])
    return s_ref_split(fx, rounds) + (63.0 * K * rounds + 1.0) * fx["split_e"]


def size_x_bound(fx, rounds):
    """|amount_in − x*| <= the final bracket + the stretch around x* that evaluations off by e cannot tell from x*.  Every
    round's winner has the largest EVALUATED gain, so the end of the next bracket nearest to x* is within 128e of the gain at
    the same end of the bracket before (the argument of the gain bound): after r rounds the bracket reaches to within a true
    gain of 128·r·e of g*, and the answer lies in it.  On a smooth optimum {gain >= g* − t} is x* ± √(2t/c), c = −gain″(x*)
    (size_curv), exact to a relative O(that stretch / x*): FLAT_MARGIN allows for it.  On a `plateau` the gain falls away from x*
    by at least size_slope per unit on either side: x* ± t/slope.  Other classes: inf (not asserted)."""
    cls = names(fx, "size_classes", fx["size_cls"])
    t = 128.0 * rounds * fx["size_e"]
    with np.errstate(all="ignore"):
        flat = np.where(cls == "interior", FLAT_MARGIN * np.sqrt(2.0 * t / fx["size_curv"]), np.where(cls == "plateau", t / fx["size_slope"], np.inf))
    return fx["size_max_in"] * (2.0 / 63.0) ** rounds + flat


def share_bound(fx, rounds):
    """|share − truth| <= the order's last slice + the stretch over which the total is flat to within what the total may fall
    short by (split_bound): with Σ d_k = 0 and equal marginals T* − T = ½ Σ_k c_k d_k² (+ terms >= 0 of empty and pinned paths),
    so |d_k| <= √(2·bound/c_k), c_k = −q_k″ at the share (split_curv; 0, hence inf here, for empty and pinned paths).  The last
    slice is rem/63 with rem <= A·(K/63)^(rounds−1): tests/test_split_paths_cpu.py, the remainder is at most K slices a round."""
    K = np.diff(fx["split_first"])
    order_of = np.repeat(np.arange(K.size), K)
    slice_ = (fx["split_A"] * (K / 63.0) ** (rounds - 1) / 63.0)[order_of]
    with np.errstate(all="ignore"):
        flat = np.where(fx["split_curv"] > 0, FLAT_MARGIN * np.sqrt(2.0 * split_bound(fx, rounds)[order_of] / fx["split_curv"]), np.inf)
    return slice_ + flat


def worst_by(names_, values):
    return {str(c): float(np.max(values[names_ == c])) for c in np.unique(names_)}


def resolution_table(fx):
    """lines: per class and round the worst and the median relative shortfall of the search over exact quotes"""
    lines = []
    for what, cls, s_of, opt in (("size_path", names(fx, "size_classes", fx["size_cls"]), s_ref_size, fx["size_g"]),
                                 ("split_paths", names(fx, "order_kinds", fx["split_kind"]), s_ref_split, fx["split_T"])):
        for c in sorted(set(cls)):
            sel = cls == c
            for r in ROUNDS:
                rel = s_of(fx, r)[sel] / opt[sel]
                lines.append(f"{what:12s} {c:14s} rounds {r:2d}: {int(sel.sum()):3d} cases, shortfall / optimum worst {rel.max():.3g} median {np.median(rel):.3g}")
    return lines


if __name__ == "__main__":
    print("\n".join(resolution_table(load())))
