"""Bounds for cfmm_swap: a module, not a test.  A swap's answer IS cfmm_quote's answer on the pool as it stands, so the unit
of one step is quote_precise_ref's unit for that quote, u·(R_o + out + cond); what is new is the error a step CARRIES into
the next one through the state it leaves.

Carried error, reserve kinds.  Step 1 leaves R_in' = fl(R_in + fl(γ·a)) -- two roundings, relative error <= 2u -- and
R_out' = fl(R_out − out₁) with out₁ off by at most K·unit₁: absolute error <= K·unit₁ + u·R_out'.  The next quote is a smooth
function of the state; to first order its answer moves by |R_in'·∂q/∂R_in|·2u + |∂q/∂R_out|·(K·unit₁ + u·R_out').  The first
factor is one term of the step's conditioning sum (<= cond₂), the second partial is computed by the caller (finite
differences on the numpy restatement) and never taken below 1.

Carried error, UniV3.  The state is the price P = k/(s'·s') or (s'·s')/k with s' = s_in + d_t: one addition, one product,
one division on prepared constants good to a few u each, so P is within 6u relative of the exact landing price, and the
constants re-prepared from it (roots of k/P, k·P, differences with the tick's α, β) move by 3u relative before their own
roundings.  quote_precise_ref.univ3_unit's conditioning sum is exactly the effect of a relative perturbation u of every
prepared constant, so the carried error is <= 8·u·cond₂ (6u from P, rounded up for the re-preparation's own operations).

Path independence.  With the fee on the input the state after swap(a₁) is R + γa₁e_in − out₁e_out, and φ is conserved by
each swap, so EXACTLY out(a₁) + out_after(a₂) = out(a₁ + a₂).  In doubles: two steps, the carried error, the addition of the
two answers (u·(out₁ + out₂)), and the twin's own quote of a₁ + a₂.  path_tolerance below is that sum.

The fixture (tests/golden/make_swap_golden.py -> tests/golden/swap_precise.npz): sequences of 1-4 swaps on one pool with the
exact state carried between the steps at 80 digits; per step the truth of the amount out and of the state it leaves, and
scale / cond / the partials |∂q/∂R_k| of quote_precise_ref's bound AT THE TRUE STATE.

The unit of a step (sequence_units): quote_precise_ref's unit u·(scale + out* + cond), plus the carried state error of the
steps before at K = 1.  Reserve kinds: an absolute error bound E_k per coin starts at 0; a step's answer carries
Σ_k |∂q/∂R_k|·E_k; afterwards E_in grows by 2u·R_in' and E_out by the step's own unit + u·R_out'.  UniV3: a relative price
error ε starts at 0 and grows by 8u per step (it passes into the next price with a factor <= 1: P' depends on P only through
s_in = √(k/P) or √(k·P) of the current tick), and a step's answer carries ε·cond.  The state a sequence leaves is held to
the same accumulators: |R_k − R_k*| <= K·E_k, |P − P*| <= K·ε·P*.  The bound of a step is K times its unit.

K per class follows quote_precise_ref's rule: the CPU restatement -- the host build of csrc/swap_pool.h, quote_pool.h and
univ3_pool.h (tests/native/swap_host.cpp), never the GPU -- is run over the fixture; K is the next power of two >= 2x its
worst ratio in the class, never above quote_precise_ref's cap (16 on `typical`, 64 elsewhere).  The measured worst ratios are
K_MEASURED (tests/test_swap_precise_cpu.py re-measures them); a class that needed more than the cap would mean the
arithmetic is wrong.  Outside the fixture a caller uses the quote table's family maximum (family_K)."""
import math
import os

import numpy as np

import quote_precise_ref as Q

U = Q.U
K_CAP = 64            # quote_precise_ref's cap outside `typical` (16 on `typical`); never raised here
UNIV3_CARRY = 8.0     # see above
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "swap_precise.npz")
RESERVE_GROUPS = ("product", "geomean", "solidly", "weighted3", "weighted8", "curve3", "curve8")
GROUPS = RESERVE_GROUPS + ("univ3",)
KIND = {"product": 0, "geomean": 1, "weighted": 3, "curve": 4, "solidly": 5}

# worst ratio (error / unit) of the host build of swap_pool.h per (family, class), over answers and states; see K_of
K_MEASURED = {
    ('curve', 'balanced'): 0.37,
    ('curve', 'lopsided'): 0.42,
    ('curve', 'low_gamma'): 0.344,
    ('curve', 'typical'): 0.398,
    ('geomean', 'balanced'): 0.338,
    ('geomean', 'lopsided'): 0.448,
    ('geomean', 'low_gamma'): 0.222,
    ('geomean', 'typical'): 0.284,
    ('product', 'balanced'): 0.265,
    ('product', 'lopsided'): 0.102,
    ('product', 'low_gamma'): 0.15,
    ('product', 'typical'): 0.295,
    ('solidly', 'balanced'): 2.35,
    ('solidly', 'lopsided'): 2.29,
    ('solidly', 'low_gamma'): 1.8,
    ('solidly', 'typical'): 2.47,
    ('univ3', 'crosses'): 0.178,
    ('univ3', 'empty_tick'): 0.041,
    ('univ3', 'exhausted'): 0.074,
    ('univ3', 'one_tick'): 0.126,
    ('univ3', 'reversal'): 0.243,
    ('univ3', 'tick_edge'): 0.0448,
    ('univ3', 'two_ticks'): 0.0818,
    ('weighted', 'balanced'): 0.384,
    ('weighted', 'lopsided'): 0.425,
    ('weighted', 'low_gamma'): 0.147,
    ('weighted', 'typical'): 0.331,
}


def K_of(group, cls):
    worst = K_MEASURED[(Q.family(group), cls)]
    k = Q.next_pow2(2.0 * worst)
    assert k <= (16 if cls == "typical" else K_CAP), (group, cls, worst)
    return k


def load():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def group(fx, g):
    return {k[len(g) + 1:]: v for k, v in fx.items() if k.startswith(g + "_")}


def sequence_units(g, s, univ3=False):
    """sequence s of group g -> (unit_out [steps], the accumulators after the last step: E [N] absolute per coin, or the
    relative price error ε), all at K = 1"""
    n = int(g["nsteps"][s])
    unit = np.zeros(n)
    if univ3:
        eps = 0.0
        for j in range(n):
            unit[j] = U * (g["scale"][s, j] + g["out"][s, j] + g["cond"][s, j]) + eps * g["cond"][s, j]
            if g["a"][s, j] != 0.0:
                eps += UNIV3_CARRY * U
        return unit, eps
    E = np.zeros(g["R0"].shape[1])
    for j in range(n):
        ci, co = int(g["cin"][s, j]), int(g["cout"][s, j])
        unit[j] = U * (g["scale"][s, j] + g["out"][s, j] + g["cond"][s, j]) + float(np.sum(g["dq"][s, j] * E))
        E[ci] += 2.0 * U * g["Rin"][s, j]
        E[co] += unit[j] + U * g["Rout"][s, j]
    return unit, E


def worst_by_class(fx, run):
    """run(group name, g, s) -> (out [steps], final state: R [N] or the price) of the implementation under test
    -> {(family, class): worst ratio over every step's answer and the final state}"""
    worst = {}
    for name in GROUPS:
        g = group(fx, name)
        u3 = name == "univ3"
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            out, final = run(name, g, s)
            unit, acc = sequence_units(g, s, u3)
            err = np.abs(np.asarray(out)[:n] - g["out"][s, :n])
            r = float(np.max(np.where(err == 0, 0.0, err / np.where(unit > 0, unit, 1e-300))))      # (no liquidity left: 0 == 0)
            if u3:
                if acc > 0:
                    r = max(r, abs(final - g["price"][s, n - 1]) / (acc * g["price"][s, n - 1]))
            else:
                Rt = true_final_reserves(g, s)
                ok = acc > 0
                r = max(r, float(np.max(np.abs(np.asarray(final)[ok] - Rt[ok]) / acc[ok])))
                assert np.array_equal(np.asarray(final)[~ok], Rt[~ok])      # coins no step touched keep every bit
            if not math.isfinite(r):
                r = math.inf
            key = (Q.family(name), str(g["cls"][s]))
            worst[key] = max(worst.get(key, 0.0), r)
    return worst


def true_final_reserves(g, s):
    R = np.array(g["R0"][s], copy=True)
    for j in range(int(g["nsteps"][s])):
        R[int(g["cin"][s, j])], R[int(g["cout"][s, j])] = g["Rin"][s, j], g["Rout"][s, j]
    return R


def family_K(family):
    """the family's largest K in quote_precise_ref's table"""
    ks = [Q.K_of(family, c) for (f, c) in Q.K_MEASURED if f == family]
    assert ks and max(ks) <= K_CAP
    return max(ks)


def carried(K, unit1, cond2, dq_dRo, Ro_after):
    """reserve kinds: what the state error step 1 leaves (answer within K·unit1) adds to step 2's answer; unit1 in absolute
    terms (u included), cond2 the second step's conditioning sum, dq_dRo = |∂q₂/∂R_out|"""
    return 2.0 * U * cond2 + np.maximum(1.0, dq_dRo) * (K * unit1 + U * Ro_after)


def carried_univ3(cond2):
    return UNIV3_CARRY * U * cond2


def path_tolerance(K, unit1, unit2, unit12, carry, out1, out2):
    """|out₁ + out₂ − quote(a₁ + a₂)| <= this; units absolute (u included)"""
    return K * (unit1 + unit2 + unit12) + carry + U * (out1 + out2)
