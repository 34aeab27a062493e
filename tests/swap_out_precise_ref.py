"""Bounds for cfmm_swap_out: a module, not a test.  A swap's answer IS cfmm_quote_out's answer on the pool as it stands, so
the unit of one step is quote_out_precise_ref's unit for that quote, u·(R_i/γ + a* + cond); what is new is the error a step
CARRIES into the next one through the state it leaves -- accumulated as swap_precise_ref does it.

Carried error, reserve kinds.  A step leaves R_out' = fl(R_out − want): want is given, one rounding, relative error <= u; and
R_in' = fl(R_in + fl(γ·a)) with a off by at most K·unit: absolute error <= γ·K·unit + 2u·R_in'.  The next quote is a smooth
function of the state; to first order its answer moves by Σ_k |∂a/∂R_k|·E_k with E_k the absolute error of reserve k.  The
fixture stores the partials at the true state.

Carried error, UniV3.  The state is the price P = k/(s'·s') or (s'·s')/k with s' = s_in + γ·a clamped into the landing tick:
swap_precise_ref's 8u per step for the operations on prepared constants and the re-preparation, and -- new here -- the
answer's own error through s': 2·γ·(K·unit)/s' relative.  A step's answer carries ε·cond, as there.

Path independence.  With the fee on the input the state after swap_out(w₁) is R + γa₁e_in − w₁e_out and φ is conserved by
each swap, so EXACTLY in(w₁) + in_after(w₂) = quote_out(w₁ + w₂).  In doubles: two steps, the carried error, the addition of
the two answers, and the twin's own quote of w₁ + w₂.  path_tolerance below is that sum.

The fixture (tests/golden/make_swap_out_golden.py -> tests/golden/swap_out_precise.npz): sequences of 1-4 exact-output swaps on
one pool with the exact state carried between the steps at 80 digits; per step the truth of the amount to tender (the
smallest a with φ conserved, by bisection on φ itself) and of the state it leaves, and scale / cond / the partials |∂a/∂R_k| of
quote_out_precise_ref's bound AT THE TRUE STATE (UniV3: and s' of the landing tick).  The UniV3 group holds steps whose wanted
amount is a running ΣR_out of the prepared records bit for bit (`boundary`, `tick_edge`) and steps that exhaust the direction
a finite input exhausts (`exhausted`).

The unit of a step (sequence_units): u·(scale + a* + cond) plus the carried state error of the steps before at K = 1.  The
state a sequence leaves is held to the same accumulators: |R_k − R_k*| <= K·E_k, |P − P*| <= K·ε·P*.  The bound of a step is
K times its unit.

K per class follows quote_precise_ref's rule: the host build of csrc/swap_pool.h, quote_pool.h and univ3_pool.h
(tests/native/swap_out_host.cpp), never the GPU, is run over the fixture; K is the next power of two >= 2x its worst ratio in
the class, never above quote_precise_ref's caps (16 on `typical`, 64 elsewhere).  The measured worst ratios are K_MEASURED
(tests/test_swap_out_precise_cpu.py re-measures them); a class that needed more than its cap would mean the arithmetic is
wrong.  Outside the fixture a caller uses the exact-output quote table's family maximum (family_K)."""
import math
import os

import numpy as np

import quote_out_precise_ref as QO
import quote_precise_ref as Q

U = Q.U
K_CAP_TYPICAL, K_CAP = Q.K_CAP_TYPICAL, Q.K_CAP
UNIV3_CARRY = 8.0     # swap_precise_ref's
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "swap_out_precise.npz")
RESERVE_GROUPS = ("product", "geomean", "solidly", "weighted3", "weighted8", "curve3", "curve8")
GROUPS = RESERVE_GROUPS + ("univ3",)
KIND = {"product": 0, "geomean": 1, "weighted": 3, "curve": 4, "solidly": 5}

# worst ratio (error / unit) of the host build per (family, class), over answers and states; see K_of
K_MEASURED = {
    ('curve', 'balanced'): 0.779,
    ('curve', 'lopsided'): 0.6,
    ('curve', 'low_gamma'): 0.47,
    ('curve', 'typical'): 0.267,
    ('geomean', 'balanced'): 0.264,
    ('geomean', 'lopsided'): 0.232,
    ('geomean', 'low_gamma'): 0.286,
    ('geomean', 'typical'): 0.178,
    ('product', 'balanced'): 0.345,
    ('product', 'lopsided'): 0.181,
    ('product', 'low_gamma'): 0.447,
    ('product', 'typical'): 0.62,
    ('solidly', 'balanced'): 0.296,
    ('solidly', 'lopsided'): 0.381,
    ('solidly', 'low_gamma'): 0.0222,
    ('solidly', 'typical'): 0.735,
    ('univ3', 'boundary'): 0.0595,
    ('univ3', 'crosses'): 0.0129,
    ('univ3', 'empty_tick'): 0.0159,
    ('univ3', 'exhausted'): 0.092,
    ('univ3', 'one_tick'): 0.0334,
    ('univ3', 'reversal'): 0.118,
    ('univ3', 'tick_edge'): 0.00322,
    ('univ3', 'two_ticks'): 0.00348,
    ('weighted', 'balanced'): 0.55,
    ('weighted', 'lopsided'): 0.418,
    ('weighted', 'low_gamma'): 0.127,
    ('weighted', 'typical'): 0.363,
}


def K_of(group, cls):
    worst = K_MEASURED[(Q.family(group), cls)]
    k = Q.next_pow2(2.0 * worst)
    assert k <= (K_CAP_TYPICAL if cls == "typical" else K_CAP), (group, cls, worst)
    return k


def load():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def group(fx, g):
    return {k[len(g) + 1:]: v for k, v in fx.items() if k.startswith(g + "_")}


def sequence_units(g, s, univ3=False):
    """sequence s of group g -> (unit_in [steps], the accumulators after the last step: E [N] absolute per coin, or the
    relative price error ε), all at K = 1"""
    n = int(g["nsteps"][s])
    unit = np.zeros(n)
    if univ3:
        eps = 0.0
        for j in range(n):
            unit[j] = U * (g["scale"][s, j] + g["a"][s, j] + g["cond"][s, j]) + eps * g["cond"][s, j]
            if g["want"][s, j] != 0.0:
                eps += UNIV3_CARRY * U + 2.0 * g["gamma"][s] * unit[j] / g["sland"][s, j]
        return unit, eps
    E = np.zeros(g["R0"].shape[1])
    for j in range(n):
        ci, co = int(g["cin"][s, j]), int(g["cout"][s, j])
        unit[j] = U * (g["scale"][s, j] + g["a"][s, j] + g["cond"][s, j]) + float(np.sum(g["da"][s, j] * E))
        E[ci] += g["gamma"][s] * unit[j] + 2.0 * U * g["Rin"][s, j]
        E[co] += U * g["Rout"][s, j]
    return unit, E


def true_final_reserves(g, s):
    R = np.array(g["R0"][s], copy=True)
    for j in range(int(g["nsteps"][s])):
        R[int(g["cin"][s, j])], R[int(g["cout"][s, j])] = g["Rin"][s, j], g["Rout"][s, j]
    return R


def worst_by_class(fx, run):
    """run(group name, g, s) -> (amount_in [steps], final state: R [N] or the price) of the implementation under test
    -> {(family, class): worst ratio over every step's answer and the final state}"""
    worst = {}
    for name in GROUPS:
        g = group(fx, name)
        u3 = name == "univ3"
        for s in range(len(g["cls"])):
            n = int(g["nsteps"][s])
            a, final = run(name, g, s)
            unit, acc = sequence_units(g, s, u3)
            err = np.abs(np.asarray(a)[:n] - g["a"][s, :n])
            r = float(np.max(np.where(err == 0, 0.0, err / np.where(unit > 0, unit, 1e-300))))
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


def family_K(family):
    """the family's largest K in quote_out_precise_ref's table"""
    ks = [QO.K_of(family, c) for (f, c) in QO.K_MEASURED if f == family]
    assert ks and max(ks) <= K_CAP
    return max(ks)


def carried(K, unit1, gamma, Ri_after, Ro_after, da_dRi, da_dRo):
    """reserve kinds: what the state error step 1 leaves (answer within K·unit1, absolute) adds to step 2's answer;
    da_dRi, da_dRo = |∂a₂/∂R_in|, |∂a₂/∂R_out| at the state step 1 left"""
    return da_dRi * (gamma * K * unit1 + 2.0 * U * Ri_after) + da_dRo * U * Ro_after


def carried_univ3(K, unit1, gamma, s_land, cond2):
    return (UNIV3_CARRY * U + 2.0 * gamma * K * unit1 / s_land) * cond2


def path_tolerance(K, unit1, unit2, unit12, carry, in1, in2):
    """|in₁ + in₂ − quote_out(w₁ + w₂)| <= this; units absolute (u included)"""
    return K * (unit1 + unit2 + unit12) + carry + U * (in1 + in2)

