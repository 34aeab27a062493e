"""cfmm_quote_rate / cfmm_quote_path_rate without a device: the path contract in numpy (tests/rate_path_ref.py: the left-fold
product, NaN slots, the zero-rate hop, the poison rule), the header (valid C11, its declarations absent from cfmm_amd.h), the
plain C client's build, and the host-side pieces of the Python layer that need no context."""
import os
import subprocess

import numpy as np

import quote_precise_ref as P
import rate_path_ref as RPATH
import rate_precise_ref as RP
from test_julia_binding_swap_out_static import declarations, read

ROOT = P.ROOT


def product_hop(R, g):
    """hop(p, k, x) over per-hop reserve pairs R[k] = (R_in, R_out) and fees g[k], with the forms of the restatements"""
    return lambda p, k, x: (P.q_product(R[k][0], R[k][1], g[k], x), RP.r_product(R[k][0], R[k][1], g[k], x))


def test_fold_is_the_left_fold_each_product_rounded():
    r = np.array([[0.1, 0.3, 0.7], [1.0 / 3.0, 3.0, 0.9], [0.7, 1e-3, np.nan]])        # [max_hops, count]
    n_hops = np.array([3, 3, 2])
    rate = RPATH.fold_rates(n_hops, r)
    assert rate[0] == (0.1 * (1.0 / 3.0)) * 0.7 and rate[1] == (0.3 * 3.0) * 1e-3 and rate[2] == 0.7 * 0.9
    assert np.isnan(RPATH.fold_rates(np.array([0, 4]), r[:, :2])).all()                 # n_hops outside 1 .. max_hops


def test_walk_chains_amounts_and_rates_and_fills_unused_slots_with_nan():
    R, g = [(1e6, 2e6), (3e6, 1e6), (5e5, 5e5)], [0.997, 0.999, 1.0]
    out, rate, hop_out, hop_rate = RPATH.walk(np.array([3, 1, 2]), 3, np.array([1e3, 0.0, 5e4]), product_hop(R, g))
    x1 = P.q_product(*R[0], g[0], 1e3)
    x2 = P.q_product(*R[1], g[1], x1)
    x3 = P.q_product(*R[2], g[2], x2)
    assert out[0] == x3 and list(hop_out[:, 0]) == [x1, x2, x3]
    r = [RP.r_product(*R[0], g[0], 1e3), RP.r_product(*R[1], g[1], x1), RP.r_product(*R[2], g[2], x2)]
    assert list(hop_rate[:, 0]) == r and rate[0] == (r[0] * r[1]) * r[2]
    # amount 0: +0.0 out, the spot rate; one hop: the rate is the hop's, the other slots NaN
    assert out[1] == 0.0 and rate[1] == g[0] * ((1e6 / 1e6) * (2e6 / 1e6)) and np.isnan(hop_out[1:, 1]).all() and np.isnan(hop_rate[1:, 1]).all()
    assert np.isnan(hop_out[2, 2]) and np.isnan(hop_rate[2, 2]) and np.isfinite(rate[2])
    np.testing.assert_array_equal(rate, RPATH.fold_rates(np.array([3, 1, 2]), hop_rate))
    # the chain rule against a central difference of the walk itself (coarse: doubles)
    e = 1e-6
    up = RPATH.walk(np.array([3]), 3, np.array([1e3 * (1 + e)]), product_hop(R, g))[0][0]
    dn = RPATH.walk(np.array([3]), 3, np.array([1e3 * (1 - e)]), product_hop(R, g))[0][0]
    assert abs((up - dn) / (2e3 * e) - rate[0]) <= 1e-6 * rate[0]


def test_a_zero_rate_hop_zeroes_the_path_and_later_hops_are_still_evaluated():
    R, g = [(1e6, 2e6), None, (5e5, 5e5)], [0.997, None, 1.0]
    inner = product_hop(R, g)
    hop = lambda p, k, x: (123.0, 0.0) if k == 1 else inner(p, k, x)                    # an exhausted ladder: what it had, rate 0
    out, rate, hop_out, hop_rate = RPATH.walk(np.array([3]), 3, np.array([10.0]), hop)
    assert rate[0] == 0.0 and not np.signbit(rate[0]) and hop_rate[1, 0] == 0.0
    assert hop_out[2, 0] == P.q_product(5e5, 5e5, 1.0, 123.0) == out[0] and hop_rate[2, 0] == RP.r_product(5e5, 5e5, 1.0, 123.0)


def test_a_refused_hop_poisons_amount_and_rate_from_there_on():
    R, g = [(1e6, 2e6)] * 3, [0.997] * 3
    inner = product_hop(R, g)
    hop = lambda p, k, x: None if (p == 1 and k == 1) else inner(p, k, x)
    out, rate, hop_out, hop_rate = RPATH.walk(np.array([3, 3, 5]), 3, np.array([1.0, 1.0, 1.0]), hop)
    assert np.isfinite([out[0], rate[0]]).all()
    assert np.isfinite(hop_out[0, 1]) and np.isnan(hop_out[1:, 1]).all() and np.isnan(hop_rate[1:, 1]).all() and np.isnan([out[1], rate[1]]).all()
    assert np.isnan([out[2], rate[2]]).all() and np.isnan(hop_out[:, 2]).all()          # n_hops 5 > max_hops 3: nothing evaluated


def test_header_is_c11_and_lives_beside_the_main_header(tmp_path):
    h = declarations(read("include", "cfmm_amd_rate.h"))
    assert set(h) == {"cfmm_quote_rate", "cfmm_quote_rate_dev", "cfmm_quote_path_rate", "cfmm_quote_path_rate_dev"}
    assert not set(h) & set(declarations(read("include", "cfmm_amd.h")))
    assert '#include "cfmm_amd.h"' in read("include", "cfmm_amd_rate.h")
    src = tmp_path / "use.c"
    src.write_text('#include "cfmm_amd_rate.h"\nint (*p1)(cfmm_ctx*, int32_t, int64_t, const int64_t*, const int32_t*, const int32_t*, '
                   'const double*, double*, double*) = cfmm_quote_rate;\nint main(void) { return p1 == 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_four_entries():
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cfmmrouter.jl_amd", "libcfmm_amd.so")],
                       capture_output=True, text=True, check=True)
    names = {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}
    assert {"cfmm_quote_rate", "cfmm_quote_rate_dev", "cfmm_quote_path_rate", "cfmm_quote_path_rate_dev"} <= names


def test_price_impact_formula():
    from cfmmrouter_amd import router
    amt, out, spot = np.array([0.0, 10.0, 10.0, 5.0]), np.array([0.0, 9.0, 0.0, 5.0]), np.array([2.0, 1.0, 0.0, 1.0])
    imp = router._impact(amt, out, spot)
    assert imp[0] == 0.0 and imp[1] == 1.0 - 9.0 / (10.0 * 1.0) and np.isnan(imp[2]) and imp[3] == 0.0
    import cfmmrouter_amd as pkg
    for name in ("quote_rate", "spot_price", "price_impact", "quote_path_rate", "path_price_impact"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
