"""cfmm_quote_to_rate / cfmm_swap_limit without a device: the header (valid C11 and C++17, its declarations absent from the
other headers, the status values), the exported symbols, the waves a batch of limited swaps is cut into (swap_waves.h, run
through tests/native/swap_host.cpp's build of it: the entry takes cfmm_swap's plan unchanged), and the pieces of the Python layer
that need no context."""
import os
import subprocess

import numpy as np
import pytest

import quote_precise_ref as P
from test_julia_binding_swap_out_static import declarations, read
from test_swap_precise_cpu import host, waves_of  # noqa: F401  (the host build of swap_waves.h, tests/native/swap_host.cpp)

ROOT = P.ROOT
ENTRIES = {"cfmm_quote_to_rate", "cfmm_quote_to_rate_dev", "cfmm_swap_limit"}


def test_header_is_c11_and_lives_beside_the_rate_header(tmp_path):
    text = read("include", "cfmm_amd_limit.h")
    h = declarations(text)
    assert set(h) == ENTRIES
    for other in ("cfmm_amd.h", "cfmm_amd_rate.h"):
        assert not set(h) & set(declarations(read("include", other)))
    assert '#include "cfmm_amd_rate.h"' in text
    # cfmm_quote_rate's list (the limit where the amount stood); cfmm_swap's with the limit, the amount used and the status
    rate = declarations(read("include", "cfmm_amd_rate.h"))
    main = declarations(read("include", "cfmm_amd.h"))
    assert h["cfmm_quote_to_rate"][1] == rate["cfmm_quote_rate"][1] == h["cfmm_quote_to_rate_dev"][1]
    assert h["cfmm_swap_limit"][1] == main["cfmm_swap"][1][:-1] + ["double*", "double*", "double*", "int32_t*"]   # (the parser drops const)
    for name, value in (("FILLED", 0), ("PARTIAL", 1), ("NONE", 2), ("REFUSED", 3)):
        assert f"#define CFMM_LIMIT_{name}" in text and f"CFMM_LIMIT_{name} {value}".replace(" ", "") in text.replace(" ", "")
    src = tmp_path / "use.c"
    src.write_text('#include "cfmm_amd_limit.h"\n'
                   'int (*p1)(cfmm_ctx*, int32_t, int64_t, const int64_t*, const int32_t*, const int32_t*, const double*, double*, double*) = cfmm_quote_to_rate;\n'
                   'int (*p2)(cfmm_ctx*, int32_t, int64_t, const int64_t*, const int32_t*, const int32_t*, const double*, const double*, double*, '
                   'double*, int32_t*) = cfmm_swap_limit;\n'
                   'int main(void) { return (p1 == 0) + (p2 == 0) + CFMM_LIMIT_FILLED + (CFMM_LIMIT_REFUSED != 3); }\n')
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_library_exports_the_three_entries():
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cfmmrouter.jl_amd", "libcfmm_amd.so")],
                       capture_output=True, text=True, check=True)
    names = {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}
    assert ENTRIES <= names


def test_limited_swaps_take_cfmm_swaps_waves(host):
    """the entry is a direction of abi_swap.cpp's shared path: ONE swap_plan call serves the three, and the kernel is behind it;
    and that plan, built for the host, on the batches the GPU tests send: a row named k times makes k waves, each of distinct
    rows ascending, the caller's order kept per row; distinct rows and idx == NULL are one wave"""
    for idx, waves in (([3, 3, 3, 3], 4), ([0, 27, 14, 0, 27, 1, 0], 3), (list((np.arange(65) * 5) % 28), 3), ([9, 3, 4], 1)):
        nw, wave, perm, off = waves_of(host, idx)
        idx = np.asarray(idx)
        assert nw == waves == int(np.max(np.bincount(idx))) and off[0] == 0 and off[-1] == idx.size
        assert sorted(perm.tolist()) == list(range(idx.size))
        for w in range(nw):
            at = perm[off[w]:off[w + 1]]
            assert np.all(wave[at] == w) and np.all(np.diff(idx[at]) > 0)          # distinct rows, ascending: no two lanes on one pool
        for row in np.unique(idx):                                                 # the caller's order per row
            assert wave[idx == row].tolist() == list(range(int(np.sum(idx == row))))
    src = read("cfmmrouter.jl_amd", "csrc", "abi_swap.cpp")
    assert "kLimited{false, \"cfmm_swap_limit\", nullptr, \"amount_in\", true}" in src                # the direction is stated once, in Dir
    assert src.count("swap_plan(count, idx)") == 1 and "launch_swap_limit(" in src and 'extern "C" int cfmm_swap_limit(' in src
    kernels = read("cfmmrouter.jl_amd", "csrc", "swap_limit_kernels.h")
    for needle in ("to_rate_any<KIND>", "quote_one<KIND>", "swap_move<KIND>", "swap_store<KIND>", "swap_univ3_price("):
        assert needle in kernels, needle
    assert "kToRateCurveIters" in read("cfmmrouter.jl_amd", "csrc", "to_rate_pool.h")


def test_python_layer_without_a_context():
    import cfmmrouter_amd as pkg
    from cfmmrouter_amd import _lib
    for name in ("amount_to_rate", "swap_limit_", "LIMIT_FILLED", "LIMIT_PARTIAL", "LIMIT_NONE", "LIMIT_REFUSED"):
        assert hasattr(pkg, name) and name in pkg.__all__, name
    assert (pkg.LIMIT_FILLED, pkg.LIMIT_PARTIAL, pkg.LIMIT_NONE, pkg.LIMIT_REFUSED) == (0, 1, 2, 3)
    for verb in ("quote_to_rate", "quote_to_rate_dev", "swap_limit"):
        assert callable(getattr(_lib.Context, verb)), verb
    ci, co, ix = _lib.Context._query_columns(1, None, [3, 4, 5], 3)
    assert ci.tolist() == [1, 1, 1] and co is None and ix.dtype == np.int64
    with pytest.raises(pkg.ArgumentError, match="one entry per query"):
        _lib.Context._query_columns([0, 1], None, None, 3)
    with pytest.raises(pkg.ArgumentError, match="idx must have one entry per query"):
        _lib.Context._query_columns(0, None, [1, 2], 3)
