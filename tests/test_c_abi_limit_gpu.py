"""cfmm_quote_to_rate / cfmm_swap_limit used from plain C (no Python, no torch in the process): tests/c/abi_limit.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_limit")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_limit.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_limit_client_compiles(tmp_path):
    """CPU: the declarations of include/cfmm_amd_limit.h are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_limit_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_limit: ok" in r.stdout
    for name in ("product", "geomean", "univ3", "weighted", "curve", "solidly"):
        assert f"{name}: spot " in r.stdout and f"{name}: swap_limit used " in r.stdout     # one pool per kind
    assert "cfmm_quote_to_rate: query 0: rate_limit must be finite and > 0" in r.stdout
    assert "cfmm_swap_limit: query 0: rate_limit must be finite and >= 0" in r.stdout
    assert "cfmm_swap_limit: query 0: amount_in must be finite and >= 0" in r.stdout
