"""cfmm_swap_order / cfmm_swap_order_out used from plain C (no Python, no torch in the process): tests/c/abi_swap_order.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_swap_order")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_swap_order.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_swap_order_client_compiles(tmp_path):
    """CPU: the declarations and the CFMM_ORDER_* constants of include/cfmm_amd_order.h are valid C11 and the client links"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_swap_order_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_swap_order: ok" in r.stdout
    assert "status 0, then" in r.stdout and "swap_refused 1, launches 2" in r.stdout and "refused order: total nan" in r.stdout.lower()
    assert "cfmm_swap_order: order 0: paths 0 and 1 share pool (segment 0, row 0)" in r.stdout
