"""cfmm_find_disjoint_paths_out used from plain C (no Python, no torch in the process): tests/c/abi_find_disjoint_out.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_find_disjoint_out")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_find_disjoint_out.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_find_disjoint_out_client_compiles(tmp_path):
    """CPU: the declaration of include/cfmm_amd_find_disjoint_out.h is valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_find_disjoint_out_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_find_disjoint_out: ok" in r.stdout
    assert "query 0: 4 paths, query 1: 0 paths" in r.stdout
    assert "cfmm_find_disjoint_paths_out: max_paths must be 1 .. 8 (got 9)" in r.stdout
    assert "cfmm_find_disjoint_paths_out: query 1: token_out 4 out of range (the market has 4 tokens)" in r.stdout
