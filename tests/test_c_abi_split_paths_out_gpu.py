"""cfmm_split_paths_out used from plain C (no Python, no torch in the process): tests/c/abi_split_paths_out.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_split_paths_out")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_split_paths_out.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_split_paths_out_client_compiles(tmp_path):
    """CPU: the declarations of include/cfmm_amd_split_out.h are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_split_paths_out_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_split_paths_out: ok" in r.stdout
    assert "order 0: status 0" in r.stdout and "order 1: status 0" in r.stdout and "order 2: status 1" in r.stdout and "order 3: status 4" in r.stdout
    assert "cfmm_split_paths_out: order 0: paths 0 and 2 share pool (segment 0, row 0)" in r.stdout
