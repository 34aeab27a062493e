"""cfmm_swap_out and cfmm_swap_path_out used from plain C (no Python, no torch in the process): tests/c/abi_swap_out.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_swap_out")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_swap_out.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_swap_out_client_compiles(tmp_path):
    """CPU: the two declarations and the CFMM_SWAP_* constants are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_swap_out_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_swap_out: ok" in r.stdout
    assert "status 0 3 1 0, swap_refused 2, launches 4" in r.stdout
    assert "status 0, then" in r.stdout and "swap_refused 1, launches 2" in r.stdout and "unobtainable path: inf" in r.stdout.lower()
    assert "cfmm_swap_path_out: path 0, hops 0 and 1" in r.stdout
