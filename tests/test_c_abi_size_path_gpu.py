"""cfmm_size_path used from plain C (no Python, no torch in the process): tests/c/abi_size_path.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_size_path")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_size_path.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_size_path_client_compiles(tmp_path):
    """CPU: the two declarations of include/cfmm_amd_size_path.h are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_size_path_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_size_path: ok" in r.stdout
    assert "path 0: status 0" in r.stdout and "path 1: status 2" in r.stdout and "path 2: status 1" in r.stdout
    assert "cfmm_size_path: path 1, hop 0: max_amount_in must be finite and >= 0" in r.stdout
