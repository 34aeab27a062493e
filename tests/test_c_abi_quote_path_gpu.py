"""cfmm_quote_path and cfmm_quote_path_out used from plain C (no Python, no torch in the process): tests/c/abi_quote_path.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_quote_path")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_quote_path.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_quote_path_client_compiles(tmp_path):
    """CPU: the four declarations are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_quote_path_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_quote_path: ok" in r.stdout
    assert "path 2, hop 1: row 3" in r.stdout and "beyond the reserve: inf inf inf inf" in r.stdout
