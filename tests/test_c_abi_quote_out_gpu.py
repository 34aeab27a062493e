"""cfmm_quote_out and cfmm_quote_out_dev used from plain C (no Python, no torch in the process): tests/c/abi_quote_out.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_quote_out")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_quote_out.c"), "-o", exe, "-L", libdir,
                    "-lcfmm_amd", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"],
                   check=True)
    return exe


def test_plain_c_quote_out_client_compiles(tmp_path):
    """CPU: the two declarations are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_quote_out_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_quote_out: ok" in r.stdout
    assert "query 1" in r.stdout and "quote_out_dev 3 -> nan" in r.stdout.lower() and "beyond the reserve: inf inf" in r.stdout
