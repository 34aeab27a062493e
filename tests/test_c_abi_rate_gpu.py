"""cfmm_quote_rate / cfmm_quote_path_rate used from plain C (no Python, no torch in the process): tests/c/abi_rate.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "abi_rate")
    libdir = os.path.join(ROOT, "cfmmrouter.jl_amd")
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "abi_rate.c"), "-o", exe, "-L", libdir, "-lcfmm_amd", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    return exe


def test_plain_c_rate_client_compiles(tmp_path):
    """CPU: the declarations of include/cfmm_amd_rate.h are valid C11 and the client links against the library"""
    build(tmp_path)


@pytest.mark.gpu
def test_plain_c_rate_client(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "abi_rate: ok" in r.stdout
    for name in ("product", "geomean", "univ3", "weighted", "curve", "solidly"):
        assert f"{name}: out " in r.stdout                                     # one query per kind
    assert "path: out " in r.stdout and "cfmm_quote_rate: query 0: amount_in must be finite and >= 0" in r.stdout
