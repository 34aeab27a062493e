"""csrc/devbuf.h, the one owner of a device array, built for the host behind tests/native/devbuf_host.cpp: DevBuf<double>
over malloc / free with a count of the live allocations and an injectable allocation failure.  What is asserted is the
ownership: the live count after every operation, 0 at the end, and an empty buffer + CFMM_ERR_HIP after a failure."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFMM_OK, CFMM_ERR_HIP = 0, -2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("devbuf") / "devbuf_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"), "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC",
                    os.path.join(ROOT, "tests", "native", "devbuf_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    ll, vp = ctypes.c_longlong, ctypes.c_void_p
    L.devbuf_live.restype = ll
    L.devbuf_fail_at.argtypes = [ll]
    L.devbuf_last_error.restype = ctypes.c_char_p
    L.devbuf_new.restype = vp
    L.devbuf_delete.argtypes = [vp]
    L.devbuf_move_new.restype, L.devbuf_move_new.argtypes = vp, [vp]
    L.devbuf_move_assign.argtypes = [vp, vp]
    for f in (L.devbuf_alloc, L.devbuf_grow, L.devbuf_alloc_fine):
        f.restype, f.argtypes = ctypes.c_int, [vp, ll]
    L.devbuf_upload.restype, L.devbuf_upload.argtypes = ctypes.c_int, [vp, vp, ll]
    L.devbuf_reset.argtypes = [vp]
    L.devbuf_size.restype, L.devbuf_size.argtypes = ll, [vp]
    L.devbuf_get.restype, L.devbuf_get.argtypes = vp, [vp]
    L.devbuf_bool.restype, L.devbuf_bool.argtypes = ctypes.c_int, [vp]
    L.devbuf_four_uploads.restype, L.devbuf_four_uploads.argtypes = ctypes.c_int, [vp, ll, ctypes.POINTER(ll)]
    assert L.devbuf_live() == 0
    yield L
    L.devbuf_fail_at(0)
    assert L.devbuf_live() == 0


def state(L, b):
    return L.devbuf_get(b), L.devbuf_size(b), L.devbuf_bool(b)


def contents(L, b):
    return np.ctypeslib.as_array(ctypes.cast(L.devbuf_get(b), ctypes.POINTER(ctypes.c_double)), shape=(L.devbuf_size(b),)).copy()


SRC = np.arange(1.0, 38.0)   # 37 doubles
P = SRC.ctypes.data_as(ctypes.c_void_p)


def test_construction_and_destruction(lib):
    b = lib.devbuf_new()
    assert state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    assert lib.devbuf_alloc(b, 5) == CFMM_OK and lib.devbuf_live() == 1
    assert state(lib, b)[1:] == (5, 1) and state(lib, b)[0]
    assert lib.devbuf_alloc(b, 0) == CFMM_OK and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0   # a count of 0: empty
    assert lib.devbuf_upload(b, P, SRC.size) == CFMM_OK and lib.devbuf_live() == 1
    np.testing.assert_array_equal(contents(lib, b), SRC)
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0
    lib.devbuf_delete(lib.devbuf_new())       # an empty one releases nothing
    assert lib.devbuf_live() == 0


def test_move_construction_hands_the_array_over(lib):
    a = lib.devbuf_new()
    assert lib.devbuf_upload(a, P, SRC.size) == CFMM_OK
    ptr = lib.devbuf_get(a)
    b = lib.devbuf_move_new(a)
    assert lib.devbuf_live() == 1 and state(lib, a) == (None, 0, 0) and state(lib, b) == (ptr, SRC.size, 1)
    lib.devbuf_delete(a)
    assert lib.devbuf_live() == 1             # the moved-from buffer owns nothing
    np.testing.assert_array_equal(contents(lib, b), SRC)
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0


def test_move_assignment_releases_what_the_target_held(lib):
    a, b = lib.devbuf_new(), lib.devbuf_new()
    assert lib.devbuf_upload(a, P, 7) == CFMM_OK and lib.devbuf_alloc(b, 1000) == CFMM_OK and lib.devbuf_live() == 2
    ptr = lib.devbuf_get(a)
    lib.devbuf_move_assign(b, a)
    assert lib.devbuf_live() == 1 and state(lib, a) == (None, 0, 0) and state(lib, b) == (ptr, 7, 1)
    np.testing.assert_array_equal(contents(lib, b), SRC[:7])
    lib.devbuf_move_assign(b, b)              # onto itself: nothing happens
    assert lib.devbuf_live() == 1 and state(lib, b) == (ptr, 7, 1)
    lib.devbuf_move_assign(b, a)              # an empty source: the target is released and empty
    assert lib.devbuf_live() == 0 and state(lib, b) == (None, 0, 0)
    lib.devbuf_delete(a)
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0


def test_grow_reallocates_only_upwards_and_never_holds_two_arrays(lib):
    b = lib.devbuf_new()
    assert lib.devbuf_grow(b, 0) == CFMM_OK and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    assert lib.devbuf_grow(b, 16) == CFMM_OK and lib.devbuf_live() == 1 and lib.devbuf_size(b) == 16
    ptr = lib.devbuf_get(b)
    # smaller or equal: untouched, as the buffers it replaces (`if (need > cap)` around free + hipMalloc)
    assert lib.devbuf_grow(b, 4) == CFMM_OK and lib.devbuf_grow(b, 16) == CFMM_OK
    assert state(lib, b) == (ptr, 16, 1) and lib.devbuf_live() == 1
    # larger: free first, then allocate -- with the ONE allocation of the growth failing, nothing is live (an
    # allocate-then-free order would still hold the old array here)
    lib.devbuf_fail_at(1)
    assert lib.devbuf_grow(b, 64) == CFMM_ERR_HIP and lib.devbuf_live() == 0 and state(lib, b) == (None, 0, 0)
    lib.devbuf_fail_at(0)
    assert lib.devbuf_grow(b, 64) == CFMM_OK and lib.devbuf_live() == 1 and lib.devbuf_size(b) == 64
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0


def test_upload_of_nothing_and_reset(lib):
    b = lib.devbuf_new()
    assert lib.devbuf_upload(b, P, 0) == CFMM_OK and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    assert lib.devbuf_upload(b, None, 0) == CFMM_OK and lib.devbuf_live() == 0
    assert lib.devbuf_upload(b, P, 3) == CFMM_OK and lib.devbuf_live() == 1
    assert lib.devbuf_upload(b, P, 0) == CFMM_OK and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0   # ... releases
    assert lib.devbuf_upload(b, P, 3) == CFMM_OK and lib.devbuf_live() == 1
    lib.devbuf_reset(b)
    assert state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    lib.devbuf_reset(b)                       # twice: nothing to release
    assert lib.devbuf_live() == 0
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0


@pytest.mark.parametrize("op", ["alloc", "upload", "grow"])
@pytest.mark.parametrize("held", [0, 8])
def test_a_failed_allocation_leaves_the_buffer_empty(lib, op, held):
    b = lib.devbuf_new()
    assert lib.devbuf_alloc(b, held) == CFMM_OK and lib.devbuf_live() == (1 if held else 0)
    lib.devbuf_fail_at(1)
    rc = lib.devbuf_upload(b, P, 20) if op == "upload" else getattr(lib, "devbuf_" + op)(b, 20)
    lib.devbuf_fail_at(0)
    assert rc == CFMM_ERR_HIP and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    assert b"160 bytes" in lib.devbuf_last_error() and b"injected failure" in lib.devbuf_last_error()
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0


@pytest.mark.parametrize("k", [1, 2, 3, 4, 0])
def test_four_uploads_in_one_scope_leave_nothing_behind(lib, k):
    """the k-th of four chained uploads fails (0: none): the k - 1 before it are live inside the scope, nothing after it"""
    inside = ctypes.c_longlong(-1)
    lib.devbuf_fail_at(k)
    rc = lib.devbuf_four_uploads(P, SRC.size, ctypes.byref(inside))
    lib.devbuf_fail_at(0)
    assert rc == (CFMM_ERR_HIP if k else CFMM_OK)
    assert inside.value == (k - 1 if k else 4)
    assert lib.devbuf_live() == 0


def test_alloc_fine_owns_like_alloc_and_fails_silently(lib):
    """the fine-grained variant (the arm buffer): what the buffer held goes first, a count of 0 or a failure leaves it empty
    -- and sets no error text, because the buffer is optional wherever it is used"""
    b = lib.devbuf_new()
    assert lib.devbuf_alloc_fine(b, 0) == 0 and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    assert lib.devbuf_alloc_fine(b, 9) == 1 and lib.devbuf_live() == 1 and lib.devbuf_size(b) == 9 and lib.devbuf_bool(b) == 1
    assert lib.devbuf_alloc_fine(b, 17) == 1 and lib.devbuf_live() == 1 and lib.devbuf_size(b) == 17    # the old array went first
    assert lib.devbuf_alloc(b, 3) == CFMM_OK and lib.devbuf_live() == 1                                  # ... whichever kind it was
    err = lib.devbuf_last_error()
    lib.devbuf_fail_at(1)
    assert lib.devbuf_alloc_fine(b, 5) == 0 and state(lib, b) == (None, 0, 0) and lib.devbuf_live() == 0
    lib.devbuf_fail_at(0)
    assert lib.devbuf_last_error() == err                                                                 # no error text
    assert lib.devbuf_alloc_fine(b, 5) == 1 and lib.devbuf_live() == 1
    lib.devbuf_delete(b)
    assert lib.devbuf_live() == 0
