"""The argument checks of pqd_tl_dynmap_pseudo after the block-Jacobi kernel (map sizes up to 576) and the binding of
pqd_tl_dynmap_timing. All of these are answered before the context is touched, so no GPU is needed: the context handed
in is a zeroed placeholder (as in tests/test_capi_hilbert.py)."""
import ctypes as C

import numpy as np

from pyaceqd_amd import _lib

PQD_OK, PQD_ERR_ARG, PQD_ERR_UNSUPPORTED = 0, 1, 3   # include/pqd.h


def _call(n, n_maps, rcond=1e-12):
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(256), C.c_void_p)
    buf = np.zeros(4, dtype=np.complex128)   # never read: every call here returns before the device is used
    rc = L.pqd_tl_dynmap_pseudo(ctx, _lib.cptr(buf), n_maps, n, rcond, _lib.cptr(buf))
    return rc, L.pqd_last_error().decode()


def test_sizes_above_36_pass_the_size_check():
    for n in (37, 50, 324, 576):
        rc, _ = _call(n, 0)
        assert rc == PQD_OK, n
    rc, _ = _call(36, 0)
    assert rc == PQD_OK


def test_refusals():
    for n in (577, 1024):
        rc, msg = _call(n, 0)
        assert rc == PQD_ERR_UNSUPPORTED and "map size %d (max 576)" % n in msg
    rc, msg = _call(0, 0)
    assert rc == PQD_ERR_UNSUPPORTED and "map size 0" in msg
    # the order of the checks: the size before n_maps before rcond
    rc, msg = _call(37, -1, rcond=-1.0)
    assert rc == PQD_ERR_ARG and "n_maps" in msg
    rc, msg = _call(37, 0, rcond=-1e-12)
    assert rc == PQD_ERR_ARG and "rcond" in msg
    rc, msg = _call(37, 0, rcond=float("nan"))
    assert rc == PQD_ERR_ARG and "rcond" in msg
    L = _lib.lib()
    buf = np.zeros(4, dtype=np.complex128)
    assert L.pqd_tl_dynmap_pseudo(None, _lib.cptr(buf), 0, 37, 1e-12, _lib.cptr(buf)) == PQD_ERR_ARG


def test_timing_is_bound_and_refuses_null():
    L = _lib.lib()
    ms = C.c_double(-7.0)
    assert L.pqd_tl_dynmap_timing(None, C.byref(ms)) == PQD_ERR_ARG
    assert b"NULL" in L.pqd_last_error()
    ctx = C.cast(C.create_string_buffer(256), C.c_void_p)
    assert L.pqd_tl_dynmap_timing(ctx, None) == PQD_ERR_ARG
    assert ms.value == -7.0
    n = C.c_int32(-7)
    assert L.pqd_tl_dynmap_sweeps(None, C.byref(n)) == PQD_ERR_ARG
    assert L.pqd_tl_dynmap_sweeps(ctx, None) == PQD_ERR_ARG
