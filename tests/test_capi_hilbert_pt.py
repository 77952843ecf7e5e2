"""pqd_pt_create_wide (the PT handle of the Hilbert-space path with a PT, PQD_PATH_HILBERT_PT): its argument checks all
come before any device call, so no GPU is needed: the context handed in is a zeroed placeholder (as
tests/test_capi_hilbert.py). pqd_pt_create keeps dim <= 6."""
import ctypes as C
import os
import re

import numpy as np

from pyaceqd_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(dim, chi=3, D=2, n_slices=2, gmap=None, drop=None):
    keep = {"Q": np.zeros((n_slices, D, max(1, chi), max(1, chi)), dtype=np.complex128),
            "closure": np.zeros((n_slices, max(1, chi)), dtype=np.complex128),
            "closure0": np.zeros(max(1, chi), dtype=np.complex128), "bond0": np.zeros(max(1, chi), dtype=np.complex128),
            "gmap": np.zeros(dim * dim, dtype=np.int32) if gmap is None else np.ascontiguousarray(gmap, dtype=np.int32)}
    d = _lib.pqd_pt_desc()
    d.chi, d.D, d.n_slices = chi, D, n_slices
    d.Q, d.closure, d.closure0 = _lib.cptr(keep["Q"]), _lib.cptr(keep["closure"]), _lib.cptr(keep["closure0"])
    d.bond0, d.gmap = _lib.cptr(keep["bond0"]), _lib.iptr(keep["gmap"])
    if drop is not None:
        setattr(d, drop, None)
    return d, keep


def _create(fn, dim, **kw):
    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(256), C.c_void_p)
    d, keep = _desc(dim, **kw)
    h = C.c_void_p()
    rc = getattr(L, fn)(ctx, dim, C.byref(d), C.byref(h))
    assert not h.value
    return rc, L.pqd_last_error().decode()


def test_entry_point_and_path_constant():
    assert "pqd_pt_create_wide" in _lib.EXPORTED and hasattr(_lib.lib(), "pqd_pt_create_wide")
    src = open(os.path.join(REPO, "include", "pqd.h")).read()
    assert "int pqd_pt_create_wide(pqd_ctx* ctx, int32_t dim, const pqd_pt_desc*" in src
    assert int(re.search(r"#define PQD_PATH_HILBERT_PT (\d+)", src).group(1)) == _lib.PQD_PATH_HILBERT_PT == 6


def test_dim_outside_2_to_24_is_refused():
    for dim in (1, 25):
        rc, msg = _create("pqd_pt_create_wide", dim)
        assert rc == _lib.PQD_ERR_UNSUPPORTED and "dim %d not in [2, 24]" % dim in msg


def test_chi_outside_1_to_256_is_refused():
    for chi in (0, 257):
        rc, msg = _create("pqd_pt_create_wide", 8, chi=chi)
        assert rc == _lib.PQD_ERR_UNSUPPORTED and "chi %d not in [1, 256]" % chi in msg


def test_argument_checks_come_before_any_device_call():
    for name in ("Q", "closure", "closure0", "bond0", "gmap"):
        rc, msg = _create("pqd_pt_create_wide", 8, drop=name)
        assert rc == 1 and "NULL PT array" in msg, name
    for D, n_slices in ((0, 2), (2, 0)):
        rc, msg = _create("pqd_pt_create_wide", 8, D=D, n_slices=n_slices)
        assert rc == 1 and "D and n_slices" in msg
    gmap = np.zeros(64, dtype=np.int32)
    gmap[63] = 2
    rc, msg = _create("pqd_pt_create_wide", 8, D=2, gmap=gmap)
    assert rc == 1 and "gmap[63]=2 out of [0,2)" in msg
    gmap[63], gmap[5] = 0, -1
    rc, msg = _create("pqd_pt_create_wide", 8, D=2, gmap=gmap)
    assert rc == 1 and "gmap[5]=-1" in msg
    L = _lib.lib()
    h = C.c_void_p()
    d, keep = _desc(8)
    assert L.pqd_pt_create_wide(None, 8, C.byref(d), C.byref(h)) == 1
    assert L.pqd_pt_create_wide(C.cast(C.create_string_buffer(256), C.c_void_p), 8, None, C.byref(h)) == 1


def test_pqd_pt_create_still_stops_at_dim_6():
    rc, msg = _create("pqd_pt_create", 8)
    assert rc == _lib.PQD_ERR_UNSUPPORTED and "dim 8" in msg
    rc, msg = _create("pqd_pt_create", 7)
    assert rc == _lib.PQD_ERR_UNSUPPORTED and "dim 7" in msg
