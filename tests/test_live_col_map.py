"""The compact row index of the lean sweep's column phase (pqd_live_col_map). Host only, no device.

rho must list the live rows in increasing order (that order keeps the compacted product bit-identical to the full one),
then the rows that stay zero, and be a permutation; KC = ceil(n_live / 4). Checked for every mask of 16 rows with 1 to 16
live ones, and by value for the bench's mask (the x-polarised biexciton: 10 live rows, three k-steps).
"""
import ctypes as C

import numpy as np

from pyaceqd_amd import _lib
from tests import live_rows_cases as LC


def col_map(live):
    live = (C.c_uint8 * len(live))(*[int(v) for v in live])
    rho, kc = (C.c_uint8 * len(live))(), C.c_int32(-1)
    _lib.check(_lib.lib().pqd_live_col_map(live, len(live), rho, C.byref(kc)))
    return list(rho), kc.value


def test_every_mask_of_16_rows():
    for mask in range(1, 1 << 16):
        live = [(mask >> a) & 1 for a in range(16)]
        rho, kc = col_map(live)
        rows = [a for a in range(16) if live[a]]
        assert sorted(rho) == list(range(16)), (mask, rho)
        assert rho[:len(rows)] == rows, (mask, rho)
        assert rho[len(rows):] == [a for a in range(16) if not live[a]], (mask, rho)
        assert kc == (len(rows) + 3) // 4, (mask, kc)


def test_bench_mask():
    live = np.zeros(16, dtype=np.uint8)
    live[LC.X_ONLY] = 1
    rho, kc = col_map(live)
    assert rho[:10] == [0, 1, 3, 4, 5, 7, 10, 12, 13, 15] and kc == 3
    assert rho[10:] == [2, 6, 8, 9, 11, 14]


def test_nonzero_bytes_count_as_live_and_arguments_are_checked():
    rho, kc = col_map([0, 7, 0, 255])
    assert rho == [1, 3, 0, 2] and kc == 1
    L = _lib.lib()
    one, kc = (C.c_uint8 * 1)(1), C.c_int32()
    assert L.pqd_live_col_map(one, 0, one, C.byref(kc)) != 0
    assert L.pqd_live_col_map(None, 1, one, C.byref(kc)) != 0
