"""The C oracle's time-bin entry points (oracle/mapchain_oracle.c: or_four_time_8op, or_four_time, or_dynamics_t1)
against the long-double restatement of timebin_tl.f90 in tests/helpers.py, on the inputs of tests/test_gpu_timebin.py
(helpers.timebin_inputs), dims 2-6. No GPU.

Bound: the worst oracle-against-long-double difference measured on these inputs, relative to the largest element of
the result, was 1.42e-15 (four_time_8op with late_t1_only, dim 4; per entry point: four_time_8op 1.37e-15,
early_only 1.36e-15, late_t1_only 1.42e-15, four_time 1.22e-15, dynamics_t1 1.26e-15). The tests assert ten times the
worst value, 1.42e-14: the factor covers summation order and libm differences between hosts.

The same file checks what the inputs have to provide for the GPU tests to mean anything: no segment needs a precalc
map that does not exist, every grid has the listed kinds of points, pairs that share a wave need different step
counts, and the strict lower triangle of every result is exactly 0."""
import numpy as np
import pytest

from oracle import oracle
from tests import helpers as H

BOUND = 1.42e-14  # 10 x the measured worst (docstring)
DIMS = [2, 3, 4, 5, 6]
N_T = {2: 33, 3: 15, 4: 9, 5: 6, 6: 5}


def rel(a, b):
    b = np.asarray(b)
    d = np.max(np.abs(np.asarray(a, dtype=b.dtype) - b))
    return float(d / np.max(np.abs(b)))


def _args(z):
    return z["dm_1"], z["dm_2"], z["rho"], z["t1"], z["precalc"], z["dt"], z["dim"]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)], ids=["plain", "early", "late_t1"])
def test_four_time_8op_oracle_vs_long_double(dim, flags):
    z = H.timebin_inputs(dim)
    ref, top = H.numpy_four_time_8op(*_args(z), z["ops8"], *flags, z["tb"])
    got = oracle.four_time_8op(*_args(z), z["ops8"], *flags, z["tb"])
    assert top < z["n_precalc"]
    assert top >= 1  # the binary powers are in use, and not only the first
    e = rel(got, ref)
    print(f"four_time_8op dim {dim} flags {flags}: oracle vs long double {e:.3e}, top precalc bit {top}")
    assert e < BOUND
    assert np.all(np.tril(got, -1) == 0)
    assert np.all(np.tril(ref, -1) == 0)
    assert np.all(np.abs(got[np.triu_indices(len(got))]) > 0)


@pytest.mark.parametrize("dim", DIMS)
def test_four_time_oracle_vs_long_double(dim):
    z = H.timebin_inputs(dim)
    ref, top = H.numpy_four_time(*_args(z), z["ops8"][:4], z["tb"])
    got = oracle.four_time(*_args(z), z["ops8"][:4], z["tb"])
    assert top < z["n_precalc"]
    e = rel(got, ref)
    print(f"four_time dim {dim}: oracle vs long double {e:.3e}, top precalc bit {top}")
    assert e < BOUND
    assert np.all(np.tril(got, -1) == 0)
    assert np.all(np.tril(ref, -1) == 0)


@pytest.mark.parametrize("dim", DIMS)
def test_dynamics_t1_oracle_vs_long_double(dim):
    z = H.timebin_inputs(dim)
    grids = [z["t1"], z["t1"][:1], z["t1"][:2], z["t1"][::-1], np.array([0.4, 1.3, 0.2, 0.2, 2.9, 0.65])]
    for t1 in grids:
        ref, top = H.numpy_dynamics_t1(z["dm_1"], z["dm_2"], z["rho"], t1, z["precalc"], z["dt"], dim)
        got = oracle.dynamics_t1(z["dm_1"], z["dm_2"], z["rho"], t1, z["precalc"], z["dt"], dim, z["tb"])
        assert top < z["n_precalc"]
        e = rel(got, ref)
        print(f"dynamics_t1 dim {dim} n_t {len(t1)}: oracle vs long double {e:.3e}, top precalc bit {top}")
        assert e < BOUND


@pytest.mark.parametrize("dim", DIMS)
def test_grid_properties(dim):
    """what the t1 grids promise (the reasons are in the docstring of test_gpu_timebin.py)"""
    z = H.timebin_inputs(dim)
    t1, dt, tb, n_map = z["t1"], z["dt"], z["tb"], z["n_map"]
    assert len(t1) == N_T[dim]
    assert np.all(np.diff(t1) >= 0)
    assert np.any(np.diff(t1) == 0)                                     # a repeated point
    assert any(t in t1 for t in (0.25, 0.65))                           # off the dt raster
    trunc = [t for t in (0.3, 0.6, 0.7) if t in t1]
    assert trunc and all(int(H.tb_round6(t) / dt) == round(t / dt) - 1 for t in trunc)  # int() truncates below the raster index
    assert np.any(t1 < n_map * dt - 1e-9) and np.any(t1 >= n_map * dt)  # inside the explicit maps, and past them
    assert t1[-1] > tb                                                  # (t2, tb) with a negative step count
    assert H.tb_steps(t1[-1], tb, dt, n_map)[1:] == (0, 0)
    # a segment that crosses from the explicit maps into the binary powers
    assert any(sd > 0 and rem > 0 for sd, rem in (H.tb_steps(0.0, t, dt, n_map)[1:] for t in t1))
    # every segment of every entry point stays inside the precalc maps
    segs = [(0.0, t) for t in t1] + [(t, tb) for t in t1] + [(a, b) for i, a in enumerate(t1) for b in t1[i:]]
    assert max(H.tb_steps(a, b, dt, n_map)[2] for a, b in segs) < 2 ** z["n_precalc"]
    # pairs in the host's order (row i, then j): the last wave is partly filled, and pairs that share a wave differ
    # in their explicit-map step counts and in their remainders in most waves
    tpw = 64 // (dim * dim)
    pairs = [(i, i + j) for i in range(len(t1)) for j in range(len(t1) - i)]
    assert len(pairs) == len(t1) * (len(t1) + 1) // 2
    if dim <= 4:
        assert len(pairs) % tpw == 1
    elif dim == 5:
        assert len(pairs) % tpw != 0
    if tpw > 1:
        waves = [pairs[k: k + tpw] for k in range(0, len(pairs) - tpw + 1, tpw)]
        st = [[H.tb_steps(t1[i], t1[j], dt, n_map)[1:] for i, j in w] for w in waves]
        mixed_dm = sum(len({s[0] for s in w}) > 1 for w in st)
        mixed_rem = sum(len({s[1] for s in w}) > 1 for w in st)
        assert mixed_dm >= 1 and mixed_rem >= 1
        assert 2 * sum(len(set(w)) > 1 for w in st) >= len(waves)


def test_round6_and_steps():
    assert H.tb_round6(0.12345649) == 0.123456 and H.tb_round6(0.1234565) == 0.123457
    assert H.tb_round6(-0.1234565) == -0.123457
    assert H.tb_steps(0.0, 0.3, 0.1, 7) == (0, 2, 0)      # 0.3 / 0.1 = 2.9999999999999996
    assert H.tb_steps(0.5, 1.2, 0.1, 7) == (5, 2, 4)      # 1.2 / 0.1 = 11.999999999999998: across the last map
    assert H.tb_steps(0.9, 2.3, 0.1, 7) == (9, 0, 13)     # start past the maps; 2.3 / 0.1 truncates to 22
    assert H.tb_steps(2.5, 2.3, 0.1, 7) == (25, 0, 0)     # negative: identity
    assert H.tb_steps(0.65, 0.65, 0.1, 7) == (6, 0, 0)
