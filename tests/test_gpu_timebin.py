"""The time-bin kernels of mapchain.hip (ft_prologue_kernel, ft_pairs_kernel, dyn_t1_kernel, behind four_time_8op,
its rows variant, four_time and dynamics_t1) against the C oracle at every dim 2-6. GPU only.

The kernels pack 64 / N^2 pairs into a wave and advance all of them to the wave's largest step count, masking the
pairs that are done (prop_tb). What can go wrong there is one pair's step count, map index or padding lane leaking
into another pair, so the inputs (helpers.timebin_inputs, properties asserted in test_timebin_oracle.py) are built
around the packing: per dim the pair triangle leaves one pair in the last wave (dims 2-4: 561 / 120 / 45 pairs at 16 /
7 / 4 pairs a wave), a ragged last wave (dim 5) or 28 idle lanes (dim 6); the sorted t1 grids hold a repeated point, a
point off the dt raster, a point where int(round6(t) / dt) truncates, points inside and past the 7 explicit maps (a
segment crosses from the maps into the 5 binary powers) and a point past tb (a negative step count: the identity), and
pairs that share a wave need different step counts.

Reference: the C oracle, itself checked against a long-double restatement of the Fortran on the same inputs
(test_timebin_oracle.py, 1.42e-15). Tolerance: 1e-12 relative to the largest element, as test_gpu_parity.py uses for
these kernels. Worst GPU-against-oracle values observed on an MI355X: four_time_8op 2.7e-15 (early_only 2.3e-15,
late_t1_only 2.2e-15), four_time 1.7e-15, dynamics_t1 1.2e-15; against the long-double restatement utils.fast_propagate
7.2e-16 and utils.propagate_tb 9.2e-16."""
import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd.timebin import timebin_tl as TB
from tests import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-12
DIMS = [2, 3, 4, 5, 6]
FLAGS = {"plain": (False, False), "early": (True, False), "late_t1": (False, True)}
_cache = {}


def rel(a, b):
    b = np.asarray(b)
    return float(np.max(np.abs(np.asarray(a, dtype=b.dtype) - b)) / max(1e-300, np.max(np.abs(b))))


def all_zero_bytes(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


def inputs(dim):
    if dim not in _cache:
        _cache[dim] = H.timebin_inputs(dim)
    return _cache[dim]


def args(z, t1=None, precalc=None):
    return (z["dm_1"], z["dm_2"], z["rho"], z["t1"] if t1 is None else t1, z["precalc"] if precalc is None else precalc,
            z["dt"], z["dim"])


def full_8op(dim, flags):
    """the GPU result on the full grid, computed once per (dim, flags) and never modified"""
    key = (dim, flags)
    if key not in _cache:
        z = inputs(dim)
        r = TB.four_time_8op(*args(z), *z["ops8"], *FLAGS[flags], z["tb"])
        r.setflags(write=False)
        _cache[key] = r
    return _cache[key]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("flags", list(FLAGS))
def test_four_time_8op_vs_oracle(dim, flags):
    z = inputs(dim)
    got = full_8op(dim, flags)
    ref = oracle.four_time_8op(*args(z), z["ops8"], *FLAGS[flags], z["tb"])
    e = rel(got, ref)
    print(f"four_time_8op {flags} dim {dim}: GPU vs oracle {e:.3e}")
    assert got.shape == ref.shape == (len(z["t1"]),) * 2
    assert e < TOL
    assert np.all(np.tril(got, -1) == 0)


@pytest.mark.parametrize("dim", DIMS)
def test_four_time_8op_flags_give_different_results(dim):
    """the three flag settings stop at different places of the chain: no two of them may agree"""
    a, b, c = (full_8op(dim, f) for f in FLAGS)
    iu = np.triu_indices(len(a))
    for x, y in ((a, b), (a, c), (b, c)):
        assert np.all(x[iu] != y[iu])


@pytest.mark.parametrize("dim", DIMS)
def test_four_time_vs_oracle(dim):
    z = inputs(dim)
    got = TB.four_time(*args(z), *z["ops8"][:4], z["tb"])
    ref = oracle.four_time(*args(z), z["ops8"][:4], z["tb"])
    e = rel(got, ref)
    print(f"four_time dim {dim}: GPU vs oracle {e:.3e}")
    assert e < TOL
    assert np.all(np.tril(got, -1) == 0)


@pytest.mark.parametrize("dim", DIMS)
def test_dynamics_t1_vs_oracle(dim):
    """the full grid, n_t = 1 (rho_init alone), n_t = 2, and grids that are not monotonic: a negative segment copies
    the state (timebin_tl.f90:61-76 with n_steps < 0)"""
    z = inputs(dim)
    N2 = dim * dim
    grids = [z["t1"], z["t1"][:1], z["t1"][:2], z["t1"][::-1].copy(), np.array([0.4, 1.3, 0.2, 0.2, 2.9, 0.65])]
    for t1 in grids:
        got = TB.dynamics_t1(*args(z, t1=t1), z["tb"])
        ref = oracle.dynamics_t1(*args(z, t1=t1), z["tb"])
        e = rel(got, ref)
        print(f"dynamics_t1 dim {dim} n_t {len(t1)}: GPU vs oracle {e:.3e}")
        assert got.shape == (N2, 2 * len(t1) - 1)
        assert e < TOL
    one = TB.dynamics_t1(*args(z, t1=z["t1"][:1]), z["tb"])
    assert np.array_equal(one[:, 0], z["rho"])
    back = TB.dynamics_t1(*args(z, t1=z["t1"][::-1].copy()), z["tb"])
    assert all(np.array_equal(back[:, k], z["rho"]) for k in range(back.shape[1]))  # every segment <= 0 steps
    mixed = TB.dynamics_t1(*args(z, t1=np.array([0.4, 1.3, 0.2, 0.2, 2.9, 0.65])), z["tb"])
    assert np.array_equal(mixed[:, 2], mixed[:, 1]) and np.array_equal(mixed[:, 3], mixed[:, 1])
    assert not np.array_equal(mixed[:, 4], mixed[:, 3])


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("flags", ["plain", "late_t1"])
def test_packing_independence(dim, flags):
    """a pair's value may not depend on which pairs share its wave: dropping the last 1 or 3 grid points shortens every
    row of the triangle, which moves every later pair to another lane group and into other company; the results
    on the shorter grid are the leading block of the full result, bit for bit"""
    z = inputs(dim)
    full = full_8op(dim, flags)
    n_t = len(z["t1"])
    tpw = 64 // (dim * dim)
    for m in (n_t - 1, n_t - 3):
        if tpw > 1:
            assert (n_t - m) % tpw != 0  # row 1 starts at another lane group than in the full call
        sub = TB.four_time_8op(*args(z, t1=z["t1"][:m]), *z["ops8"], *FLAGS[flags], z["tb"])
        assert np.array_equal(sub, full[:m, :m])


@pytest.mark.parametrize("dim", DIMS)
def test_four_time_packing_independence(dim):
    z = inputs(dim)
    full = TB.four_time(*args(z), *z["ops8"][:4], z["tb"])
    m = len(z["t1"]) - 1
    sub = TB.four_time(*args(z, t1=z["t1"][:m]), *z["ops8"][:4], z["tb"])
    assert np.array_equal(sub, full[:m, :m])


@pytest.mark.parametrize("dim", DIMS)
def test_rows_in_one_process(dim):
    """four_time_8op(rows=(lo, hi)): the rows asked for are the full call's bit for bit, every other byte is 0"""
    z = inputs(dim)
    full = full_8op(dim, "plain")
    n_t = len(z["t1"])
    k = n_t // 2 + 1
    call = lambda rows: TB.four_time_8op(*args(z), *z["ops8"], False, False, z["tb"], rows=rows)  # noqa: E731
    lo, hi = call((0, k)), call((k, n_t))
    assert np.array_equal(lo[:k], full[:k]) and all_zero_bytes(lo[k:])
    assert np.array_equal(hi[k:], full[k:]) and all_zero_bytes(hi[:k])
    assert np.array_equal(lo + hi, full)
    assert all_zero_bytes(call((k, k)))
    one = call((1, 2))
    assert np.array_equal(one[1], full[1]) and all_zero_bytes(one[0]) and all_zero_bytes(one[2:])
    for bad in ((-1, 2), (0, n_t + 1), (3, 2), (n_t + 1, n_t + 2)):
        with pytest.raises(ValueError, match="rows"):
            call(bad)


@pytest.mark.parametrize("dim", [3, 4])
def test_utils_fast_propagate_every_step_count(dim):
    """utils.fast_propagate for every n_steps that 5 binary powers can express, against the long-double restatement"""
    z = inputs(dim)
    worst = 0.0
    for n in range(2 ** z["n_precalc"]):
        got = TB.utils.fast_propagate(z["rho"], z["precalc"], n)
        ref, top = H.numpy_fast_propagate(z["rho"], z["precalc"], n)
        assert top == n.bit_length() - 1
        worst = max(worst, rel(got, ref))
        if n == 0:
            assert np.array_equal(got, z["rho"])
    print(f"utils.fast_propagate dim {dim}: GPU vs long double {worst:.3e}")
    assert worst < TOL
    with pytest.raises(ValueError, match="precalc"):
        TB.utils.fast_propagate(z["rho"], z["precalc"], 2 ** z["n_precalc"])


@pytest.mark.parametrize("dim", [3, 4])
def test_utils_propagate_tb(dim):
    z = inputs(dim)
    segs = [(0.65, 0.65), (0.3, 0.3), (0.0, 0.3), (0.25, 0.6), (0.0, 0.7), (0.5, 1.2), (0.6, 2.3), (0.9, 2.3),
            (0.7, 0.8), (1.25, 3.05), (0.0, 3.8), (2.5, 2.3)]
    kinds = set()
    worst = 0.0
    for a, b in segs:
        got = TB.utils.propagate_tb(a, b, z["dt"], z["rho"], z["dm_1"], z["precalc"])
        ref, top = H.numpy_propagate_tb(a, b, z["dt"], z["rho"], z["dm_1"], z["precalc"])
        assert top < z["n_precalc"]
        n_start, sd, rem = H.tb_steps(a, b, z["dt"], z["n_map"])
        kinds.add((n_start >= z["n_map"], sd > 0, rem > 0))
        if sd == 0 and rem == 0:
            assert np.array_equal(got, z["rho"])
        worst = max(worst, rel(got, ref))
    # t_start == t_stop, a start past the maps, a segment inside the maps, one crossing n_dm
    assert {(False, False, False), (True, False, True), (False, True, False), (False, True, True)} <= kinds
    print(f"utils.propagate_tb dim {dim}: GPU vs long double {worst:.3e}")
    assert worst < TOL


@pytest.mark.parametrize("dim", [2, 5])
def test_refuses_a_remainder_beyond_the_precalc_maps(dim):
    """fast_propagate reads dm_tl_precalc(:, :, bit + 1) for every set bit of the steps left after the explicit maps
    (timebin_tl.f90:36-46): a remainder of 2^n_precalc or more would read past the array. Such a call is refused; the
    same call with one more binary power passes and agrees with the oracle"""
    z = inputs(dim)
    more = np.asfortranarray(np.concatenate([z["precalc"], (z["precalc"][:, :, -1] @ z["precalc"][:, :, -1])[:, :, None]],
                                            axis=2))
    o = z["ops8"]
    # (0, 3.95): 39 steps, 7 on the maps, 32 left = 2^5
    assert H.tb_steps(0.0, 3.95, z["dt"], z["n_map"])[2] == 32 and H.tb_steps(0.0, 3.85, z["dt"], z["n_map"])[2] == 31
    t_ok, t_bad = np.array([0.0, 0.25, 3.85]), np.array([0.0, 0.25, 3.95])
    calls = {
        "8op": lambda t, p: TB.four_time_8op(*args(z, t1=t, precalc=p), *o, False, False, z["tb"]),
        "4op": lambda t, p: TB.four_time(*args(z, t1=t, precalc=p), *o[:4], z["tb"]),
        "dyn": lambda t, p: TB.dynamics_t1(*args(z, t1=t, precalc=p), z["tb"]),
    }
    refs = {
        "8op": lambda t, p: oracle.four_time_8op(*args(z, t1=t, precalc=p), o, False, False, z["tb"]),
        "4op": lambda t, p: oracle.four_time(*args(z, t1=t, precalc=p), o[:4], z["tb"]),
        "dyn": lambda t, p: oracle.dynamics_t1(*args(z, t1=t, precalc=p), z["tb"]),
    }
    for name, f in calls.items():
        assert rel(f(t_ok, z["precalc"]), refs[name](t_ok, z["precalc"])) < TOL
        with pytest.raises(ValueError, match="needs precalc map 6 of 5"):
            f(t_bad, z["precalc"])
        assert rel(f(t_bad, more), refs[name](t_bad, more)) < TOL
    # the segment (t2, tb) is not reached under early_only: tb = 4.0 leaves 33 steps only there
    t = np.array([0.0, 0.25])
    early = lambda tb: TB.four_time_8op(*args(z, t1=t), *o, True, False, tb)  # noqa: E731
    assert rel(early(4.0), oracle.four_time_8op(*args(z, t1=t), o, True, False, 4.0)) < TOL
    with pytest.raises(ValueError, match="precalc"):
        TB.four_time_8op(*args(z, t1=t), *o, False, False, 4.0)
    with pytest.raises(ValueError, match="precalc"):
        TB.four_time_8op(*args(z, t1=t), *o, False, True, 4.0)
    # a segment that would index the explicit maps below 1
    with pytest.raises(ValueError, match="before the first map"):
        TB.dynamics_t1(*args(z, t1=np.array([-0.2, 0.3])), z["tb"])
