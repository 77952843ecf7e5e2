"""The corners of the Hilbert-space no-PT kernel (lind_hilbert.hip, set up by setup_hilbert in pqd_host.cpp) that
tests/test_gpu_hilbert.py does not reach: dynamic LDS above 64 KiB, every count of jump operators and channels up to
the unrolled maxima, jump operators with few nonzeros (and none), both placements of the nonzero lists, a factor count
that moves with the pulse and comes close to its cap, and pulse samples on a raster that the time grid never hits.
GPU only.

Each case restates in Python, from the constants of the kernel's header, the quantity that puts it on its corner (LDS
bytes, bytes of the nonzero lists, the step bound theta per sub-step) and asserts the side of the threshold it means
to be on, so that a change of the helpers cannot move it off quietly.

Tolerances
  1e-12 relative to max|reference|: the project's figure for short no-PT runs (tests/test_gpu_parity.py,
      tests/test_gpu_hilbert.py); the reference is helpers.numpy_propagate (scipy expm of the full Liouvillian).
  1e-12 for |tr rho - 1| (identity column, trajectories without an MTO): the same figure, the trace is 1.
  1e-13 for the Hermiticity of the full readout: absolute, the elements of rho are at most 1 and each pair (a, b),
      (b, a) is the same sum in the kernel up to the order of the Taylor terms' rounding.
  byte equality where DESIGN.md promises the same bits: a trajectory's outputs in any batch, with its lists in LDS
      or in global memory.
  near the cap (theta = 0.97 * 4096): the reference is the closed form U rho U^dag from numpy.linalg.eigh (expm of the
      superoperator is itself a few 1e-13 off there). The bound NEAR_CAP_TOL = 5e-12 is 8 x the error measured on an
      MI355X (5.36e-13), rounded up to one significant digit, and must stay below n_factors N 2^-52, the worst-case linear growth of rounding
      over the run's Taylor factors (asserted in the test).
"""
import functools
import math

import numpy as np
import pytest

from pyaceqd_amd import _lib, engine
from pyaceqd_amd.engine import MTO, Grid, System, Trajectories
from tests import helpers as H

pytestmark = pytest.mark.gpu

# lind_hilbert.hip / pqd_common.h
HB_LMAX, HB_CSR_LDS, HB_SMAX = 8, 32768, 4096
LDS_DEFAULT = 65536  # dynamic LDS a kernel may ask for without hipFuncSetAttribute
TOL = 1e-12
NEAR_CAP_TOL = 5e-12  # 8 x 5.36e-13 measured on an MI355X (test_near_the_factor_cap) = 4.3e-12, rounded up


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _dense(rng, N):
    return rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))


# ------------------------------------------------------------------------------------------ restated quantities
def lds_bytes(N, nl_max):
    """R, T, Tn, K, Kd and one B per jump operator of the batch's largest system, 16-byte elements"""
    return (5 + nl_max) * N * N * 16


def list_bytes(sysd):
    """values, gamma conj(values) (16 B each) and columns (4 B) per nonzero, N + 1 row offsets per operator,
    rounded up to 16"""
    nnz = sum(int(np.count_nonzero(A)) for _, A in sysd.lindblad)
    return (nnz * 36 + len(sysd.lindblad) * (sysd.dim + 1) * 4 + 15) // 16 * 16


def lists_in_lds(systems):
    """placement is per batch: LDS when every system's lists fit (and there is a list at all)"""
    worst = max(list_bytes(s) for s in systems)
    return 0 < worst <= HB_CSR_LDS


def sample(sysd, t):
    """every channel at time t: linear interpolation, clamped at both ends (helpers.numpy_liouvillian's rule)"""
    u = (t - sysd.sample_t0) / sysd.sample_dt
    out = []
    for _, f in sysd.channels:
        if u <= 0:
            out.append(f[0])
        elif u >= len(f) - 1:
            out.append(f[-1])
        else:
            k = int(np.floor(u))
            out.append(f[k] + (u - k) * (f[k + 1] - f[k]))
    return out


def thetas(sysd, grid):
    """the kernel's step bound per sub-step, in the order the kernel takes them:
    theta = w (2 (|K0| + sum_p |f_p(t_mid)| (|Xs_p| + |Xt_p|)) + sum_k |gamma_k| |A_k|^2), Frobenius norms,
    K0 = -(i/hbar) H0 - 1/2 sum_k gamma_k A_k^dag A_k, Xs_p = -(i/hbar) X_p, Xt_p = -(i/hbar) X_p^dag"""
    fro = np.linalg.norm
    w = 0.5 * grid.dt / grid.n_sub
    K0 = -1j / sysd.hbar * np.asarray(sysd.H0, dtype=complex)
    nD = 0.0
    for g, A in sysd.lindblad:
        K0 = K0 - 0.5 * g * A.conj().T @ A
        nD += abs(g) * fro(A) ** 2
    nX = [2.0 * fro(X) / sysd.hbar for X, _ in sysd.channels]
    out = []
    for n in range(grid.n_steps):
        for h in range(2):
            for j in range(grid.n_sub):
                t = grid.ta + n * grid.dt + h * 0.5 * grid.dt + (j + 0.5) * w
                nk = fro(K0) + sum(abs(f) * x for f, x in zip(sample(sysd, t), nX))
                out.append(w * (2.0 * nk + nD))
    return out


def factors(theta):
    """Taylor factors per sub-step: s = ceil(theta), at least 1"""
    return max(1, math.ceil(theta))


# ------------------------------------------------------------------------------------------ builders
def _system(N, n_chan, n_lind, jump, seed, n_steps, n_sub=1):
    """random_system with dense jump operators, or with helpers.sparse_jump_ops in their place"""
    dense = jump == "dense"
    sysd, grid = H.random_system(N, n_chan=n_chan, n_lind=n_lind if dense else 0, seed=seed, n_steps=n_steps,
                                 n_sub=n_sub)
    if not dense:
        sysd.lindblad = H.sparse_jump_ops(N, n_lind, seed + 1000)
    assert len(sysd.lindblad) == n_lind and len(sysd.channels) == n_chan
    return sysd, grid


def degenerate_raster(sysd, grid, kind):
    """off-grid samples, or one of the rasters on which every midpoint is clamped: a single sample, samples that end
    before ta, samples that begin after the last step"""
    if kind == "offgrid":
        return H.offgrid_channels(sysd, grid)
    if kind == "one_sample":
        H.offgrid_channels(sysd, grid)
        sysd.channels = [(X, f[3:4].copy()) for X, f in sysd.channels]
        assert all(len(f) == 1 for _, f in sysd.channels)
    elif kind == "before":
        H.offgrid_channels(sysd, grid, cover=(-0.61, -0.07))
        assert sysd.sample_t0 + sysd.sample_dt * (len(sysd.channels[0][1]) - 1) < grid.ta
    elif kind == "after":
        H.offgrid_channels(sysd, grid, cover=(1.09, 1.57))
        assert sysd.sample_t0 > grid.ta + grid.n_steps * grid.dt
    else:
        raise ValueError(kind)
    return sysd


RASTERS = ["offgrid", "one_sample", "before", "after"]


def _two_windows(rng, N, n_steps):
    """windows [0, n] and [1, n], one MTO of kind 0 (on the second: the first keeps tr rho = 1)"""
    return Trajectories(np.array([0, 1]), np.array([n_steps, n_steps]), [MTO(1, 1, True, 0, _dense(rng, N) / N)])


def _three_kinds(rng, N, n_steps):
    A = lambda: _dense(rng, N) / N  # noqa: E731
    return Trajectories(np.array([0, 2]), np.array([n_steps, n_steps]),
                        [MTO(0, 0, True, 1, A()), MTO(0, 2, False, 2, A()), MTO(1, n_steps, True, 0, A()),
                         MTO(1, 1, True, 0, A())])


def _check(label, got, ref, tol=TOL):
    assert len(got) == len(ref)
    for t, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape
        err = rel(a, b)
        print(f"{label} traj {t}: rel err {err:.3e}")
        assert err < tol


# ------------------------------------------------------------------------------------------ 1. LDS above 64 KiB
@functools.lru_cache(maxsize=None)
def _lds_case(N, n_lind, jump, n_chan, n_steps):
    sysd, grid = _system(N, n_chan, n_lind, jump, seed=3 * N + n_lind, n_steps=n_steps)
    rng = np.random.default_rng(200 + N + n_lind)
    n_out = 256 if (N, n_lind, jump) == (24, 8, "sparse") else 3  # 256: the interface's limit, over 9 waves
    ops = [np.eye(N)] + [_dense(rng, N) for _ in range(n_out - 1)]
    tr = _two_windows(rng, N, n_steps)
    rho0 = H.random_rho(N)
    return sysd, grid, rho0, ops, tr, H.numpy_propagate(sysd, grid, rho0, ops, tr)


@pytest.mark.parametrize("N,n_lind,jump,n_chan,n_steps,in_lds",
                         [(24, 8, "sparse", 4, 2, True), (24, 3, "sparse", 2, 2, True), (18, 8, "sparse", 4, 3, True),
                          (24, 8, "dense", 1, 1, False)])
def test_lds_above_64k(N, n_lind, jump, n_chan, n_steps, in_lds):
    """the hipFuncSetAttribute branch of hb_launch: (24, 8 sparse) is the header's maximum with its lists in LDS,
    (24, 8 dense) is 119,808 B of matrices with its lists in global memory"""
    sysd, grid, rho0, ops, tr, ref = _lds_case(N, n_lind, jump, n_chan, n_steps)
    total = lds_bytes(N, n_lind) + (list_bytes(sysd) if in_lds else 0)
    print(f"N={N} n_lind={n_lind} {jump}: LDS {lds_bytes(N, n_lind)} + lists {list_bytes(sysd)} B "
          f"({'LDS' if in_lds else 'global'}), theta {max(thetas(sysd, grid)):.1f}")
    assert lds_bytes(N, n_lind) > LDS_DEFAULT and total <= 160 * 1024
    assert lists_in_lds([sysd]) == in_lds
    assert max(thetas(sysd, grid)) < HB_SMAX
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    _check(f"lds N={N} n_lind={n_lind} {jump}", got, ref)
    tr_err = float(np.max(np.abs(got[0][:, 0] - 1)))
    print(f"lds N={N} n_lind={n_lind} {jump}: |tr - 1| {tr_err:.3e}")
    assert tr_err < 1e-12


# ------------------------------------------------------------------------------------------ 2. counts at N = 9
@functools.lru_cache(maxsize=None)
def _count_case(n_lind, n_chan, jump, n_sub):
    N, n_steps = 9, 6
    sysd, grid = _system(N, n_chan, n_lind, jump, seed=31 + 5 * n_lind + n_chan, n_steps=n_steps, n_sub=n_sub)
    rng = np.random.default_rng(300 + n_lind)
    ops = [np.eye(N), _dense(rng, N), _dense(rng, N)]
    tr = _three_kinds(rng, N, n_steps)
    rho0 = H.random_rho(N)
    return sysd, grid, rho0, ops, tr, H.numpy_propagate(sysd, grid, rho0, ops, tr)


@pytest.mark.parametrize("n_sub", [1, 2])
@pytest.mark.parametrize("jump", ["dense", "sparse"])
@pytest.mark.parametrize("n_lind,n_chan", [(1, 1), (3, 3), (4, 4), (5, 4), (8, 4), (8, 0), (0, 4)])
def test_operator_and_channel_counts(n_lind, n_chan, jump, n_sub):
    """81 threads: two waves, the second mostly idle; every unrolled slot of both loops up to HB_LMAX = 8 and 4
    channels, and both loops empty"""
    sysd, grid, rho0, ops, tr, ref = _count_case(n_lind, n_chan, jump, n_sub)
    assert n_lind <= HB_LMAX and lds_bytes(9, n_lind) <= LDS_DEFAULT
    assert lists_in_lds([sysd]) == (n_lind > 0)
    if jump == "sparse" and n_lind >= 5:
        assert not np.any(sysd.lindblad[4][1])  # the operator without a nonzero
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    _check(f"counts n_lind={n_lind} n_chan={n_chan} {jump} n_sub={n_sub}", got, ref)


# ------------------------------------------------------------------------------------------ 3. both placements
@pytest.mark.parametrize("N,in_lds", [(10, True), (11, False)])
def test_both_list_placements_with_eight_dense_operators(N, in_lds):
    """8 dense operators: 29,152 B of lists at N = 10 (LDS), 35,232 B at N = 11 (global memory)"""
    n_steps = 4
    sysd, grid = _system(N, 2, 8, "dense", seed=50 + N, n_steps=n_steps)
    print(f"N={N}: lists {list_bytes(sysd)} B")
    assert list_bytes(sysd) == {10: 29152, 11: 35232}[N]
    assert lists_in_lds([sysd]) == in_lds and (list_bytes(sysd) <= HB_CSR_LDS) == in_lds
    rng = np.random.default_rng(400 + N)
    ops = [np.eye(N), _dense(rng, N)]
    tr = _three_kinds(rng, N, n_steps)
    rho0 = H.random_rho(N)
    _check(f"placement N={N}", engine.propagate(sysd, grid, rho0, ops, tr),
           H.numpy_propagate(sysd, grid, rho0, ops, tr))


# ------------------------------------------------------------------------------------------ 4. placement and bits
def test_list_placement_does_not_change_bits():
    """A's trajectory alone reads its lists from LDS (and B_0 .. B_5); in a batch with B every list is in global
    memory (and the LDS holds B_0 .. B_7): the same bits, as DESIGN.md and the kernel's header promise"""
    N, n_steps = 11, 4
    A, grid = _system(N, 2, 6, "sparse", seed=61, n_steps=n_steps)
    B, _ = _system(N, 2, 8, "dense", seed=62, n_steps=n_steps)
    assert lists_in_lds([A]) and not lists_in_lds([A, B])
    rng = np.random.default_rng(410)
    ops = [np.eye(N), _dense(rng, N), _dense(rng, N)]
    rho0 = H.random_rho(N)
    op = _dense(rng, N) / N
    one = Trajectories(np.array([1]), np.array([n_steps]), [MTO(0, 2, False, 0, op)])
    two = Trajectories(np.array([1, 0]), np.array([n_steps, n_steps]), [MTO(0, 2, False, 0, op)],
                       system=np.array([0, 1]))
    alone = engine.propagate(A, grid, rho0, ops, one)[0]
    batch = engine.propagate([A, B], grid, rho0, ops, two)
    _check("placement bits A", [alone], H.numpy_propagate(A, grid, rho0, ops, one))
    _check("placement bits B", [batch[1]], H.numpy_propagate(B, grid, rho0, ops, H.simple_traj(n_steps)))
    assert alone.tobytes() == batch[0].tobytes()


# ------------------------------------------------------------------------------------------ 5. unlike systems
def test_mixed_batch_of_unlike_systems():
    """(n_lind, n_chan) = (0, 0), (8, 4) sparse, (2, 1) dense, (5, 3) sparse with the all-zero operator; different
    numbers of samples and sample spacings; ragged windows, one of a single row after an MTO before it"""
    N, n_steps = 8, 6
    spec = [(0, 0, "dense", None, None), (8, 4, "sparse", (0.23, 0.78), 0.0137 * np.pi),
            (2, 1, "dense", (0.10, 0.60), 0.0211 * np.pi), (5, 3, "sparse", (0.40, 0.95), 0.0089 * np.pi)]
    systems = []
    for k, (n_lind, n_chan, jump, cover, sdt) in enumerate(spec):
        sysd, grid = _system(N, n_chan, n_lind, jump, seed=70 + k, n_steps=n_steps, n_sub=2)
        if n_chan:
            H.offgrid_channels(sysd, grid, cover=cover, sdt=sdt)
        systems.append(sysd)
    ns = [len(s.channels[0][1]) for s in systems[1:]]
    assert len(set(ns)) == 3 and len({s.sample_dt for s in systems[1:]}) == 3
    assert len({int(np.count_nonzero(np.stack([A for _, A in s.lindblad]))) for s in systems[1:]}) == 3  # unlike nnz
    assert not np.any(systems[3].lindblad[4][1]) and lists_in_lds(systems)
    rng = np.random.default_rng(420)
    ops = [np.eye(N), _dense(rng, N)]
    rho0 = H.random_rho(N)
    tsys = np.array([1, 0, 3, 2, 1, 3, 3])
    begins = np.array([0, 1, 0, 2, 4, 3, 0])
    ends = np.array([6, 6, 4, 6, 4, 6, 5])
    steps = [1, 2, 3, 0, 2, 2, 3]  # trajectory 4: out_begin == out_end == 4, its MTO at step 2
    mto_of = {t: MTO(t, steps[t], bool(t % 2), t % 3, _dense(rng, N) / N) for t in range(7)}
    tr = Trajectories(begins, ends, [mto_of[t] for t in range(7)], system=tsys)
    batch = engine.propagate(systems, grid, rho0, ops, tr)
    refs = {}
    for k in range(4):  # one reference run per system, over its trajectories
        mine = [t for t in range(7) if tsys[t] == k]
        sub = Trajectories(begins[mine], ends[mine],
                           [MTO(q, mto_of[t].step, mto_of[t].before, mto_of[t].kind, mto_of[t].op)
                            for q, t in enumerate(mine)])
        refs.update(zip(mine, H.numpy_propagate(systems[k], grid, rho0, ops, sub)))
    for t in range(7):
        m = mto_of[t]
        one = Trajectories(begins[t: t + 1], ends[t: t + 1], [MTO(0, m.step, m.before, m.kind, m.op)])
        single = engine.propagate(systems[tsys[t]], grid, rho0, ops, one)[0]
        ref = refs[t]
        err = rel(batch[t], ref)
        print(f"mixed batch traj {t} (system {tsys[t]}): rel err {err:.3e}")
        assert batch[t].shape == ref.shape == (ends[t] - begins[t] + 1, 2)
        assert err < TOL
        assert single.tobytes() == batch[t].tobytes(), t


# ------------------------------------------------------------------------------------------ 6. full readout
def test_full_density_matrix_readout():
    """n_out = 169 unit matrices |a><b| at N = 13: out[a 13 + b] = rho[b, a], three waves of outputs"""
    N, n_steps = 13, 5
    sysd, grid = _system(N, 2, 3, "sparse", seed=81, n_steps=n_steps)
    ops = [H.ketbra(N, a, b) for a in range(N) for b in range(N)]
    rho0 = H.random_rho(N)
    tr = H.simple_traj(n_steps)
    got = engine.propagate(sysd, grid, rho0, ops, tr)[0]
    ref = H.numpy_propagate(sysd, grid, rho0, ops, tr)[0]
    assert got.shape == ref.shape == (n_steps + 1, N * N)
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    rho = got.reshape(n_steps + 1, N, N).transpose(0, 2, 1)
    herm = float(np.max(np.abs(rho - rho.conj().transpose(0, 2, 1))))
    tr_err = float(np.max(np.abs(np.trace(rho, axis1=1, axis2=2) - 1)))
    print(f"full readout: rel err {err:.3e}, Hermiticity {herm:.3e}, |tr - 1| {tr_err:.3e}")
    assert err < TOL
    assert herm < 1e-13
    assert tr_err < 1e-12


# ------------------------------------------------------------------------------------------ 7. a moving factor count
def test_factor_count_moves_with_the_pulse():
    """H0 scaled down and one channel scaled up: s = 1 before and after the samples' zero ends, above 16 at the peak,
    changing from sub-step to sub-step in between (and the degree with theta / s)"""
    N, n_steps = 8, 8
    sysd, grid = _system(N, 1, 2, "sparse", seed=91, n_steps=n_steps, n_sub=2)
    sysd.H0 = sysd.H0 * 0.05
    H.offgrid_channels(sysd, grid, floor=0.0)
    sysd.channels = [(X * 25.0, f) for X, f in sysd.channels]
    s = [factors(th) for th in thetas(sysd, grid)]
    print(f"factor counts per sub-step: {s}")
    assert len(s) == 4 * n_steps and len(set(s)) >= 3 and min(s) == 1 and max(s) > 16 and max(s) < HB_SMAX
    rng = np.random.default_rng(430)
    ops = [np.eye(N), _dense(rng, N)]
    tr = _three_kinds(rng, N, n_steps)
    rho0 = H.random_rho(N)
    _check("moving s", engine.propagate(sysd, grid, rho0, ops, tr), H.numpy_propagate(sysd, grid, rho0, ops, tr))


# ------------------------------------------------------------------------------------------ 8, 9. the cap
def _cap_system(frac):
    """time-independent Hermitian H0 at N = 8 with theta = frac * HB_SMAX per sub-step"""
    N = 8
    rng = np.random.default_rng(440)
    Hh = _dense(rng, N)
    Hh = 0.5 * (Hh + Hh.conj().T)
    grid = Grid(0.0, 0.1, 2, 1)
    sysd = System(dim=N, H0=Hh)
    sysd.H0 = Hh * (frac * HB_SMAX / thetas(sysd, grid)[0])
    return sysd, grid


def test_near_the_factor_cap():
    """theta = 0.97 * 4096 against U rho U^dag from eigh. Measured on an MI355X: 5.36e-13 relative
    (profiles/r11/hilbert_envelope); NEAR_CAP_TOL = 5e-12 is 8 x that, rounded up to one digit, and below
    n_factors N 2^-52 = 15,896 x 8 x 2^-52 = 2.8e-11. (scipy's expm of the superoperator is 5.2e-13 from the same
    closed form on the CPU: reference and kernel are equally far from it.)"""
    sysd, grid = _cap_system(0.97)
    N = sysd.dim
    th = thetas(sysd, grid)
    assert len(th) == 4 and all(0.96 * HB_SMAX < x < 0.98 * HB_SMAX for x in th)
    n_factors = sum(factors(x) for x in th)
    assert NEAR_CAP_TOL < n_factors * N * 2.0 ** -52
    rng = np.random.default_rng(441)
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    E, V = np.linalg.eigh(sysd.H0)
    ref = []
    for n in range(grid.n_steps + 1):
        U = (V * np.exp(-1j * E * (n * grid.dt) / sysd.hbar)) @ V.conj().T
        rho = U @ rho0 @ U.conj().T
        ref.append([np.trace(O @ rho) for O in ops])
    ref = np.array(ref)
    got = engine.propagate(sysd, grid, rho0, ops, H.simple_traj(grid.n_steps))[0]
    err = rel(got, ref)
    print(f"near the cap: theta {th[0]:.1f}, {n_factors} factors, rel err vs eigh {err:.3e} "
          f"(bound {NEAR_CAP_TOL:.1e}, condition {n_factors * N * 2.0 ** -52:.2e})")
    assert got.shape == ref.shape and err < NEAR_CAP_TOL


def test_refusal_above_the_factor_cap():
    sysd, grid = _cap_system(1.03)
    N = sysd.dim
    assert all(1.02 * HB_SMAX < x < 1.04 * HB_SMAX for x in thetas(sysd, grid))
    with pytest.raises(_lib.PQDError) as ei:
        engine.propagate(sysd, grid, H.random_rho(N), [np.eye(N)], H.simple_traj(grid.n_steps))
    assert ei.value.code == _lib.PQD_ERR_UNSUPPORTED, ei.value
    assert "4096" in str(ei.value) and "lower dt or raise n_sub" in str(ei.value)
    # the context stays usable
    ok, g = H.random_system(N, n_steps=3, seed=3)
    ops = [np.eye(N)]
    out = engine.propagate(ok, g, H.random_rho(N), ops, H.simple_traj(3))
    _check("after the refusal", out, H.numpy_propagate(ok, g, H.random_rho(N), ops, H.simple_traj(3)))


# ------------------------------------------------------------------------------------------ 10. off-grid samples
@functools.lru_cache(maxsize=None)
def _raster_case(kind, n_sub):
    N, n_steps = 8, 12
    sysd, grid = _system(N, 2, 2, "dense", seed=95, n_steps=n_steps, n_sub=n_sub)
    degenerate_raster(sysd, grid, kind)
    rng = np.random.default_rng(450)
    ops = [np.eye(N), _dense(rng, N)]
    tr = _three_kinds(rng, N, n_steps)
    rho0 = H.random_rho(N)
    return sysd, grid, rho0, ops, tr, H.numpy_propagate(sysd, grid, rho0, ops, tr)


@pytest.mark.parametrize("n_sub", [1, 2])
@pytest.mark.parametrize("kind", RASTERS)
def test_offgrid_sampling(kind, n_sub):
    """samples on a raster incommensurate with dt over the middle of the run: midpoints between samples, before the
    first and after the last; and the rasters on which every midpoint is clamped"""
    sysd, grid, rho0, ops, tr, ref = _raster_case(kind, n_sub)
    if kind == "offgrid":
        w = 0.5 * grid.dt / n_sub
        u = (grid.ta + (np.arange(2 * n_sub * grid.n_steps) + 0.5) * w - sysd.sample_t0) / sysd.sample_dt
        ns = len(sysd.channels[0][1])
        inside = u[(u > 0) & (u < ns - 1)]
        frac = np.abs(inside - np.round(inside))
        print(f"off-grid n_sub={n_sub}: {len(inside)} midpoints inside, {np.sum(u <= 0)} below, "
              f"{np.sum(u >= ns - 1)} above, closest to a sample {frac.min():.4f} of a spacing")
        assert len(inside) >= 10 and np.sum(u <= 0) >= 5 and np.sum(u >= ns - 1) >= 5 and frac.min() > 1e-3
        assert abs(sysd.channels[0][1][0]) > 0.1 and abs(sysd.channels[0][1][-1]) > 0.1
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    _check(f"raster {kind} n_sub={n_sub}", got, ref)
