"""The Hilbert-space no-PT kernel (lind_hilbert.hip, PQD_PATH_HILBERT): dim 7..24 against the numpy restatement with
scipy's expm of the full Liouvillian (tests/helpers.numpy_propagate), and dim <= 6 forced onto the path against the
C oracle. GPU only.

Tolerances: 1e-12 relative to max|reference| (the project's figure for short no-PT runs, tests/test_gpu_parity.py),
1e-11 against closed-form solutions through the drop-in wrappers (test_cw_drive_matches_exact_lindblad_solution's
figure), 1e-13 for the trapezoid reduction (as test_gpu_parity's trapz test). Bit-equality where the issue is
reproducibility: a trajectory's outputs do not depend on the batch it runs in.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pyaceqd_amd import _lib, engine
from pyaceqd_amd.engine import MTO, Grid, System, Trajectories
from tests import helpers as H

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _dense(rng, N):
    return rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))


def _mtos(rng, N, n_steps):
    """all three kinds, both `before` flags, one at step 0, one at the last step, two in one (traj, step, before) slot
    (their order matters: A rho A^dag then B rho is not B (A rho A^dag) in the other order)"""
    A = lambda: _dense(rng, N) / N  # noqa: E731
    return [MTO(0, 0, True, 1, A()), MTO(0, 2, False, 2, A()), MTO(1, n_steps, True, 0, A()),
            MTO(1, 1, True, 0, A()), MTO(1, 1, True, 1, A())]


@functools.lru_cache(maxsize=None)
def _parity_case(N, n_sub, scale):
    """system, grid, inputs and the reference of one parity case (computed once, read-only afterwards)"""
    n_steps = 3 if N == 24 else 8
    sysd, grid = H.random_system(N, n_chan=2, n_lind=2, n_steps=n_steps, dt=0.1, n_sub=n_sub, seed=N)
    sysd.H0 = sysd.H0 * scale
    rng = np.random.default_rng(100 + N)
    tr = Trajectories(np.array([0, 2]), np.array([n_steps, n_steps]), _mtos(rng, N, n_steps))
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    return sysd, grid, rho0, ops, tr, H.numpy_propagate(sysd, grid, rho0, ops, tr)


# ------------------------------------------------------------------------------------------ 1. parity above dim 6
@pytest.mark.parametrize("n_sub", [1, 2])
@pytest.mark.parametrize("N,scale", [(7, 1), (8, 1), (13, 1), (18, 1), (24, 1), (8, 20)])
def test_parity_above_dim_6(N, scale, n_sub):
    """7: first above the old limit; 8: N^2 = 64; 13, 18: N^2 no multiple of the workgroup; 24: the LDS maximum;
    H0 x 20 at N = 8: many Taylor factors per sub-step (s > 1)"""
    sysd, grid, rho0, ops, tr, ref = _parity_case(N, n_sub, scale)
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    assert len(got) == len(ref) == 2
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        print(f"N={N} scale={scale} n_sub={n_sub}: rel err {rel(a, b):.3e}")
        assert rel(a, b) < 1e-12


def test_plan_reports_the_hilbert_path():
    sysd, grid, rho0, ops, tr, ref = _parity_case(8, 1, 1)
    plan = engine.Plan(sysd, grid, rho0, ops, tr)
    d = plan.describe()
    assert d["path"] == str(_lib.PQD_PATH_HILBERT) and d["BT"] == "1" and d["win"] == "0" and d["lean"] == "0"
    assert plan.info()[1] == 1 and not plan.windows() and not plan.sweep_lean()
    keys_nopt = list(engine.Plan(*H.random_system(3, n_steps=4), H.random_rho(3), [np.eye(3)],
                                 H.simple_traj(4)).describe())
    assert list(d) == keys_nopt  # the same keys in the same order as an existing plan's line
    for rebuild in (True, False):  # rebuild_free is ignored: there are no free propagators
        plan.execute(rebuild_free=rebuild)
        for a, b in zip(plan.download(), ref):
            assert rel(a, b) < 1e-12
    ms_free, ms_sweep, n = plan.timing()
    assert ms_free == 0.0 and ms_sweep > 0.0 and n == 2


# ------------------------------------------------------------------------------------------ 2. edges at N = 8
@pytest.mark.parametrize("n_chan,n_lind", [(2, 0), (0, 2), (0, 0)])
def test_no_jump_operators_or_no_channels(n_chan, n_lind):
    N = 8
    sysd, grid = H.random_system(N, n_chan=n_chan, n_lind=n_lind, n_steps=6, seed=21 + n_chan + 3 * n_lind)
    rng = np.random.default_rng(3)
    ops = [_dense(rng, N), np.eye(N)]
    rho0 = H.random_rho(N)
    tr = H.simple_traj(6, mtos=[MTO(0, 3, False, 0, _dense(rng, N) / N)])
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    ref = H.numpy_propagate(sysd, grid, rho0, ops, tr)
    assert rel(got[0], ref[0]) < 1e-12


def test_zero_steps_gives_the_initial_expectation():
    N = 8
    sysd, _ = H.random_system(N, n_steps=1, seed=4)
    rng = np.random.default_rng(4)
    ops = [_dense(rng, N) for _ in range(2)]
    rho0 = H.random_rho(N)
    out = engine.propagate(sysd, Grid(0.0, 0.1, 0), rho0, ops, Trajectories(np.array([0]), np.array([0])))
    want = np.array([[np.trace(O @ rho0) for O in ops]])
    assert out[0].shape == (1, 2) and rel(out[0], want) < 1e-12


def test_more_than_eight_outputs():
    N = 8
    sysd, grid = H.random_system(N, n_steps=5, seed=6)
    rng = np.random.default_rng(6)
    ops = [_dense(rng, N) for _ in range(9)]
    rho0 = H.random_rho(N)
    tr = H.simple_traj(5)
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    ref = H.numpy_propagate(sysd, grid, rho0, ops, tr)
    assert got[0].shape == (6, 9) and rel(got[0], ref[0]) < 1e-12


def test_no_dynamics_leaves_every_row_bit_equal():
    """H0 = 0, no jump operators, no channels: L = 0, every Taylor term is exactly zero and rho never changes"""
    N = 8
    sysd = System(dim=N, H0=np.zeros((N, N)))
    rng = np.random.default_rng(7)
    ops = [_dense(rng, N) for _ in range(3)]
    out = engine.propagate(sysd, Grid(0.0, 0.1, 7, 2), H.random_rho(N), ops, H.simple_traj(7))[0]
    assert out.shape == (8, 3) and np.all(np.isfinite(out))
    for row in out[1:]:
        assert row.tobytes() == out[0].tobytes()


# ------------------------------------------------------------------------------------------ 3. forced path, dim <= 6
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import oracle
from pyaceqd_amd import engine
from pyaceqd_amd.engine import MTO, Trajectories
from tests import helpers as H
res = {}
for N in (2, 3, 6):
    sysd, grid = H.random_system(N, n_steps=20, seed=40 + N)
    rng = np.random.default_rng(N)
    A = lambda: (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) / N
    mt = [MTO(0, 0, True, 1, A()), MTO(0, 7, False, 2, A()), MTO(1, 20, True, 0, A()), MTO(1, 5, True, 0, A()),
          MTO(1, 5, True, 1, A())]
    tr = Trajectories(np.array([0, 3]), np.array([20, 20]), mt)
    ops = [H.ketbra(N, 0, 0), H.ketbra(N, N - 1, 0), np.eye(N)]
    rho0 = H.random_rho(N)
    plan = engine.Plan(sysd, grid, rho0, ops, tr)
    plan.execute()
    got = plan.download()
    ref = oracle.propagate(sysd, grid, rho0, ops, tr)
    err = max(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(got, ref))
    res[str(N)] = {"path": plan.describe()["path"], "err": err}
print("RESULT " + json.dumps(res))
"""


def test_forced_path_matches_the_oracle_below_dim_7(monkeypatch):
    """PQD_HILBERT=1 is read once per plan creation; a fresh child process keeps the switch away from this one"""
    env = dict(os.environ, PQD_HILBERT="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for N in ("2", "3", "6"):
        print(f"N={N}: path {res[N]['path']} rel err vs oracle {res[N]['err']:.3e}")
        assert res[N]["path"] == str(_lib.PQD_PATH_HILBERT)
        assert res[N]["err"] < 1e-12
    # without the switch the same kind of plan stays on the one-wave no-PT kernel
    monkeypatch.delenv("PQD_HILBERT", raising=False)
    sysd, grid = H.random_system(3, n_steps=20, seed=43)
    plan = engine.Plan(sysd, grid, H.random_rho(3), [np.eye(3)], H.simple_traj(20))
    assert plan.describe()["path"] == str(_lib.PQD_PATH_NOPT)


# ------------------------------------------------------------------------------------------ 4. batch independence
def test_mixed_batch_is_bit_equal_to_single_runs():
    N, n_steps = 8, 6
    systems = [H.random_system(N, n_steps=n_steps, seed=60 + k, n_lind=1 + k)[0] for k in range(3)]
    grid = Grid(0.0, 0.1, n_steps)
    rng = np.random.default_rng(8)
    ops = [_dense(rng, N) for _ in range(2)]
    rho0 = H.random_rho(N)
    tsys = np.array([2, 0, 1, 1, 0, 2, 0])
    begins = np.array([0, 1, 0, 2, 0, 3, 0])
    ends = np.array([6, 6, 4, 6, 5, 6, 6])
    mto_of = {t: [MTO(t, int(1 + t % 4), bool(t % 2), t % 3, _dense(rng, N) / N)] for t in range(7)}
    tr = Trajectories(begins, ends, [m for t in range(7) for m in mto_of[t]], system=tsys)
    batch = engine.propagate(systems, grid, rho0, ops, tr)
    for t in range(7):
        m = mto_of[t][0]
        one = Trajectories(begins[t: t + 1], ends[t: t + 1], [MTO(0, m.step, m.before, m.kind, m.op)])
        single = engine.propagate(systems[tsys[t]], grid, rho0, ops, one)[0]
        assert single.tobytes() == batch[t].tobytes(), t


def test_600_identical_trajectories():
    """more workgroups than CUs: all bit-equal to each other and within 1e-12 of the reference"""
    N, n_steps, n_traj = 7, 4, 600
    sysd, grid = H.random_system(N, n_steps=n_steps, seed=70)
    rng = np.random.default_rng(9)
    ops = [_dense(rng, N) for _ in range(2)]
    rho0 = H.random_rho(N)
    A = _dense(rng, N) / N
    tr = Trajectories(np.zeros(n_traj, dtype=int), np.full(n_traj, n_steps), [MTO(t, 2, True, 0, A) for t in range(n_traj)])
    got = engine.propagate(sysd, grid, rho0, ops, tr)
    one = Trajectories(np.array([0]), np.array([n_steps]), [MTO(0, 2, True, 0, A)])
    ref = H.numpy_propagate(sysd, grid, rho0, ops, one)[0]
    assert rel(got[0], ref) < 1e-12
    first = got[0].tobytes()
    assert all(g.tobytes() == first for g in got)


# ------------------------------------------------------------------------------------------ 5. the other entry points
def test_table_and_trapz_on_this_path():
    N, n_steps = 8, 10
    sysd, grid = H.random_system(N, n_steps=n_steps, seed=80)
    rng = np.random.default_rng(10)
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    tr = Trajectories(np.array([0, 4, 9]), np.array([10, 10, 10]), [MTO(1, 3, False, 1, _dense(rng, N) / N)])
    flat = engine.propagate(sysd, grid, rho0, ops, tr)
    tabs = engine.propagate_table(sysd, grid, rho0, ops, tr)
    for a, b in zip(tabs, engine.tables_from_outputs(flat, tr, grid)):
        np.testing.assert_array_equal(a, b)
    kh, kt, dx = [0, 2, 1], [1, 2, 0], 0.1
    got = engine.propagate_trapz(sysd, grid, rho0, ops, tr, kh, kt, dx)
    assert got.shape == (3, 3)
    for t, y in enumerate(flat):
        for q in range(3):
            L = y.shape[0]
            want = 0.0 if L < 2 else dx * (0.5 * y[0, kh[q]] + y[1: L - 1, kt[q]].sum() + 0.5 * y[L - 1, kt[q]])
            assert abs(got[t, q] - want) <= 1e-13 * max(1.0, abs(want))


# ------------------------------------------------------------------------------------------ 6. refusals
def _unsupported(fn, *a, **k):
    with pytest.raises(_lib.PQDError) as ei:
        fn(*a, **k)
    assert ei.value.code == _lib.PQD_ERR_UNSUPPORTED, ei.value
    return str(ei.value)


def test_refusals_name_the_limit():
    rho = lambda N: H.random_rho(N)  # noqa: E731
    s25 = System(dim=25, H0=np.zeros((25, 25)))
    assert "dim 25 not in [2, 24]" in _unsupported(engine.propagate, s25, Grid(0, 0.1, 2), rho(25), [np.eye(25)],
                                                   H.simple_traj(2))
    s9, g9 = H.random_system(8, n_lind=9, n_steps=2, seed=1)
    assert "n_lind 9" in _unsupported(engine.propagate, s9, g9, rho(8), [np.eye(8)], H.simple_traj(2))
    s8, g8 = H.random_system(8, n_steps=2, seed=2)
    assert "dim 8 not in [2, 6]" in _unsupported(engine.free_propagators, s8, g8)
    from pyaceqd_amd import pt as ptmod
    pt = ptmod.random_pt(8, 16, D=4, n_slices=3, seed=1, eps=0.1)
    assert "dim 8" in _unsupported(engine.propagate, s8, g8, rho(8), [np.eye(8)], H.simple_traj(2), pt=pt)


def test_nan_in_h0_is_a_numeric_error():
    """the step bound is not finite: the kernel takes one factor of the maximum degree, ends, and synchronize finds
    the non-finite outputs (finite loop counts on every input)"""
    s8, g8 = H.random_system(8, n_steps=3, seed=3)
    s8.H0 = s8.H0.copy()
    s8.H0[2, 5] = np.nan
    with pytest.raises(_lib.NumericError):
        engine.propagate(s8, g8, H.random_rho(8), [np.eye(8)], H.simple_traj(3))
    # the context stays usable
    ok, g = H.random_system(8, n_steps=3, seed=3)
    out = engine.propagate(ok, g, H.random_rho(8), [np.eye(8)], H.simple_traj(3))[0]
    assert np.all(np.isfinite(out))


# ------------------------------------------------------------------------------------------ 7. through the drop-in
def test_jaynes_cummings_vacuum_rabi_oscillation():
    """one excitation shared between the dot and a lossless resonant mode: <|1><1|>(t) = cos^2(g t / hbar)"""
    from pyaceqd_amd.constants import hbar
    from pyaceqd_amd.two_level_system.tls import tls_photon
    g = 0.06
    t, pop = tls_photon(0, 20, dt=0.1, delta_cx1=0, cav_loss1=0, cav_coupl1=g, lindblad=False,
                        initial="|1><1|_2 otimes |0><0|_3", output_ops=["|1><1|_2 otimes Id_3"])
    assert len(t) == 201
    want = np.cos(g * t.real / hbar) ** 2
    print(f"Jaynes-Cummings: max abs err {np.max(np.abs(pop - want)):.3e}")
    assert rel(pop, want) < 1e-11


def test_cavity_decay_is_exponential():
    from pyaceqd_amd.two_level_system.tls import tls_photon
    kappa = 0.3
    t, n = tls_photon(0, 20, dt=0.1, delta_cx1=0, cav_loss1=kappa, cav_coupl1=0, lindblad=False,
                      initial="|0><0|_2 otimes |1><1|_3", output_ops=["Id_2 otimes n_3"])
    want = np.exp(-kappa * t.real)
    print(f"cavity decay: max abs err {np.max(np.abs(n - want)):.3e}")
    assert rel(n, want) < 1e-11


@pytest.mark.parametrize("model", ["tls_photons", "biexciton_photons_extended"])
def test_dim_18_models_match_the_numpy_reference(model, monkeypatch):
    from pyaceqd_amd.general_system import general_system as gs
    from pyaceqd_amd.pulses import ChirpedPulse
    if model == "tls_photons":
        from pyaceqd_amd.two_level_system.tls import tls_photons as fn
    else:
        from pyaceqd_amd.four_level_system.linear import biexciton_photons_extended as fn
    seen = {}
    real = gs.propagate_table

    def spy(system, grid, rho0, out_ops, traj, pt=None, ctx=None):
        seen.update(system=system, grid=grid, rho0=rho0, out_ops=out_ops, traj=traj)
        return real(system, grid, rho0, out_ops, traj, pt=pt, ctx=ctx)
    monkeypatch.setattr(gs, "propagate_table", spy)
    pulse = ChirpedPulse(tau_0=0.4, e_start=0.0, e0=2.0, t0=1.0, alpha=0.5)
    res = fn(0, 2, pulse, dt=0.1, lindblad=True)
    assert seen["system"].dim == 18 and seen["grid"].n_steps == 20
    ref = H.numpy_propagate(seen["system"], seen["grid"], seen["rho0"], seen["out_ops"], seen["traj"])[0]
    got = np.asarray(res[1:]).T
    print(f"{model}: rel err {rel(got, ref):.3e}")
    assert got.shape == ref.shape and rel(got, ref) < 1e-12
    assert np.max(np.abs(got[:, 0] - 1)) > 1e-3  # the pulse did drive the system


def test_phonons_above_dim_6_are_refused():
    from pyaceqd_amd.pulses import ChirpedPulse
    from pyaceqd_amd.two_level_system.tls import tls_photons
    with pytest.raises(NotImplementedError, match="phonons"):
        tls_photons(0, 2, ChirpedPulse(tau_0=0.4, e_start=0.0, e0=2.0, t0=1.0), dt=0.1, phonons=True)
