"""The Hilbert-space kernel with a process tensor (lind_hilbert_pt.hip, PQD_PATH_HILBERT_PT): the opt-in wide_pt=True
at dim 7..24 against the numpy restatement (tests/helpers.numpy_propagate with a PT), at dim <= 6 against the C oracle
and the existing sweep, and through the drop-in wrappers. GPU only.

Tolerances: 1e-12 relative to max|reference| (the project's figure, tests/test_gpu_hilbert.py; the two CPU
restatements agree to 2e-15 on such inputs), 1e-13 for the trapezoid reduction, 1e-10 where two different paths each
pinned to 1e-11 by the exact-solution tests are compared. Bit-equality where the issue is reproducibility: a
trajectory's outputs depend neither on the batch nor on the number of bond slices in flight (PQD_HBPT_G).
Every measured error is printed.
"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from pyaceqd_amd import _lib, engine
from pyaceqd_amd import pt as ptmod
from pyaceqd_amd import ptgen
from pyaceqd_amd.engine import MTO, Grid, Trajectories
from tests import helpers as H

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _dense(rng, N):
    return rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))


def _mtos(rng, N, n_steps):
    """as tests/test_gpu_hilbert.py: all three kinds, both `before` flags, one at step 0, one at the last step, two in
    one (traj, step, before) slot"""
    A = lambda: _dense(rng, N) / N  # noqa: E731
    return [MTO(0, 0, True, 1, A()), MTO(0, 2, False, 2, A()), MTO(1, n_steps, True, 0, A()),
            MTO(1, 1, True, 0, A()), MTO(1, 1, True, 1, A())]


@functools.lru_cache(maxsize=None)
def _case(N, chi, D, n_sub=1, scale=1, n_init=None):
    """system, grid, inputs, PT and the numpy reference of one parity case (computed once, read-only afterwards): two
    trajectories, begins 0 and 2, ends n_steps - 1 and n_steps, MTOs of every kind and flag"""
    n_steps = 3 if N >= 18 else 6
    sysd, grid = H.random_system(N, n_chan=2, n_lind=2, n_steps=n_steps, dt=0.1, n_sub=n_sub, seed=N)
    sysd.H0 = sysd.H0 * scale
    rng = np.random.default_rng(200 + N + chi)
    tr = Trajectories(np.array([0, 2]), np.array([n_steps - 1, n_steps]), _mtos(rng, N, n_steps))
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    pt = ptmod.random_pt(N, chi, D, n_slices=4, seed=chi, eps=0.1)
    if n_init is not None:
        pt.n_init = n_init
    return sysd, grid, rho0, ops, tr, pt, H.numpy_propagate(sysd, grid, rho0, ops, tr, pt=pt)


def _check(got, ref, what, tol=1e-12):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape
        print(f"{what} trajectory {k}: rel err {rel(a, b):.3e}")
        assert rel(a, b) < tol


# ------------------------------------------------------------------------------------------ 1. parity, dim 7..24
SHAPES = [(7, 5, 4), (8, 16, 4), (9, 33, 9), (13, 16, 4), (18, 8, 4), (24, 4, 4), (7, 1, 1), (7, 130, 4), (7, 256, 4)]


@pytest.mark.parametrize("N,chi,D,n_sub", [s + (1,) for s in SHAPES] + [s + (2,) for s in SHAPES[:3]])
def test_parity_with_the_numpy_reference(N, chi, D, n_sub):
    """(7, 5): N^2 below a wave, odd chi; (9, 33): chi past a pad width, odd N^2, D = 9; 24: 8 jump operators would be
    the LDS maximum, G = 1 at this size either way; chi 1, above 128, and the largest bond"""
    sysd, grid, rho0, ops, tr, pt, ref = _case(N, chi, D, n_sub)
    got = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    _check(got, ref, f"N={N} chi={chi} D={D} n_sub={n_sub}")


def test_parity_at_24_with_eight_jump_operators():
    """the LDS maximum: 13 matrices of 24 x 24 and the nonzero lists, one slice in flight"""
    N = 24
    sysd, grid = H.random_system(N, n_chan=2, n_lind=0, n_steps=3, dt=0.1, seed=24)
    sysd.lindblad = H.sparse_jump_ops(N, 8, seed=5)
    rng = np.random.default_rng(77)
    tr = Trajectories(np.array([0, 2]), np.array([2, 3]), _mtos(rng, N, 3))
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    pt = ptmod.random_pt(N, 4, 4, n_slices=4, seed=4, eps=0.1)
    ref = H.numpy_propagate(sysd, grid, rho0, ops, tr, pt=pt)
    _check(engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True), ref, "N=24, 8 jump operators")


def test_many_taylor_factors():
    """H0 x 20: s > 1 factors per sub-step"""
    sysd, grid, rho0, ops, tr, pt, ref = _case(8, 4, 4, 1, 20)
    _check(engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True), ref, "N=8 chi=4 H0 x 20")


def test_periodic_schedule():
    """n_init = 1 of 4 slices over 6 steps: slices 0, 1, 2, 3, 1, 2"""
    sysd, grid, rho0, ops, tr, pt, ref = _case(8, 16, 4, 1, 1, 1)
    assert list(pt.schedule(6)) == [0, 1, 2, 3, 1, 2]
    _check(engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True), ref, "N=8 chi=16 periodic")


# ------------------------------------------------------------------------------------------ 2. forced below dim 7
@pytest.mark.parametrize("N,chi", [(2, 7), (3, 16), (6, 64)])
def test_forced_path_matches_the_oracle_and_the_sweep(N, chi):
    from oracle import oracle
    sysd, grid = H.random_system(N, n_chan=2, n_lind=2, n_steps=6, dt=0.1, seed=40 + N)
    rng = np.random.default_rng(N)
    tr = Trajectories(np.array([0, 2]), np.array([5, 6]), _mtos(rng, N, 6))
    ops = [H.ketbra(N, 0, 0), H.ketbra(N, N - 1, 0), np.eye(N)]
    rho0 = H.random_rho(N)
    pt = ptmod.random_pt(N, chi, n_slices=4, seed=chi, eps=0.1)
    plan = engine.Plan(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    assert plan.describe()["path"] == str(_lib.PQD_PATH_HILBERT_PT)
    plan.execute()
    got = plan.download()
    _check(got, oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt), f"N={N} chi={chi} vs oracle")
    sweep = engine.Plan(sysd, grid, rho0, ops, tr, pt=pt)
    assert sweep.describe()["path"] != str(_lib.PQD_PATH_HILBERT_PT)
    sweep.execute()
    _check(got, sweep.download(), f"N={N} chi={chi} vs the existing sweep")


# ------------------------------------------------------------------------------------------ 3. invariants
def test_structured_pt_leaves_the_physics_unchanged():
    """synthetic_pt(structured=True): bond channel 0 is decoupled and closes the bond, so the outputs are those of the
    no-PT Hilbert run while the whole chi x chi arithmetic is performed"""
    N = 8
    sysd, grid = H.random_system(N, n_steps=6, dt=0.1, seed=81)
    rng = np.random.default_rng(81)
    tr = Trajectories(np.array([0, 2]), np.array([5, 6]), _mtos(rng, N, 6))
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    pt = ptmod.synthetic_pt(np.diag(np.arange(N) % 2).astype(float), 16, structured=True)
    got = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    _check(got, engine.propagate(sysd, grid, rho0, ops, tr), "structured PT vs no PT")


@pytest.mark.parametrize("N,n_sub", [(7, 1), (9, 2)])
def test_a_trivial_pt_gives_the_bits_of_the_run_without_a_pt(N, n_sub):
    """chi = 1, D = 1, every slice Q = [[1]], closures and bond0 = 1: what the PT kernel does beyond the shared step
    (lind_hilbert_step.h) is a multiplication by 1 or an addition of 0, and the output sums run in the same order
    whichever wave takes them, so the result is that of lind_hilbert_kernel bit for bit"""
    n_steps = 6
    sysd, grid = H.random_system(N, n_chan=2, n_lind=2, n_steps=n_steps, dt=0.1, n_sub=n_sub, seed=N)
    rng = np.random.default_rng(300 + N)
    tr = Trajectories(np.array([0, 2]), np.array([n_steps - 1, n_steps]), _mtos(rng, N, n_steps))
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    one = np.ones(1, dtype=np.complex128)
    pt = engine.ProcessTensor(Q=np.ones((1, 1, 1, 1), dtype=np.complex128), closure=one[None, :], closure0=one,
                              bond0=one, gmap=np.zeros(N * N, dtype=np.int32), n_init=0)
    got = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    want = engine.propagate(sysd, grid, rho0, ops, tr)
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert np.all(np.isfinite(b)) and np.max(np.abs(b)) > 0
        assert np.array_equal(a, b)


def test_alone_and_in_a_batch_of_70_are_byte_equal():
    N, chi, n_steps, n_traj = 7, 5, 5, 70
    systems = [H.random_system(N, n_steps=n_steps, seed=60 + k, n_lind=1 + k)[0] for k in range(3)]
    grid = Grid(0.0, 0.1, n_steps)
    rng = np.random.default_rng(8)
    ops = [_dense(rng, N) for _ in range(2)]
    rho0 = H.random_rho(N)
    pt = ptmod.random_pt(N, chi, 4, n_slices=4, seed=3, eps=0.1)
    tsys = np.arange(n_traj) % 3
    begins = np.arange(n_traj) % 4
    ends = n_steps - (np.arange(n_traj) % 2)
    mto_of = {t: MTO(t, int(1 + t % 4), bool(t % 2), t % 3, _dense(rng, N) / N) for t in range(n_traj)}
    tr = Trajectories(begins, ends, [mto_of[t] for t in range(n_traj)], system=tsys)
    batch = engine.propagate(systems, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    for t in (0, 1, 2, 35, 68, 69):
        m = mto_of[t]
        one = Trajectories(begins[t: t + 1], ends[t: t + 1], [MTO(0, m.step, m.before, m.kind, m.op)])
        single = engine.propagate(systems[tsys[t]], grid, rho0, ops, one, pt=pt, wide_pt=True)[0]
        assert single.tobytes() == batch[t].tobytes(), t


def test_slices_in_flight_do_not_change_a_bit(monkeypatch):
    """default G against PQD_HBPT_G=1 (and 2) at dim 7, chi 33"""
    sysd, grid, rho0, ops, tr, pt, ref = _case(7, 33, 4)
    monkeypatch.delenv("PQD_HBPT_G", raising=False)
    base = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    _check(base, ref, "N=7 chi=33 default G")
    for g in ("1", "2"):
        monkeypatch.setenv("PQD_HBPT_G", g)
        got = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
        for a, b in zip(got, base):
            assert a.tobytes() == b.tobytes(), g


def test_zero_steps_gives_the_initial_expectation_through_the_closure():
    N, chi = 8, 5
    sysd, _ = H.random_system(N, n_steps=1, seed=4)
    rng = np.random.default_rng(4)
    ops = [_dense(rng, N) for _ in range(2)]
    rho0 = H.random_rho(N)
    pt = ptmod.random_pt(N, chi, 4, n_slices=4, seed=9, eps=0.1)
    out = engine.propagate(sysd, Grid(0.0, 0.1, 0), rho0, ops, Trajectories(np.array([0]), np.array([0])), pt=pt,
                           wide_pt=True)
    want = np.array([[np.trace(O @ rho0) for O in ops]]) * (pt.closure0 @ pt.bond0)
    print(f"zero steps: rel err {rel(out[0], want):.3e}")
    assert out[0].shape == (1, 2) and rel(out[0], want) < 1e-12


# ------------------------------------------------------------------------------------------ 4. the other entry points
def test_table_and_trapz_on_this_path():
    N, n_steps = 8, 10
    sysd, grid = H.random_system(N, n_steps=n_steps, seed=80)
    rng = np.random.default_rng(10)
    ops = [_dense(rng, N) for _ in range(3)]
    rho0 = H.random_rho(N)
    pt = ptmod.random_pt(N, 6, 4, n_slices=4, seed=6, eps=0.1)
    tr = Trajectories(np.array([0, 4, 9]), np.array([10, 10, 10]), [MTO(1, 3, False, 1, _dense(rng, N) / N)])
    flat = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    tabs = engine.propagate_table(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    for a, b in zip(tabs, engine.tables_from_outputs(flat, tr, grid)):
        np.testing.assert_array_equal(a, b)
    kh, kt, dx = [0, 2, 1], [1, 2, 0], 0.1
    got = engine.propagate_trapz(sysd, grid, rho0, ops, tr, kh, kt, dx, pt=pt, wide_pt=True)
    assert got.shape == (3, 3)
    for t, y in enumerate(flat):
        for q in range(3):
            L = y.shape[0]
            want = 0.0 if L < 2 else dx * (0.5 * y[0, kh[q]] + y[1: L - 1, kt[q]].sum() + 0.5 * y[L - 1, kt[q]])
            assert abs(got[t, q] - want) <= 1e-13 * max(1.0, abs(want))


def test_plan_reports_the_path():
    sysd, grid, rho0, ops, tr, pt, ref = _case(8, 16, 4)
    plan = engine.Plan(sysd, grid, rho0, ops, tr, pt=pt, wide_pt=True)
    d = plan.describe()
    assert d["path"] == str(_lib.PQD_PATH_HILBERT_PT) == "6" and d["BT"] == "1" and d["win"] == "0" and d["lean"] == "0"
    assert plan.info()[1] == 1 and "wide PT" in plan.info()[0] and not plan.windows() and not plan.sweep_lean()
    keys = list(engine.Plan(*H.random_system(3, n_steps=4), H.random_rho(3), [np.eye(3)], H.simple_traj(4)).describe())
    assert list(d) == keys  # the same keys in the same order as an existing plan's line
    outs = []
    for rebuild in (True, False):  # rebuild_free is ignored: there are no free propagators
        plan.execute(rebuild_free=rebuild)
        outs.append(plan.download())
        _check(outs[-1], ref, f"plan, rebuild_free={rebuild}")
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    ms_free, ms_sweep, n = plan.timing()
    assert ms_free == 0.0 and ms_sweep > 0.0 and n == 2


# ------------------------------------------------------------------------------------------ 5. refusals
def _refused(fn, *a, **k):
    with pytest.raises((_lib.PQDError, ValueError)) as ei:
        fn(*a, **k)
    assert ei.value.code in (_lib.PQD_ERR_UNSUPPORTED, 1), ei.value
    return str(ei.value)


def test_refusals_with_a_wide_handle_name_the_value():
    rho = H.random_rho(8)
    pt = ptmod.random_pt(8, 4, 4, n_slices=3, seed=1, eps=0.1)
    s9, g9 = H.random_system(8, n_lind=9, n_steps=2, seed=1)
    assert "n_lind 9" in _refused(engine.propagate, s9, g9, rho, [np.eye(8)], H.simple_traj(2), pt=pt, wide_pt=True)
    s3, g3 = H.random_system(3, n_lind=9, n_steps=2, seed=1)  # the limit holds at every dim on this path
    pt3 = ptmod.random_pt(3, 4, 4, n_slices=3, seed=1, eps=0.1)
    assert "n_lind 9" in _refused(engine.propagate, s3, g3, H.random_rho(3), [np.eye(3)], H.simple_traj(2), pt=pt3,
                                  wide_pt=True)
    s8, g8 = H.random_system(8, n_steps=2, seed=2)
    s8.H0 = s8.H0 * 1e7
    msg = _refused(engine.propagate, s8, g8, rho, [np.eye(8)], H.simple_traj(2), pt=pt, wide_pt=True)
    assert "norm bound" in msg and "4096" in msg and "e+" in msg
    # a PT handle of dim 7 handed to a dim-8 plan (engine._prep checks the map's length first, so go below it)
    ctx = _lib.context()
    pt7 = ptmod.random_pt(7, 4, 4, n_slices=3, seed=1, eps=0.1)
    ok, g = H.random_system(8, n_steps=2, seed=2)
    with ctx.lock:
        keep, total = engine._prep(ok, g, rho, [np.eye(8)], H.simple_traj(2), None, ctx)
        k1, k2, r0, ops, sched, sc, gc, tc, tsys, n_sys = keep
        h = C.c_void_p()
        rc = _lib.lib().pqd_plan_create_multi(ctx.handle, n_sys, sc, _lib.iptr(tsys), C.byref(gc),
                                              pt7.handle(ctx, 7, wide=True), None, _lib.cptr(r0), 1, _lib.cptr(ops),
                                              C.byref(tc), max(1, total), C.byref(h))
        msg = _lib.lib().pqd_last_error().decode()
    assert rc == 1 and "PT dim 7 != system dim 8" in msg and not h.value
    # without the opt-in a PT at dim 8 is refused as before
    assert "dim 8" in _refused(engine.propagate, ok, g, rho, [np.eye(8)], H.simple_traj(2), pt=pt)


# ------------------------------------------------------------------------------------------ 6. through the drop-in
BATH = dict(t_mem=0.8, threshold=1e-6, max_bond=16, ae=3.0, temperature=1.0)
ID = " otimes Id_2 otimes Id_2"


@pytest.fixture(scope="module")
def pt_files(tmp_path_factory):
    """the PT of the coupling |1><1|_2 and of the same coupling with two identity factors, from identical small
    parameters (host generator), saved as pqd containers: (bare file, wide file)"""
    d = tmp_path_factory.mktemp("wide_pt")
    B = np.diag([0.0, 1.0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the bond cap decides cuts at these parameters (recorded in meta)
        bare = ptgen.qd_phonon_pt(B, 0.1, **BATH)
        wide = ptgen.qd_phonon_pt(np.kron(B, np.eye(4)), 0.1, **BATH)
    np.testing.assert_array_equal(bare.Q, wide.Q)
    ptmod.save_pt(str(d / "bare.npz"), bare, dim=2)
    ptmod.save_pt(str(d / "wide.npz"), wide, dim=8)
    return str(d / "bare.npz"), str(d / "wide.npz")


def _pulse():
    from pyaceqd_amd.pulses import ChirpedPulse
    return ChirpedPulse(tau_0=1.0, e_start=0.0, e0=3.0, t0=4.0)


def test_identity_factors_do_not_change_the_two_level_system(pt_files):
    """TLS (x) Id_2 (x) Id_2 at dim 8 on the new path against the TLS at dim 2 on the existing one: one driven pulse,
    200 steps at dt 0.1, the same PT slices. Occupation and coherence agree to 1e-10 (each path is pinned to 1e-11 by
    the exact-solution tests; two different exponentials)"""
    from pyaceqd_amd.general_system.general_system import system_ace_stream
    bare, wide = pt_files

    def run(sfx, pt_file, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the files' generation parameters are not the call's defaults
            return system_ace_stream(0, 20, _pulse(), dt=0.1, phonons=True, pt_file=pt_file,
                                     boson_op="|1><1|_2" + sfx, initial="|0><0|_2" + sfx.replace("Id_2", "|0><0|_2"),
                                     system_op=["0.3 * (|1><1|_2" + sfx + ")"],
                                     lindblad_ops=[["|0><1|_2" + sfx, 0.01]], interaction_ops=[["|1><0|_2" + sfx, "x"]],
                                     output_ops=["|1><1|_2" + sfx, "|0><1|_2" + sfx], **kw)
    got = run(ID, wide, wide_pt=True)
    ref = run("", bare)
    assert got.shape == ref.shape == (3, 201)
    err = float(np.max(np.abs(got[1:] - ref[1:])))
    print(f"TLS (x) Id (x) Id vs TLS: max abs difference {err:.3e}; max occupation {np.max(ref[1].real):.3f}")
    assert np.max(ref[1].real) > 0.1  # the pulse did drive the system
    assert err <= 1e-10


def test_tls_two_sensor_with_phonons_matches_the_numpy_reference(monkeypatch, tmp_path):
    """the wrapper with the PT of the device generator (the wrapper fixes ACE's threshold entry as the reference does,
    so the keyword passes through unused); what engine.propagate_table received is propagated again by numpy"""
    from pyaceqd_amd.general_system import general_system as gs
    from pyaceqd_amd.two_level_system.tls import tls_two_sensor
    seen = {}
    real = gs.propagate_table

    def spy(system, grid, rho0, out_ops, traj, pt=None, ctx=None, **kw):
        seen.update(system=system, grid=grid, rho0=rho0, out_ops=out_ops, traj=traj, pt=pt, kw=kw)
        return real(system, grid, rho0, out_ops, traj, pt=pt, ctx=ctx, **kw)
    monkeypatch.setattr(gs, "propagate_table", spy)
    monkeypatch.delenv("PQD_PTGEN", raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = tls_two_sensor(0, 2, _pulse(), dt=0.1, phonons=True, wide_pt=True, t_mem=2.0, threshold="6",
                             temp_dir=str(tmp_path) + "/")
    assert seen["system"].dim == 8 and seen["grid"].n_steps == 20 and seen["kw"] == {"wide_pt": True}
    pt = seen["pt"]
    assert pt is not None and pt.gmap.shape[0] == 64 and pt.D == 4
    ref = H.numpy_propagate(seen["system"], seen["grid"], seen["rho0"], seen["out_ops"], seen["traj"], pt=pt)[0]
    got = np.asarray(res[1:]).T
    print(f"tls_two_sensor with phonons: chi {pt.chi}, rel err {rel(got, ref):.3e}")
    assert got.shape == ref.shape and rel(got, ref) < 1e-12


def test_sensors_do_not_disturb_the_phonon_dressed_dot(pt_files):
    """the occupation of the dot read by two sensors (epsilon = 1e-4) against tls(phonons=True) with the same bath:
    within 10 x the same difference without phonons (existing paths) + 1e-10"""
    from pyaceqd_amd.two_level_system.tls import tls, tls_two_sensor
    bare, wide = pt_files
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a0 = tls(0, 10, _pulse(), dt=0.1, phonons=False)
        b0 = tls_two_sensor(0, 10, _pulse(), dt=0.1, phonons=False)
        a1 = tls(0, 10, _pulse(), dt=0.1, phonons=True, pt_file=bare)
        b1 = tls_two_sensor(0, 10, _pulse(), dt=0.1, phonons=True, wide_pt=True, pt_file=wide)
    d0 = float(np.max(np.abs(np.asarray(a0[2]) - np.asarray(b0[2]))))
    d1 = float(np.max(np.abs(np.asarray(a1[2]) - np.asarray(b1[2]))))
    print(f"sensor coupling: occupation difference without phonons {d0:.3e}, with phonons {d1:.3e}")
    assert np.max(np.abs(np.asarray(a1[2]) - np.asarray(a0[2]))) > 1e-4  # the bath does act
    assert d1 <= 10 * d0 + 1e-10
