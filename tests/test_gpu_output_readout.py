"""The output readout of every propagation path with dense operators and many outputs, vs the CPU oracle. GPU only.

Every path ends a step by closing the bond and contracting the reduced state with n_out output rows (ovec, or for fused
steps W(n) = ovec . M_b(n-1)); each kernel has its own readout code with its own thresholds in n_out (1..256 through the
C-ABI). The cases sit on both sides of each threshold, with full complex non-Hermitian operators (helpers.dense_ops), a
non-Hermitian initial matrix (helpers.dense_state) and helpers.readout_trajectories (ragged windows, a window opening
at step 2, MTOs of kinds 0, 1, 2 with both flags, MTOs at steps with outputs):

  no PT (sweep_nopt_kernel)        lane k owns outputs k, k + 64, ...                               64 | 65
  batched sweep, general instance  one lane per (trajectory, output, row) while BT n_out N2 <= NT at
                                   N2 = 4, 16, else the generic loop                                NT | NT + 1
  batched sweep, lean instance     at most 4 outputs, else the general instance                     4 | 5
  split groups                     RPP = 16 (N2 <= 16) or 64 outputs a pass; rows staged in LDS
                                   while n_out N2 <= 1024, else read from memory                    RPP | RPP + 1, 1024 | 1025
  quads                            four lanes per (trajectory, output k < 4), in passes             4 | 5, 8 | 9
  multi-trajectory split groups    outputs two at a time, at most 8                                 odd / even, 8 | 9
  Hilbert space, without / with PT wave v sums outputs v, v + n_waves, ...                          n_waves | n_waves + 1
  fuse kernels                     W(m), Widle: n_out N2 elements on 256 threads                    256 elements

Each case asserts the path the plan reports (Plan.describe()["path"], the workgroup shape, the lean flag where it
matters, and no fallback launch): a case that silently ran another kernel fails.

Comparison, per trajectory and output column k: max_n |got - ref| / max_n |ref[:, k]| (helpers.column_errors), so one
wrong column cannot hide under the largest entry of a 256-column table; the reference's smallest column maximum must
exceed 0.05 of its largest, so the normalisation cannot become empty. Tolerances are DESIGN.md section 5's: 1e-11 for PT
sweeps, 1e-12 without a PT, 1e-12 for the two Hilbert-space kernels (the bound of tests/test_gpu_hilbert.py and
tests/test_gpu_hilbert_pt.py). One oracle run per input set with 256 operators serves every n_out (dense_ops draws
operator by operator, so fewer outputs are the leading columns). Every worst column error is printed.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle
from pyaceqd_amd import _lib, engine
from tests import helpers as H

pytestmark = pytest.mark.gpu

NOPT, BATCHED, SPLIT, QUAD, MSPLIT, HILBERT, HILBERT_PT = range(7)  # the keys of engine.Plan.PATHS
TOL_PT, TOL_NOPT, TOL_HILBERT = 1e-11, 1e-12, 1e-12
N_STEPS, N_MAX, DT = 12, 256, 0.1
PULSE = (0.25, 0.6)  # windowed systems: the drive is exactly zero outside this fraction of the samples


@functools.lru_cache(maxsize=None)
def inputs(N, chi, n_traj=5, windowed=False, n_steps=N_STEPS):
    """(system, grid, rho0, 256 operators, trajectories, pt, oracle outputs) of one input set, built once and read-only
    afterwards"""
    sysd, grid = H.random_system(N, n_steps=n_steps, dt=DT, seed=500 + N)
    if windowed:
        chans = []
        for X, f in sysd.channels:
            f = np.array(f)
            keep = np.zeros(len(f), bool)
            keep[int(PULSE[0] * len(f)):int(PULSE[1] * len(f))] = True
            f[~keep] = 0.0
            chans.append((X, f))
        sysd.channels = chans
    tr = H.readout_trajectories(N, n_steps, n_traj, seed=N + n_traj)
    pt = None if chi is None else H.readout_pt(N, chi, seed=100 * chi + N)
    rho0 = H.dense_state(N, seed=N)
    ops = H.dense_ops(N, N_MAX, seed=20 + N)
    ref = oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt, nthreads=4)
    for r in ref:
        r.setflags(write=False)
    return sysd, grid, rho0, ops, tr, pt, ref


def check(case, n_out, tol, what, path, expect=None, wide=False):
    """run the plan of `case` with its first n_out operators; the plan must report `path` (an int, or a predicate) and
    the describe() entries of `expect` before and after the run, without a fallback launch; every column within tol"""
    sysd, grid, rho0, ops, tr, pt, ref = case
    plan = engine.Plan(sysd, grid, rho0, ops[:n_out], tr, pt=pt, wide_pt=wide)
    for when in ("created", "executed"):
        d = plan.describe()
        p = int(d["path"])
        assert path(p) if callable(path) else p == path, f"{what}: path {p} ({engine.Plan.PATHS[p]}) when {when}"
        for k, v in (expect or {}).items():
            assert d[k] == str(v), f"{what}: {k}={d[k]}, expected {v} when {when}"
        if when == "created":
            plan.execute()
            got = plan.download()
    assert plan.info()[2] == 0, f"{what}: {plan.info()[2]} launches fell back to another kernel"
    err, ratio = H.column_errors(got, [r[:, :n_out] for r in ref])
    print(f"{what} n_out={n_out} [{engine.Plan.PATHS[p]}]: worst column {float(err.max()):.3e}, "
          f"smallest column ratio {ratio:.3f}")
    assert err.shape == (tr.n_traj, n_out)
    assert ratio > 0.05
    assert np.all(np.isfinite(err)) and float(err.max()) < tol, (float(err.max()), np.argwhere(~(err < tol))[:8].tolist())
    return plan, got


# ---------------------------------------------------------------------------------------------- no PT
@pytest.mark.parametrize("n_out", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("N", [3, 6])
def test_no_pt(N, n_out):
    """lane k of the trajectory's wave owns outputs k, k + 64, ...: a wave short of full, full, one past, four rounds"""
    check(inputs(N, None, 3), n_out, TOL_NOPT, f"no PT N={N}", NOPT)


# ---------------------------------------------------------------------------------------------- batched sweep
def batched_env(monkeypatch, bt):
    monkeypatch.setenv("PQD_SPLIT", "0")  # neither kind of split groups
    monkeypatch.setenv("PQD_QUAD", "0")
    monkeypatch.setenv("PQD_BT", bt)


@pytest.mark.parametrize("bt", ["4", "8"])
@pytest.mark.parametrize("N,n_out", [(N, k) for N in (3, 5, 6) for k in (1, N * N, 37, 256)])
def test_batched_generic_loop(monkeypatch, N, n_out, bt):
    """N2 = 9, 25, 36 never take one lane per row: the loop over (trajectory, output) pairs of the general instance,
    with fewer pairs than threads and many more; five trajectories are two workgroups of four (the second with one
    trajectory) or one of eight with three empty slots. N2 > 16 holds four trajectories per workgroup at most"""
    batched_env(monkeypatch, bt)
    BT = min(int(bt), 8 if N * N <= 16 else 4)
    check(inputs(N, 16), n_out, TOL_PT, f"batched N={N} BT={BT}", BATCHED, {"BT": BT, "lean": 0})


def lane_limit(N2, BT, CHI):
    """the largest n_out the general instance reads with one lane per (trajectory, output, row): pt_sweep.hip takes that
    readout when N2 is 4 or 16, the trace rows are prefetched (trpre) and ntr = BT n_out N2 <= NT, the workgroup's
    threads. NT = 64 BT WPT with WPT = sweep_wpt(N2, BT, CHI) waves per trajectory (pqd_common.h): 2 at BT = 4 and
    chi >= 32, else 1. So ntr <= NT is n_out N2 <= 64 WPT, and since N2 divides 64 the largest such n_out has
    ntr == NT exactly: 16 (N2 = 4) and 4 (N2 = 16) with one wave per trajectory, 32 and 8 with two"""
    wpt = 2 if BT == 4 and CHI >= 32 else 1
    NT = 64 * BT * wpt
    assert NT % (BT * N2) == 0
    return NT // (BT * N2), NT


@pytest.mark.parametrize("side", ["at", "past"])
@pytest.mark.parametrize("bt", ["4", "8"])
@pytest.mark.parametrize("N,chi", [(4, 16), (4, 32), (2, 16), (2, 32)])
def test_batched_lane_per_row_threshold(monkeypatch, N, chi, bt, side):
    """N2 = 16 and N2 = 4 (the two-level system with the quads switched off) on the general instance: ntr == NT, the
    last count read with one lane per row, and the first count past it, on the generic loop; NT from the BT the plan
    reports"""
    batched_env(monkeypatch, bt)
    lim, _ = lane_limit(N * N, int(bt), chi)
    n_out = lim if side == "at" else lim + 1
    plan, _ = check(inputs(N, chi), n_out, TOL_PT, f"batched N={N} chi={chi} BT={bt} {side} NT", BATCHED,
                    {"BT": bt, "lean": 0, "trpre": 1, "fuse": 1})
    BT = int(plan.describe()["BT"])
    lim, NT = lane_limit(N * N, BT, chi)
    ntr = BT * n_out * N * N
    assert ntr == NT if side == "at" else (ntr > NT and ntr - BT * N * N == NT)


@pytest.mark.parametrize("N,n_out", [(4, 4), (2, 16)])
def test_batched_without_prefetched_trace_rows(monkeypatch, N, n_out):
    """PQD_TRPRE=0: the counts the lane-per-row readout would take go through the generic loop"""
    batched_env(monkeypatch, "8")
    monkeypatch.setenv("PQD_TRPRE", "0")
    check(inputs(N, 16), n_out, TOL_PT, f"batched N={N} trpre=0", BATCHED, {"BT": 8, "lean": 0, "trpre": 0})


@pytest.mark.parametrize("lean_ro", ["default", "0"])
@pytest.mark.parametrize("n_out", [1, 4, 5])
def test_lean_instance_takes_four_outputs(monkeypatch, n_out, lean_ro):
    """N = 4, chi = 64, BT = 8: up to four outputs run the lean instance (BT n_out N2 <= 512), read in its fused column
    phase after the last MTO (default) or in the closure pass everywhere (PQD_LEAN_RO=0); five must run the general
    instance (its generic loop: ntr = 640 > NT = 512)"""
    batched_env(monkeypatch, "8")
    if lean_ro == "0":
        monkeypatch.setenv("PQD_LEAN_RO", "0")
    lean = n_out <= 4
    plan, _ = check(inputs(4, 64), n_out, TOL_PT, f"lean N=4 chi=64 LEAN_RO={lean_ro}", BATCHED,
                    {"BT": 8, "lean": int(lean)})
    assert plan.sweep_lean() == lean
    assert plan.sweep_readout() == (lean and lean_ro == "default")


def test_general_instance_at_the_lean_shape(monkeypatch):
    """PQD_SWEEP_LEAN=0 at four outputs: the general instance with ntr == NT = 512, one lane per row"""
    batched_env(monkeypatch, "8")
    monkeypatch.setenv("PQD_SWEEP_LEAN", "0")
    plan, _ = check(inputs(4, 64), 4, TOL_PT, "general N=4 chi=64 BT=8", BATCHED, {"BT": 8, "lean": 0, "trpre": 1})
    assert not plan.sweep_lean() and lane_limit(16, 8, 64) == (4, 512)


# ---------------------------------------------------------------------------------------------- split groups
SPLIT_COUNTS = {4: (16, 17, 64, 65, 256),   # RPP = 16; 64 N2 = 1024 staged, 65 read from memory
                3: (16, 17, 113, 114),      # RPP = 16; 113 x 9 = 1017 staged, 114 x 9 = 1026 from memory
                5: (40, 41, 64, 65),        # 40 x 25 = 1000 staged, 41 x 25 = 1025 from memory; RPP = 64
                6: (28, 29, 64, 65, 256)}   # 28 x 36 = 1008 staged, 29 x 36 = 1044 from memory; RPP = 64


@pytest.mark.parametrize("ow", ["1", "0"])
@pytest.mark.parametrize("N,n_out", [(N, k) for N, ks in SPLIT_COUNTS.items() for k in ks])
def test_split_single_trajectory(monkeypatch, N, n_out, ow):
    """one trajectory over N2 workgroups, the outputs written by the output workgroup or (PQD_SPLIT_OW=0) by workgroup
    0: one pass and one more, rows staged in LDS and rows read from memory, up to sixteen passes"""
    monkeypatch.setenv("PQD_SPLIT", "2")
    monkeypatch.setenv("PQD_SPLIT_OW", ow)
    check(inputs(N, 16, 1), n_out, TOL_PT, f"split N={N} OW={ow}", SPLIT, {"split_ow": ow, "split_chunk": 0})


def test_split_over_consecutive_launches():
    """the plan tests/golden/plan_choice.json records as split-N4-chi64-20-nout9, run: nine outputs keep 20 biexciton
    trajectories off the multi-trajectory groups, so they run as split groups in two launches (default switches)"""
    plan, _ = check(inputs(4, 64, 20), 9, TOL_PT, "split N=4 chi=64, 20 trajectories", SPLIT)
    d = plan.describe()
    assert 0 < int(d["split_chunk"]) < 20 and d["split_ow"] == "1"


# ---------------------------------------------------------------------------------------------- quads
@pytest.mark.parametrize("n_out", [1, 3, 4, 5, 8, 9, 256])
def test_quad(n_out):
    """four lanes per (trajectory, output k < 4): a partial pass, one, one and a bit, two, two and a bit, 64; five
    trajectories are one full quad and one with a single trajectory"""
    check(inputs(2, 16), n_out, TOL_PT, "quad N=2", QUAD, {"quad": 1})


# ---------------------------------------------------------------------------------------------- msplit
@pytest.mark.parametrize("tb", ["auto", "3"])
@pytest.mark.parametrize("n_out", list(range(1, 9)))
@pytest.mark.parametrize("N,chi", [(4, 64), (3, 32)])
def test_msplit_every_output_count(monkeypatch, N, chi, n_out, tb):
    """outputs two at a time, odd and even counts up to the path's eight; one trajectory per group, and (PQD_MS_TB=3)
    groups of three and two. Every trajectory has an MTO inside its window, so the rows of those steps are the
    composite events' (Wev) and the others ovec's or W(n)'s"""
    monkeypatch.setenv("PQD_MSPLIT", "2")
    if tb != "auto":
        monkeypatch.setenv("PQD_MS_TB", tb)
    plan, _ = check(inputs(N, chi), n_out, TOL_PT, f"msplit N={N} chi={chi} TB={tb}", MSPLIT,
                    {"ms_TB": 1 if tb == "auto" else tb})
    assert int(plan.describe()["n_cev"]) >= 5  # composite MTO steps were built


@pytest.mark.parametrize("N,chi", [(4, 64), (3, 32)])
def test_msplit_leaves_the_path_at_nine_outputs(monkeypatch, N, chi):
    monkeypatch.setenv("PQD_MSPLIT", "2")
    check(inputs(N, chi), 9, TOL_PT, f"msplit refused N={N} chi={chi}", lambda p: p != MSPLIT, {"ms_TB": 0})


# ---------------------------------------------------------------------------------------------- Hilbert space
@pytest.mark.parametrize("chi", [None, 5])
@pytest.mark.parametrize("N,n_out", [(7, 1), (7, 2), (7, 256), (9, 2), (9, 3), (9, 256)])
def test_hilbert(N, n_out, chi):
    """one thread per element in whole waves: dim 7 (49 elements) runs one wave, dim 9 (81) two; wave v sums outputs
    v, v + n_waves, ...: n_waves outputs, one more, 256. Without a PT, and with a wide PT of bond 5"""
    n_waves = (N * N + 63) // 64
    assert n_out in (n_waves, n_waves + 1, 256)
    check(inputs(N, chi, 3, n_steps=8), n_out, TOL_HILBERT, f"Hilbert N={N} chi={chi}", HILBERT_PT if chi else HILBERT,
          wide=chi is not None)


def test_hilbert_forced_at_dim_3(monkeypatch):
    """PQD_HILBERT=1: a plan without PT of dim <= 6 on the Hilbert-space kernel, 65 outputs on its single wave"""
    monkeypatch.setenv("PQD_HILBERT", "1")
    check(inputs(3, None, 3), 65, TOL_HILBERT, "Hilbert forced N=3", HILBERT)


# ---------------------------------------------------------------------------------------------- fused rows, pulse windows
@pytest.mark.parametrize("win", ["default", "0"])
@pytest.mark.parametrize("N,n_out,path", [(4, 37, BATCHED), (6, 37, BATCHED), (2, 65, QUAD)])
def test_fused_rows_and_pulse_windows(monkeypatch, N, n_out, path, win):
    """a drive that is exactly zero outside 35% of the run: the fuse kernels build W(m) = ovec . M_b(m-1) for n_out N2 =
    592, 1,332 and 260 elements on 256 threads (the general, the matrix-core and the flat kernel), and PQD_FUSE=0 reads
    ovec on the stepped state instead; both against the oracle and against each other. Pulse windows exist where
    every kernel of the plan reads through them, which is the quads (N = 2: W(m) inside the window, Widle outside it);
    the batched sweep at N = 4 and 6 stores every half step, with or without PQD_WIN"""
    monkeypatch.setenv("PQD_SPLIT", "0")
    monkeypatch.setenv("PQD_TRUNK", "0")  # (a trunk pre-pass would read every half step as stored: no windows)
    if win == "0":
        monkeypatch.setenv("PQD_WIN", "0")
    windows =path == QUAD and win == "default"
    res = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("PQD_FUSE", fuse)
        plan, res[fuse] = check(inputs(N, 16, 5, True), n_out, TOL_PT, f"windows N={N} FUSE={fuse} WIN={win}", path,
                                {"fuse": fuse, "win": int(windows)})
        assert plan.windows() == windows
    err, _ = H.column_errors(res["1"], res["0"])
    print(f"windows N={N} WIN={win}: fused vs unfused worst column {float(err.max()):.3e}")
    assert float(err.max()) < TOL_PT


# ---------------------------------------------------------------------------------------------- tables and integrals
def test_table_of_256_outputs_is_bit_equal_to_the_flat_outputs(monkeypatch):
    monkeypatch.setenv("PQD_SPLIT", "0")
    sysd, grid, rho0, ops, tr, pt, ref = inputs(4, 16)
    flat = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt)
    err, _ = H.column_errors(flat, ref)
    assert float(err.max()) < TOL_PT
    want = engine.tables_from_outputs(flat, tr, grid)
    got = engine.propagate_table(sysd, grid, rho0, ops, tr, pt=pt)
    assert len(got) == len(want) == tr.n_traj
    for g, w in zip(got, want):
        assert g.shape == w.shape == (1 + N_MAX, w.shape[1]) and np.array_equal(g, w)


def test_trapz_over_the_first_and_last_of_256_outputs(monkeypatch):
    """pairs (head 255, tail 0) and (head 0, tail 255) against the same sums over the flat outputs on the host, to the
    bound of test_gpu_parity.test_output_trapz_matches_host_integrals"""
    monkeypatch.setenv("PQD_SPLIT", "0")
    sysd, grid, rho0, ops, tr, pt, ref = inputs(4, 16)
    kh, kt, dx = [255, 0], [0, 255], 0.25
    got = engine.propagate_trapz(sysd, grid, rho0, ops, tr, kh, kt, dx, pt=pt)
    flat = engine.propagate(sysd, grid, rho0, ops, tr, pt=pt)
    assert got.shape == (tr.n_traj, 2)
    for t, y in enumerate(flat):
        L = y.shape[0]
        assert L >= 2
        for q in range(2):
            want = dx * (0.5 * y[0, kh[q]] + y[1: L - 1, kt[q]].sum() + 0.5 * y[L - 1, kt[q]])
            print(f"trapz trajectory {t} pair {q}: |got - want| = {abs(got[t, q] - want):.3e}, |want| = {abs(want):.3e}")
            assert abs(got[t, q] - want) <= 1e-13 * max(1.0, abs(want))


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("n_out", [0, 257])
def test_output_counts_outside_1_to_256_are_refused(n_out):
    """pqd_plan_create_multi with n_out = 0 and 257 (the operator buffer holds 257): PQD_ERR_ARG, the value named"""
    N = 3
    sysd, grid = H.random_system(N, n_steps=4, seed=1)
    tr = H.simple_traj(4)
    ctx = _lib.context()
    with ctx.lock:
        keep, total = engine._prep(sysd, grid, H.dense_state(N, 1), H.dense_ops(N, 257, 2), tr, None, ctx)
        k1, k2, r0, ops, sched, sc, gc, tc, tsys, n_sys = keep
        h = C.c_void_p()
        rc = _lib.lib().pqd_plan_create_multi(ctx.handle, n_sys, sc, _lib.iptr(tsys), C.byref(gc), None,
                                              _lib.iptr(sched), _lib.cptr(r0), n_out, _lib.cptr(ops), C.byref(tc),
                                              max(1, total), C.byref(h))
        msg = _lib.lib().pqd_last_error().decode(errors="replace")
    assert rc == 1 and not h.value  # PQD_ERR_ARG (include/pqd.h), no plan
    assert f"n_out {n_out} not in [1, 256]" in msg
    if n_out == 257:
        with pytest.raises(ValueError, match="n_out 257"):
            engine.Plan(sysd, grid, H.dense_state(N, 1), H.dense_ops(N, 257, 2), tr)
