"""Bit-for-bit comparison of the PT propagation paths and of the map-chain family between two libpqd builds.

usage: python scripts/compare_split_builds.py LIB_A LIB_B [--only SUBSTRING[,SUBSTRING...]] [--log FILE]
                                              [--names NAME_A,NAME_B  (what the log calls the two; default: the paths)]

For every case one child process per library (one after the other, each under its own time limit, the library chosen
through PQD_LIB, the case's switches in its environment) runs a plan on seeded inputs and saves every trajectory's
outputs, the plan's path, its fallback count and pqd_plan_describe's text; the parent compares every array with
np.array_equal and the texts as strings. Inputs are built like tests/test_gpu_parity.py::test_sweep_pt_split_groups and
tests/test_gpu_msplit.py: three systems, ragged windows, MTOs before and after an output (at step 0 and at a window's
last step among them), 150 steps, and a schedule that changes the slice at most steps and repeats it at some, so the
split kernels' schedule reader crosses its 64-entry chunk boundary twice. The cases together run every instance of
pt_split_kernel and pt_msplit_kernel (named in the case id), their switches, and one case per N2 of the batched sweep,
the quad kernel and the free propagators (the launch layer's dispatch).

The batched sweep itself (pt_sweep.hip; case ids sweep_*, PQD_SPLIT=0 PQD_MSPLIT=0 PQD_QUAD=0): the lean instance with one
system, two systems in a workgroup, PQD_LEAN_STAGE=0 and PQD_LEAN_RO=0 (19 trajectories, 60 steps, every MTO in the first
14), with partial units and PQD_LIVE_PART=0, the general instance at that shape, PQD_PT_MODE 0-5 at BT 4 and 8 and the
VALU rows at chi 16, 32 and 64, PQD_FUSE=0, PQD_TRPRE=0, PQD_CMUL3=0, PQD_COLBIG at N2 = 25 and 36, chi = 128, shared
trunks from the pre-pass (PQD_TRUNK=1) and from a slot of the workgroup, and chi = 1 at every N2 (sweep_nopt_kernel).
For these the saved text also holds sweep_lean(), sweep_readout() and sweep_stage().

The map-chain family (mapchain.hip; case ids mc_* and ft_*, e.g. --only mc_,ft_): the three sweep modes at dims 2-6 on
the default path, with PQD_MC_BLOCKED=0, with PQD_MC_BLOCKED=0 PQD_MC_PIPE=0 and (modes 0, 1) with PQD_MC_L=8;
propagate_tau and map_tail at dims 2-6; four_time_8op with its three flag settings, four_time and dynamics_t1 at dims
2, 3, 5. Inputs are seeded and built like those of tests/test_gpu_mapchain_paths.py and helpers.timebin_inputs: the
last wave of every sweep is part-filled, trunk ends lie on both sides of n_tb, and t1 segments reach the precalc maps.

Exit status 0: all equal; 1: a difference; 2: a child failed (the run stops there: nothing more is started on the
device)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

N_STEPS = 150
SWITCHES = ("PQD_SPLIT", "PQD_SPLIT_GRAN", "PQD_SPLIT_OW", "PQD_SPLIT_XCD", "PQD_SPLIT_L2", "PQD_SPLIT_SPIN",
            "PQD_MSPLIT", "PQD_MS_L2", "PQD_MS_PTM", "PQD_MS_TB", "PQD_ABLATE", "PQD_FPM", "PQD_QUAD",
            "PQD_MC_BLOCKED", "PQD_MC_PIPE", "PQD_MC_L", "PQD_MC_TIMING",
            "PQD_BT", "PQD_PT_MODE", "PQD_CMUL3", "PQD_COLBIG", "PQD_TRPRE", "PQD_FUSE", "PQD_SWEEP_LEAN", "PQD_LEAN_RO",
            "PQD_LEAN_STAGE", "PQD_LIVE_PART", "PQD_LIVE_COL", "PQD_LIVE_ROWS", "PQD_TRUNK", "PQD_BRANCH")
SPLIT, MSPLIT = "split groups", "split groups, several trajectories per group"
BATCHED, QUAD = "batched lock-step sweep", "register-resident TLS quads"
NOPT = "no PT (one wave per trajectory)"


def _sweep_cases(c):
    """the batched sweep (pt_sweep.hip): every instance kind and switch of pt_sweep_kernel, and sweep_nopt_kernel.
    `want`: what the child asserts of the plan besides its path (lean instance, readout in the column phase, staging
    workgroups, partial units), so that a case that left the path it is here for fails"""
    sw = dict(PQD_SPLIT=0, PQD_MSPLIT=0, PQD_QUAD=0)
    lean = dict(N=4, chi=64, n_traj=19, late=60)
    on = dict(lean=True, readout=True)
    c["sweep_lean_one_system"] = ("pt", dict(lean, want=dict(on, stage=True)), dict(sw, PQD_BT=8), BATCHED)
    # trajectories are packed by system (10 and 9): the second of the three workgroups mixes the two and does not stage
    c["sweep_lean_two_systems"] = ("pt", dict(lean, n_sys=2, want=dict(on, stage=True, staging=2)), dict(sw, PQD_BT=8),
                                   BATCHED)
    c["sweep_lean_stage=0"] = ("pt", dict(lean, want=dict(on, stage=False)), dict(sw, PQD_BT=8, PQD_LEAN_STAGE=0), BATCHED)
    c["sweep_lean_ro=0"] = ("pt", dict(lean, want=dict(lean=True, readout=False)), dict(sw, PQD_BT=8, PQD_LEAN_RO=0),
                            BATCHED)
    c["sweep_lean=0"] = ("pt", dict(lean, want=dict(lean=False)), dict(sw, PQD_BT=8, PQD_SWEEP_LEAN=0), BATCHED)
    live = dict(N=4, chi=64, live="x_only")
    c["sweep_lean_parts"] = ("pt", dict(live, want=dict(lean=True, parts="1")), dict(sw, PQD_BT=8), BATCHED)
    c["sweep_lean_parts_live_part=0"] = ("pt", dict(live, want=dict(lean=True, parts="0")),
                                         dict(sw, PQD_BT=8, PQD_LIVE_PART=0), BATCHED)
    # the general instances' PT rows: modes 0-5 (PQD_SWEEP_LEAN=0: mode 4 is the default and would run the lean instance);
    # mode 0 at BT = 4 runs the VALU rows with 4, 1 and 2 columns per lane (chi = 64, 16, 32)
    g = dict(N=4, chi=64, n_traj=9, want=dict(lean=False))
    for bt in (4, 8):
        for m in range(6):
            c[f"sweep_N2=16_chi=64_bt={bt}_ptmode={m}"] = ("pt", g, dict(sw, PQD_BT=bt, PQD_PT_MODE=m, PQD_SWEEP_LEAN=0),
                                                          BATCHED)
    c["sweep_N2=4_chi=16_bt=4_ptmode=0"] = ("pt", dict(N=2, chi=16, n_traj=9), dict(sw, PQD_BT=4, PQD_PT_MODE=0), BATCHED)
    c["sweep_N2=9_chi=32_bt=4_ptmode=0"] = ("pt", dict(N=3, chi=32, n_traj=9), dict(sw, PQD_BT=4, PQD_PT_MODE=0), BATCHED)
    for s in ("PQD_FUSE", "PQD_TRPRE", "PQD_CMUL3"):
        c[f"sweep_N2=16_chi=64_bt=8_{s[4:].lower()}=0"] = ("pt", g, dict(sw, PQD_BT=8, **{s: 0}), BATCHED)
    for N in (5, 6):
        c[f"sweep_N2={N * N}_chi=32_colbig=0"] = ("pt", dict(N=N, chi=32, n_traj=9), dict(sw, PQD_COLBIG=0), BATCHED)
        c[f"sweep_N2={N * N}_chi=32_colbig=default"] = ("pt", dict(N=N, chi=32, n_traj=9), sw, BATCHED)
    c["sweep_N2=16_chi=128_bt=4"] = ("pt", dict(N=4, chi=128, n_traj=9), dict(sw, PQD_BT=4), BATCHED)
    # shared trunks: the pre-pass instance and activations from its checkpoints, activations from a slot of the workgroup
    for N, chi, bt in ((4, 64, 8), (3, 16, 4)):
        # trunks: the plan has trunk pre-pass launches; shared: it propagates fewer trajectory-steps than full runs would
        br = dict(N=N, chi=chi, branch=29)
        c[f"sweep_N2={N * N}_chi={chi}_bt={bt}_trunk=1"] = ("pt", dict(br, want=dict(trunks=True)),
                                                           dict(sw, PQD_BT=bt, PQD_TRUNK=1), BATCHED)
        c[f"sweep_N2={N * N}_chi={chi}_bt={bt}_trunk=0_branch=1"] = (
            "pt", dict(br, want=dict(trunks=False, branch="1", shared=True)),
            dict(sw, PQD_BT=bt, PQD_TRUNK=0, PQD_BRANCH=1), BATCHED)
    for N in (2, 3, 4, 5, 6):   # no PT: MTOs before and after an output at one step (_trajectories, k = 2)
        c[f"sweep_nopt_N2={N * N}"] = ("pt", dict(N=N, chi=1, n_traj=9), sw, NOPT)


def _cases():
    """id -> (kind, parameters, switches, expected path or None)"""
    c = {}
    modes = {"granule": {"PQD_SPLIT_GRAN": 1}, "counter_ow": {"PQD_SPLIT_OW": 1}, "counter_noow": {"PQD_SPLIT_OW": 0}}
    for N in (2, 3, 4, 5, 6):
        for chi in (16, 32, 64):
            for tag, env in modes.items():
                c[f"split_N2={N * N}_chi={chi}_{tag}"] = ("pt", dict(N=N, chi=chi), dict(PQD_SPLIT=2, **env), SPLIT)
    for chi, Ns in ((32, (3, 4, 5, 6)), (64, (3, 4, 6)), (128, (3, 4)), (256, (2, 3, 4))):
        for N in Ns:
            c[f"msplit_N2={N * N}_chi={chi}"] = ("pt", dict(N=N, chi=chi, n_traj=7), dict(PQD_MSPLIT=2), MSPLIT)
    sp = dict(N=4, chi=64)
    ms = dict(N=4, chi=64, n_traj=19)
    c["split_N2=16_chi=64_noxcd"] = ("pt", sp, dict(PQD_SPLIT=2, PQD_SPLIT_XCD=0), SPLIT)
    c["msplit_N2=16_chi=64_noxcd"] = ("pt", ms, dict(PQD_MSPLIT=2, PQD_SPLIT_XCD=0), MSPLIT)
    c["split_N2=16_chi=64_l2=0"] = ("pt", sp, dict(PQD_SPLIT=2, PQD_SPLIT_L2=0), SPLIT)
    c["msplit_N2=16_chi=64_l2=0"] = ("pt", ms, dict(PQD_MSPLIT=2, PQD_MS_L2=0), MSPLIT)
    # a placement miss: the split plan falls back to the batched kernel, the msplit plan re-runs with sc1 stores
    c["split_N2=16_chi=64_ablate=512"] = ("pt", sp, dict(PQD_SPLIT=2, PQD_ABLATE=512), BATCHED)
    c["msplit_N2=16_chi=64_ablate=512"] = ("pt", ms, dict(PQD_MSPLIT=2, PQD_ABLATE=512), MSPLIT)
    # every wait times out: both fall back to the batched kernel
    c["split_N2=16_chi=64_spin=0"] = ("pt", sp, dict(PQD_SPLIT=2, PQD_SPLIT_SPIN=0), BATCHED)
    c["msplit_N2=16_chi=64_spin=0"] = ("pt", ms, dict(PQD_MSPLIT=2, PQD_SPLIT_SPIN=0), BATCHED)
    for ptm in (0, 1):
        c[f"msplit_N2=16_chi=64_ptm={ptm}"] = ("pt", ms, dict(PQD_MSPLIT=2, PQD_MS_PTM=ptm), MSPLIT)
    for tb in (1, 3, 5):
        c[f"msplit_N2=16_chi=64_tb={tb}"] = ("pt", ms, dict(PQD_MSPLIT=2, PQD_MS_TB=tb), MSPLIT)
    # G = 37 > 32: the single-counter branch (also split_N2=36_* above)
    c["split_N2=36_chi=32_single_counter"] = ("pt", dict(N=6, chi=32, n_traj=3), dict(PQD_SPLIT=2), SPLIT)
    # a batch above the co-resident capacity: split_chunk consecutive launches (auto mode)
    c["split_N2=9_chi=16_consecutive_launches"] = ("pt", dict(N=3, chi=16, n_traj=256 // 9 + 2), {}, SPLIT)
    for N in (2, 3, 4, 5, 6):
        # (PQD_QUAD=0: the two-level system on the batched kernel too)
        c[f"sweep_N2={N * N}_chi=32"] = ("pt", dict(N=N, chi=32, n_traj=9), dict(PQD_SPLIT=0, PQD_QUAD=0), BATCHED)
        c[f"free_N2={N * N}"] = ("free", dict(N=N), {}, None)
        c[f"free_N2={N * N}_fpm=0"] = ("free", dict(N=N), dict(PQD_FPM=0), None)
    for chi in (16, 32, 64):
        c[f"quad_N2=4_chi={chi}"] = ("pt", dict(N=2, chi=chi, n_traj=9), dict(PQD_SPLIT=0, PQD_QUAD=2), QUAD)
    _sweep_cases(c)
    # the map-chain family
    mc_env = {"default": {}, "noblocked": dict(PQD_MC_BLOCKED=0), "noblocked_nopipe": dict(PQD_MC_BLOCKED=0, PQD_MC_PIPE=0),
              "L=8": dict(PQD_MC_L=8)}
    for N in (2, 3, 4, 5, 6):
        for mode in (0, 1, 2):
            for tag, env in mc_env.items():
                if not (mode == 2 and tag == "L=8"):
                    c[f"mc_mode{mode}_dim={N}_{tag}"] = ("sweep", dict(N=N, mode=mode), env, None)
        c[f"mc_propagate_tau_dim={N}"] = ("propagate_tau", dict(N=N), {}, None)
        c[f"mc_map_tail_dim={N}"] = ("map_tail", dict(N=N), {}, None)
    for N in (2, 3, 5):
        for tag, flags in (("plain", (False, False)), ("early", (True, False)), ("late_t1", (False, True))):
            c[f"ft_8op_{tag}_dim={N}"] = ("ft8", dict(N=N, flags=flags), {}, None)
        c[f"ft_4op_dim={N}"] = ("ft4", dict(N=N), {}, None)
        c[f"ft_dynamics_t1_dim={N}"] = ("dyn", dict(N=N), {}, None)
    return c


def _trajectories(N, n_traj, seed):
    """ragged windows and ends; MTOs of kinds 0/1/2 at step 0, mid-run and at the window's last step, before and after
    at one step, two in one slot, and trajectories without any (tests/test_gpu_msplit.py mixed_trajectories)"""
    from pyaceqd_amd.engine import MTO, Trajectories
    rng = np.random.default_rng(seed)
    beg, end, mt = [], [], []
    for t in range(n_traj):
        e = int(rng.integers(N_STEPS // 2, N_STEPS + 1))
        if t == 0:
            e = N_STEPS  # one trajectory reads the whole schedule
        b = int(rng.integers(0, e))
        beg.append(b)
        end.append(e)
        A = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
        B = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
        A, B = A / np.linalg.norm(A), B / np.linalg.norm(B)
        s = int(rng.integers(0, e + 1))
        k = t % 6
        if k == 0:
            mt += [MTO(t, s, False, 2, A), MTO(t, s, False, 1, B)]
        elif k == 1:
            mt += [MTO(t, 0, True, 0, A)]
        elif k == 2:
            mt += [MTO(t, s, True, 1, A), MTO(t, s, False, 2, B)]
        elif k == 3:
            mt += [MTO(t, e, False, 0, A), MTO(t, max(0, e - 3), True, 2, B)]
        elif k == 4:
            mt += [MTO(t, s, False, 0, A), MTO(t, min(e, s + 1), False, 1, np.eye(N) * 0.5 + B)]
    return Trajectories(np.array(beg), np.array(end), mt)


def _late_trajectories(N, n_traj, n_sys, n_steps):
    """every MTO in the first 14 steps, ragged windows to the end, one window that opens after its MTO
    (tests/test_gpu_sweep_readout.py trajectories): the lean instance's fast region runs for most of the steps"""
    from pyaceqd_amd.engine import MTO, Trajectories
    rng = np.random.default_rng(100 + n_traj)
    A = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    B = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    A, B = A / np.linalg.norm(A), B / np.linalg.norm(B)
    t1 = [1 + (5 * i) % 14 for i in range(n_traj)]
    mt = [m for i in range(n_traj) for m in (MTO(i, t1[i], False, 2, A), MTO(i, t1[i], False, 1, B))]
    beg = [t1[i] + 6 if i == 2 else t1[i] for i in range(n_traj)]
    end = [n_steps - (3 * i) % 11 for i in range(n_traj)]
    return Trajectories(np.array(beg), np.array(end), mt, system=np.arange(n_traj) % n_sys if n_sys > 1 else None)


def _branching_trajectories(N, n_traj, n_sys, n_steps, seed):
    """trajectories that share their MTO-free start (a two-time sweep: trajectory i branches off at t1_i and runs to the
    end), with an applyBefore MTO, a second later MTO, MTO-free ones, MTOs at step 0, a window that opens before the MTO
    and one that ends early (tests/test_gpu_branching.py g2_reuse_shape)"""
    from pyaceqd_amd.engine import MTO, Trajectories
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    B = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    A, B = A / np.linalg.norm(A), B / np.linalg.norm(B)
    beg, end, mt = [], [], []
    for i in range(n_traj):
        t1, kind = int(i * (n_steps - 2) / max(1, n_traj - 1)), i % 7
        if kind == 3:
            mt.append(MTO(i, max(t1, 1), True, 0, A))
        elif kind == 6:
            mt += [MTO(i, 0, False, 2, A), MTO(i, 0, False, 1, B)]
        elif kind != 5:
            mt += [MTO(i, t1, False, 2, A), MTO(i, t1, False, 1, B)]
            if kind == 4:
                mt.append(MTO(i, min(n_steps, t1 + 3), False, 1, B))
        beg.append(max(0, t1 - 2) if kind == 2 else t1)
        end.append(n_steps if kind != 1 else max(t1, n_steps - 4))
    return Trajectories(np.array(beg), np.array(end), mt, system=np.arange(n_traj) % n_sys if n_sys > 1 else None)


def _schedule(n_slices, seed):
    """a new slice at about four steps of five, the same slice again at the others"""
    rng = np.random.default_rng(seed)
    s = np.zeros(N_STEPS, dtype=np.int32)
    for n in range(1, N_STEPS):
        s[n] = s[n - 1] if rng.random() < 0.2 else (s[n - 1] + 1 + rng.integers(0, n_slices - 1)) % n_slices
    return s


def _mapchain_child(kind, p):
    """the outputs of one map-chain case; maps, operators and states as in tests/test_gpu_mapchain_paths.py"""
    from pyaceqd_amd.timebin import timebin_tl as TB
    from pyaceqd_amd.two_time import propagate_tau_module as M
    from tests import helpers as H
    dim = p["N"]
    N2 = dim * dim
    rng = np.random.default_rng(900 + 10 * dim + p.get("mode", 0))
    mk = lambda: np.eye(N2) + 0.05 * (rng.normal(size=(N2, N2)) + 1j * rng.normal(size=(N2, N2))) / dim  # noqa: E731
    F = lambda maps: np.asfortranarray(np.asarray(maps).transpose(1, 2, 0))  # noqa: E731
    if kind in ("ft8", "ft4", "dyn"):
        z = H.timebin_inputs(dim)
        a = (z["dm_1"], z["dm_2"], z["rho"], z["t1"], z["precalc"], z["dt"], z["dim"])
        if kind == "ft8":
            return {"G": TB.four_time_8op(*a, *z["ops8"], *p["flags"], z["tb"])}
        if kind == "ft4":
            return {"G": TB.four_time(*a, *z["ops8"][:4], z["tb"])}
        return {"rho": TB.dynamics_t1(*a, z["tb"])}
    rho = H.random_rho(dim).reshape(N2)
    if kind == "propagate_tau":
        maps = F([mk() for _ in range(30)])
        return {f"n_tau={n}_j_start={j}": M.propagate_tau(maps, rho, n, dim, j) for n, j in ((0, 0), (25, 0), (5, 25))}
    if kind == "map_tail":
        X = rng.normal(size=(N2, 37)) + 1j * rng.normal(size=(N2, 37))  # 37 rows: the last wave is part-filled
        w = rng.normal(size=N2) + 1j * rng.normal(size=N2)
        return {"out": M.map_tail(mk(), X, w, 300)}
    n_t = max(2 * (64 // N2) + 1, 7)  # odd: full waves and a part-filled last one (dim 6: one trajectory a wave)
    ops = [rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)) for _ in range(3)]
    if p["mode"] == 0:
        n_tau, n_tfull = 40, 260
        maps = F([mk() for _ in range(n_tfull - 1)])
        time = np.round(np.arange(n_tfull) * 0.1, 6)
        ts = np.sort(np.concatenate([[0.0, 0.05, 0.8], np.round(rng.uniform(0.0, 10.85, n_t - 3), 2)]))
        return {"G": M.calc_onetime_parallel(maps, rho, n_tau, dim, *ops, time, ts)}
    time = np.round(np.arange(60) * 0.1, 6)
    if p["mode"] == 1:
        n_tb, nx_tau, n_map = 12, 9, 7
        # trunk ends j = 1 + #{time < ts}: 1, inside n_tb, n_tb, n_tb + 1 and past it
        ts = np.sort(np.concatenate([[0.0, 0.4, 1.1, 1.2, 3.3], np.round(rng.uniform(0.0, 2.4, n_t - 5), 2)]))
        return {"G": M.calc_onetime_parallel_block(F([mk() for _ in range(n_map)]), np.asfortranarray(mk()), rho, n_tb,
                                                   nx_tau, dim, *ops, time, ts)}
    n_tb, nx_tau, n_map, n_tauc = 5, 3, 7, n_t // 2
    sep1, sep2, dm_s = F([mk() for _ in range(n_map)]), F([mk() for _ in range(n_map)]), np.asfortranarray(mk())
    tc = np.zeros((N2, N2, n_tauc, n_map), dtype=complex, order="F")
    for i in range(n_tauc):
        for jj in range(n_map):
            tc[:, :, i, jj] = mk()
    ts = np.sort(np.concatenate([[0.0, 0.15, 0.4, 0.5, 0.85], np.round(rng.uniform(0.0, 1.2, n_t - 5), 2)]))
    return {"G": M.calc_twotime_phonon_block(tc, sep1, sep2, dm_s, rho, n_tb, nx_tau, dim, *ops, time, ts)}


def _child(case, out):
    kind, p, _, want = _cases()[case]
    if kind not in ("pt", "free"):
        return np.savez(out, **_mapchain_child(kind, p))
    from pyaceqd_amd import engine, pt as ptmod
    from pyaceqd_amd.engine import Grid
    from tests import helpers as H
    N = p["N"]
    res = {}
    if kind == "free":
        sysd, grid = H.random_system(N, n_steps=12, n_sub=2, dt=1.0, seed=7 * N)
        res["M"] = engine.free_propagators(sysd, grid)
    else:
        chi = p["chi"]
        n_traj = p.get("n_traj", max(1, min(7, 256 // (N * N + 1))))  # every group resident
        ops = [H.ketbra(N, 0, 0), H.ketbra(N, 1, 0), np.eye(N)]
        rho0 = H.random_rho(N)
        if "live" in p:
            # a drive that leaves Liouville rows exactly zero (tests/test_gpu_live_rows.py), four outputs
            import dataclasses
            from tests import live_rows_cases
            systems, grid, rho0, ops, tr, _ = live_rows_cases.build(p["live"], 4)
            # one slice per row in a shuffled order, 5 slice sets
            pt = ptmod.random_pt(N, chi, D=N * N, n_slices=5, seed=chi + 16, eps=0.12)
            pt = dataclasses.replace(pt, gmap=np.random.default_rng(chi).permutation(N * N).astype(np.int32))
        elif "late" in p or "branch" in p:
            n_steps = p.get("late", 36)
            n_sys = p.get("n_sys", 1 if "late" in p else 2)
            systems = [H.random_system(N, n_steps=n_steps, seed=80 + k)[0] for k in range(n_sys)]
            grid = Grid(0.0, 0.1, n_steps)
            if n_sys == 1:
                systems = systems[0]
            if "late" in p:
                tr = _late_trajectories(N, n_traj, n_sys, n_steps)
            else:
                tr = _branching_trajectories(N, p["branch"], n_sys, n_steps, seed=N + chi)
            pt = ptmod.random_pt(N, chi, D=min(N * N, 9), n_slices=12, seed=chi + N, eps=0.12)
        else:
            systems = [H.random_system(N, n_steps=N_STEPS, seed=40 + k)[0] for k in range(3)]
            grid = Grid(0.0, 0.1, N_STEPS)
            tr = _trajectories(N, n_traj, seed=N + chi)
            tr.system = np.array([k % 3 for k in range(n_traj)])
            pt = None
            if chi > 1:
                pt = ptmod.random_pt(N, chi, D=min(N * N, 9), n_slices=9, seed=chi + N, eps=0.05)
                sched = _schedule(9, seed=chi + 7 * N)
                pt.schedule = lambda n_steps: np.ascontiguousarray(sched[:n_steps])
        plan = engine.Plan(systems, grid, rho0, ops, tr, pt=pt)
        d = plan.describe()
        desc = " ".join(f"{k}={v}" for k, v in sorted(d.items()))
        plan.execute()
        for t, a in enumerate(plan.download()):
            res[f"out{t:03d}"] = a
        path, bt, fb = plan.info()
        if want is not None and path != want:
            raise SystemExit(f"{case}: ran on '{path}', not on '{want}'")
        res["info"] = np.array(f"path={path} bt={bt} split_fallbacks={fb}")
        if path == BATCHED:
            sw = dict(lean=plan.sweep_lean(), readout=plan.sweep_readout(), stage=plan.sweep_stage())
            res["info"] = np.array(f"{res['info']} " + " ".join(f"{k}={int(v)}" for k, v in sw.items()))
            sw.update(stage=sw["stage"] > 0, staging=sw["stage"], parts=d.get("parts", "0"), branch=d["branch"],
                      trunks=int(d["n_trunk"]) > 0, shared=plan.traj_steps() < int(np.sum(tr.out_end + 1)))
            bad = {k: (sw[k], v) for k, v in p.get("want", {}).items() if sw[k] != v}
            if bad:
                raise SystemExit(f"{case}: (found, wanted) {bad}")
        res["describe"] = np.array(desc)
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default="")
    ap.add_argument("--names", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return _child(a.child, a.out)
    if len(a.libs) != 2:
        ap.error("two library paths")
    libs = [os.path.abspath(x) for x in a.libs]
    log = open(a.log, "w") if a.log else None

    def say(line):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    names = a.names.split(",") if a.names else a.libs
    say(f"# A = {names[0]}  B = {names[1]}; one child process per case and library; np.array_equal on every output, "
        "the plan's path, fallbacks and description as text")
    n_diff = 0
    cases = {k: v for k, v in _cases().items() if any(t in k for t in a.only.split(","))}
    with tempfile.TemporaryDirectory() as tmp:
        for cid, (_, _, sw, _) in cases.items():
            got = []
            for i, lib in enumerate(libs):
                env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
                env["PQD_LIB"] = lib
                assert all(k in SWITCHES for k in sw)
                env.update({k: str(v) for k, v in sw.items()})
                out = os.path.join(tmp, f"{i}.npz")
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cid, "--out", out],
                                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
                except subprocess.TimeoutExpired:
                    say(f"CHILD TIMED OUT {cid} lib {'AB'[i]}")
                    return 2
                if r.returncode != 0:
                    say(f"CHILD FAILED {cid} lib {'AB'[i]} exit {r.returncode}\n{r.stdout[-2000:]}")
                    return 2
                with np.load(out) as z:
                    got.append({k: z[k] for k in z.files})
            A, B = got
            bad = [k for k in sorted(set(A) | set(B))
                   if k not in A or k not in B or A[k].shape != B[k].shape or not np.array_equal(A[k], B[k])]
            n_diff += bool(bad)
            what = (str(A["info"]) if "info" in A else f"M{tuple(A['M'].shape)}" if "M" in A
                    else ", ".join(f"{k}{tuple(v.shape)}" for k, v in sorted(A.items())))
            say(f"{'DIFFER ' + ','.join(bad) if bad else 'equal '} {cid}  [{len(A)} arrays; {what}]")
    say(f"# {len(cases)} cases, {n_diff} differ")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
