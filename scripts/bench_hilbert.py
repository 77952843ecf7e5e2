"""Kernel time of the Hilbert-space no-PT path (csrc/lind_hilbert.hip, PQD_PATH_HILBERT) at the cavity models' sizes.

Jobs: a 256-point pulse-area scan (one system per area, one trajectory each) over 2,000 steps of 0.05 ps, one output
per level of the dot, with the models' decay and cavity-loss terms:
  (a) tls_photons        dim 18 (two-level system, two cavity modes of 3 levels)
      biexciton_photons  dim 16 (biexciton, two cavity modes of 2 levels)
  (b) tls_photon         dim 6, twice: on the default no-PT path (free propagators + one wave per trajectory) and forced
                         onto the Hilbert-space path in a child process (PQD_HILBERT=1 is read at plan creation); the
                         only like-for-like comparison with existing code. `ratio` = Hilbert kernel / default kernels
  (c) the host yardstick: tests/helpers.numpy_propagate's work per step at dim 18 (scipy expm of the 324 x 324
      Liouvillian, two half steps), timed on a few steps
One JSON line per run:
  kernel_ms   median over the executes of the plan's device-event time (pqd_plan_timing: free propagators + sweep;
              the Hilbert path has no free-propagator kernel), after one warm-up execute
  flop        the FP64 operations of the algorithm from the shapes: per Taylor term 8 (2 N^3 + 2 N nnz) (K T + T K^dag
              and the two passes over the jump operators' nonzeros), times the terms sum_substeps s * deg of every
              system from the kernel's own step bound, restated here
  valu_share  flop / kernel time over the 78.6 TFLOP/s FP64 vector peak of the MI355X
usage: python scripts/bench_hilbert.py [--jobs a,b,c] [--points 256] [--steps 2000] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

FP64_VALU_PEAK = 78.6e12  # flop / s
DT = 0.05


def build_job(model, n_points, n_steps):
    """systems of a pulse-area scan of `model`, grid, rho0, output operators, trajectories"""
    from pyaceqd_amd import opgrammar
    from pyaceqd_amd.constants import hbar
    from pyaceqd_amd.engine import Grid, System, Trajectories
    from pyaceqd_amd.four_level_system.linear import biexciton_photons_ops
    from pyaceqd_amd.two_level_system.tls import tls_composite_ops
    if model == "tls_photons":
        cav = (3, 0.06, 0.12 / hbar, -2)
        system_op, _, lind, inter, _, initial, _ = tls_composite_ops([cav, cav], [], 0.01, True, False, None, None)
        outs = ["|{0}><{0}|_2 otimes Id_3 otimes Id_3".format(k) for k in range(2)]
    elif model == "tls_photon":
        system_op, _, lind, inter, _, initial, _ = tls_composite_ops([(3, 0.06, 0.12 / hbar, -2)], [], 0.01, True,
                                                                     False, None, None)
        outs = ["|{0}><{0}|_2 otimes Id_3".format(k) for k in range(2)]
    else:
        system_op, _, lind, inter, _ = biexciton_photons_ops(2, 2, delta_xy=0.1, lindblad=True)
        initial = "|0><0|_4 otimes |0><0|_2 otimes |0><0|_2"
        outs = ["|{0}><{0}|_4 otimes Id_2 otimes Id_2".format(k) for k in range(4)]
    N = opgrammar.to_matrix(initial).shape[0]
    mat = lambda s: opgrammar.to_matrix(s, N)  # noqa: E731
    H0 = sum(mat(s) for s in system_op)
    T = DT * n_steps
    ds = DT / 4
    ts = ds * np.arange(4 * n_steps + 1)
    env = np.exp(-0.5 * ((ts - 0.3 * T) / (0.05 * T)) ** 2) / (np.sqrt(2 * np.pi) * 0.05 * T) * np.exp(-1j * 0.3 * ts)
    systems = []
    for area in np.linspace(0.5, 20.0, n_points):
        chans = [(-0.5 * np.pi * hbar * mat(op), area * env * (0.8 if pol == "x" else 0.6)) for op, pol in inter]
        systems.append(System(dim=N, H0=H0, lindblad=[(float(r), mat(o)) for o, r in lind], channels=chans,
                              sample_t0=0.0, sample_dt=ds))
    tr = Trajectories(np.zeros(n_points, dtype=int), np.full(n_points, n_steps), [], system=np.arange(n_points))
    return N, systems, Grid(0.0, DT, n_steps), mat(initial), [mat(o) for o in outs], tr


def taylor_terms(systems, grid):
    """sum over systems and sub-steps of s * deg, from the kernel's step bound (lind_hilbert.hip header)"""
    w = 0.5 * grid.dt / grid.n_sub
    tm = (grid.ta + 0.5 * grid.dt * np.arange(2 * grid.n_steps)[:, None]
          + (np.arange(grid.n_sub)[None, :] + 0.5) * w).reshape(-1)
    total = 0
    for sy in systems:
        mih = -1j / sy.hbar
        K0 = mih * np.asarray(sy.H0, dtype=complex)
        nD = 0.0
        for g, A in sy.lindblad:
            K0 = K0 - 0.5 * g * A.conj().T @ A
            nD += abs(g) * np.linalg.norm(A) ** 2
        nk = np.full(len(tm), np.linalg.norm(K0))
        for X, f in sy.channels:
            tf = sy.sample_t0 + sy.sample_dt * np.arange(len(f))
            fa = np.abs(np.interp(tm, tf, f.real) + 1j * np.interp(tm, tf, f.imag))
            nk = nk + fa * 2 * np.linalg.norm(mih * X)
        theta = w * (2 * nk + nD)
        s = np.maximum(1, np.ceil(theta)).astype(int)
        x = theta / s
        deg = np.ones(len(tm), dtype=int)
        rem = 0.5 * x * x
        for _ in range(17):
            more = (deg < 18) & (rem * (deg + 2.0) / (deg + 2.0 - x) >= 2.0 ** -56)
            deg = deg + more
            rem = np.where(more, rem * x / (deg + 1), rem)
        total += int(np.sum(s * deg))
    return total


def run_plan(model, n_points, n_steps, min_ms=300.0):
    from pyaceqd_amd import engine
    N, systems, grid, rho0, outs, tr = build_job(model, n_points, n_steps)
    plan = engine.Plan(systems, grid, rho0, outs, tr)
    plan.execute()
    plan.synchronize()
    plan.timing()
    ms = []
    while len(ms) < 3 or (sum(ms) < min_ms and len(ms) < 50):
        plan.execute()
        plan.synchronize()
        f, s, _ = plan.timing()
        ms.append(f + s)
    out = plan.download()
    nnz = sum(int(np.count_nonzero(A)) for _, A in systems[0].lindblad)
    return dict(model=model, N=N, points=n_points, steps=n_steps, path=plan.describe()["path"], executes=len(ms),
                kernel_ms=round(float(np.median(ms)), 4), kernel_ms_min=round(float(np.min(ms)), 4),
                kernel_ms_max=round(float(np.max(ms)), 4), nnz_jump=nnz,
                checksum=float(np.sum(np.abs(np.concatenate([o.ravel() for o in out]))))), systems, grid


def with_flops(r, systems, grid):
    terms = taylor_terms(systems, grid)
    flop = 8.0 * (2 * r["N"] ** 3 + 2 * r["N"] * r["nnz_jump"]) * terms
    r.update(taylor_terms=terms, flop=flop, tflops=round(flop / (1e-3 * r["kernel_ms"]) / 1e12, 3),
             valu_share=round(flop / (1e-3 * r["kernel_ms"]) / FP64_VALU_PEAK, 4))
    return r


def job_a(n_points, n_steps):
    for model in ("tls_photons", "biexciton_photons"):
        r, systems, grid = run_plan(model, n_points, n_steps)
        yield dict(job="a", **with_flops(r, systems, grid))


def job_b(n_points, n_steps):
    r0, systems, grid = run_plan("tls_photon", n_points, n_steps)
    env = dict(os.environ, PQD_HILBERT="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-b", "--points", str(n_points),
                            "--steps", str(n_steps)], env=env, capture_output=True, text=True)
    if child.returncode != 0:
        raise RuntimeError("forced-path child failed:\n" + child.stdout + child.stderr)
    r1 = json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("{")][-1])
    yield dict(job="b", variant="default", **r0)
    yield dict(job="b", variant="PQD_HILBERT=1", **r1)
    yield dict(job="b", variant="ratio", ratio_hilbert_over_default=round(r1["kernel_ms"] / r0["kernel_ms"], 4),
               checksum_rel_diff=abs(r1["checksum"] - r0["checksum"]) / abs(r0["checksum"]))


def job_c(n_steps=4):
    sys.path.insert(0, os.path.join(HERE))
    from tests import helpers
    N, systems, grid, rho0, outs, tr = build_job("tls_photons", 1, n_steps)
    from pyaceqd_amd.engine import Trajectories
    one = Trajectories(np.array([0]), np.array([n_steps]), [])
    t0 = time.perf_counter()
    helpers.numpy_propagate(systems[0], grid, rho0, outs, one)
    dt = time.perf_counter() - t0
    yield dict(job="c", model="tls_photons", N=N, steps=n_steps, host_s_per_step=round(dt / n_steps, 4),
               threads=os.environ.get("OMP_NUM_THREADS", ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="a,b,c")
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child-b", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_b:
        r, systems, grid = run_plan("tls_photon", a.points, a.steps)
        print(json.dumps(with_flops(r, systems, grid)), flush=True)
        return
    jobs = {"a": lambda: job_a(a.points, a.steps), "b": lambda: job_b(a.points, a.steps), "c": job_c}
    for j in a.jobs.split(","):
        for r in jobs[j]():
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
