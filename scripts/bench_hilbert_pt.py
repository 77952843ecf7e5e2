"""Kernel time of the Hilbert-space path with a process tensor (csrc/lind_hilbert_pt.hip, PQD_PATH_HILBERT_PT) at the
sensor and cavity models' sizes, modelled on scripts/bench_hilbert.py.

Jobs: a 256-point pulse-area scan (one system per area, one trajectory each) over 2,000 steps of 0.1 ps (the wrappers'
default dt), the occupations of the dot as outputs, with the models' decay, cavity-loss and sensor terms:
  tls_two_sensor  dim 8   (two-level system read by two sensors)
  tls_photons     dim 18  (two-level system, two cavity modes of 3 levels)
each with the PT of the wrapper's reference defaults (t_mem 10, threshold 1e-10, a_e and temperature of the wrapper;
the device generator, bond capped at ptgen.default_max_bond). Per model one JSON line per run:
  pt       the job on the new path: kernel_ms (median of the plan's device-event times after a warm-up execute), chi
  nopt     the same job without a PT on lind_hilbert_kernel (PQD_PATH_HILBERT)
  chi1     the same job with a chi = 1 PT (pt.markov_dephasing_pt): against `nopt` the price of the state living in
           the workspace instead of LDS
  ratios   per_slice = pt / (chi nopt): the time per bond slice relative to the no-PT run (1 = the model "chi times the
           no-PT time"); chi1_over_nopt
  g        (--jobs g) the `pt` job at fewer steps under PQD_HBPT_G caps: the A/B behind the default number of slices
           in flight
  flop     FP64 operations from the shapes: chi times bench_hilbert's Taylor count plus 8 N^2 chi^2 per step for the PT
usage: python scripts/bench_hilbert_pt.py [--models tls_two_sensor,tls_photons] [--jobs main,g] [--points 256]
       [--steps 2000] [--g-steps 200] [--t-mem 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))

FP64_VALU_PEAK = 78.6e12  # flop / s
DT = 0.1
BATH = {"tls_two_sensor": dict(ae=3.0, temperature=1), "tls_photons": dict(ae=5.0, temperature=4)}


def build_job(model, n_points, n_steps):
    """systems of a pulse-area scan of `model`, grid, rho0, output operators, trajectories, the coupling operator"""
    from pyaceqd_amd import opgrammar
    from pyaceqd_amd.constants import hbar
    from pyaceqd_amd.engine import Grid, System, Trajectories
    from pyaceqd_amd.two_level_system.tls import tls_composite_ops
    if model == "tls_photons":
        cav = (3, 0.06, 0.12 / hbar, -2)
        built = tls_composite_ops([cav, cav], [], 0.01, True, False, None, None)
    else:
        built = tls_composite_ops([], [(0, 0.01), (0, 0.01)], 0.01, True, False, None, 0.0001)
    system_op, boson_op, lind, inter, _, initial, outs = built
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
    return N, systems, Grid(0.0, DT, n_steps), mat(initial), [mat(o) for o in outs], tr, mat(boson_op)


def run_plan(job, pt, min_ms=300.0, max_executes=50):
    """median device-event time of the plan's executes after one warm-up; at least 3 executes"""
    from pyaceqd_amd import engine
    N, systems, grid, rho0, outs, tr, _ = job
    plan = engine.Plan(systems, grid, rho0, outs, tr, pt=pt, **({"wide_pt": True} if pt is not None else {}))
    plan.execute()
    plan.synchronize()
    plan.timing()
    ms = []
    while len(ms) < 3 or (sum(ms) < min_ms and len(ms) < max_executes):
        plan.execute()
        plan.synchronize()
        f, s, _ = plan.timing()
        ms.append(f + s)
    out = plan.download()
    return dict(N=N, points=len(systems), steps=grid.n_steps, path=plan.describe()["path"], executes=len(ms),
                kernel_ms=round(float(np.median(ms)), 4), kernel_ms_min=round(float(np.min(ms)), 4),
                kernel_ms_max=round(float(np.max(ms)), 4),
                checksum=float(np.sum(np.abs(np.concatenate([o.ravel() for o in out])))))


def model_pt(model, boson, t_mem):
    from pyaceqd_amd import ptgen_gpu
    t0 = time.perf_counter()
    pt = ptgen_gpu.qd_phonon_pt_gpu(boson, DT, t_mem=t_mem, threshold=1e-10, use_infinite=False, **BATH[model])
    return pt, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="tls_two_sensor,tls_photons")
    ap.add_argument("--jobs", default="main")
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--g-steps", type=int, default=200)
    ap.add_argument("--g-caps", default="0,4,2,1", help="PQD_HBPT_G values of job g (0: no cap)")
    ap.add_argument("--t-mem", type=float, default=10.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    from bench_hilbert import taylor_terms
    from pyaceqd_amd import pt as ptmod

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for model in a.models.split(","):
        job = build_job(model, a.points, a.steps)
        N, systems, grid, boson = job[0], job[1], job[2], job[6]
        pt, gen_s = model_pt(model, boson, a.t_mem)
        emit(dict(model=model, run="generated_pt", chi=pt.chi, D=pt.D, n_slices=pt.n_slices, n_init=pt.n_init,
                  seconds=round(gen_s, 2), truncation=(pt.meta or {}).get("truncation")))
        if "main" in a.jobs.split(","):
            r_no = run_plan(job, None)
            emit(dict(model=model, run="nopt", **r_no))
            r_1 = run_plan(job, ptmod.markov_dephasing_pt(boson, 0.01, DT, chi=1))
            emit(dict(model=model, run="chi1", chi=1, **r_1))
            r_pt = run_plan(job, pt, max_executes=5)
            nnz = sum(int(np.count_nonzero(A)) for _, A in systems[0].lindblad)
            flop = pt.chi * 8.0 * (2 * N ** 3 + 2 * N * nnz) * taylor_terms(systems, grid) \
                + 8.0 * N * N * pt.chi ** 2 * grid.n_steps * len(systems)
            emit(dict(model=model, run="pt", chi=pt.chi, flop=flop,
                      tflops=round(flop / (1e-3 * r_pt["kernel_ms"]) / 1e12, 3),
                      valu_share=round(flop / (1e-3 * r_pt["kernel_ms"]) / FP64_VALU_PEAK, 4), **r_pt))
            emit(dict(model=model, run="ratios", chi=pt.chi,
                      per_slice=round(r_pt["kernel_ms"] / (pt.chi * r_no["kernel_ms"]), 4),
                      chi1_over_nopt=round(r_1["kernel_ms"] / r_no["kernel_ms"], 4)))
        if "g" in a.jobs.split(","):
            gjob = build_job(model, a.points, a.g_steps)
            for rep in range(2):  # the caps alternate twice: the spread shows beside the differences
                for cap in a.g_caps.split(","):
                    if cap == "0":
                        os.environ.pop("PQD_HBPT_G", None)
                    else:
                        os.environ["PQD_HBPT_G"] = cap
                    emit(dict(model=model, run="g", cap=int(cap), rep=rep, chi=pt.chi,
                              **run_plan(gjob, pt, max_executes=3)))
            os.environ.pop("PQD_HBPT_G", None)


if __name__ == "__main__":
    main()
