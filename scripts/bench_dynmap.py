"""Time of one dynamical map on the Hilbert-space path (pqd_dynmap_wide: the map instance of csrc/lind_hilbert.hip and
the device-side assembly) at the sensor and cavity models' sizes, modelled on scripts/bench_hilbert_pt.py.

Jobs: one map E(t_n, 0), n = 1 .. steps, over 2,000 steps of 0.1 ps with the models' decay, cavity-loss and sensor
terms and a Gaussian pulse:
  tls_two_sensor     dim 8   (map of 131 MB)
  biexciton_photons  dim 16  (2.1 GB)
  tls_photons        dim 18  (3.4 GB)
Per model one JSON line per run:
  map      engine.dynmap_wide: kernel_ms (device events around the map instance, after a warm-up call of 20 steps),
           call_s (the whole call: upload, kernel, assembly, finite check, download), bytes
  trace    (dim 8 and 16 only: N^2 <= 256 outputs) the route through N^2 trace outputs on N^2 MTO-prepared trajectories,
           engine.propagate as general_system._dynmap calls it: kernel_ms (the plan's device events), call_s (the whole
           engine.propagate call and the np.stack of its result into the map layout)
The two routes alternate `--reps` times, so the spread of repeated runs shows beside their difference; `equal` says
whether the two routes' maps are the same bits.
usage: python scripts/bench_dynmap.py [--models tls_two_sensor,biexciton_photons,tls_photons] [--steps 2000] [--reps 2]
       [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

DT = 0.1


def build_system(model, n_steps):
    """the model's System with its decay terms on a grid of n_steps steps (the drop-in layer's lowering)"""
    from pyaceqd_amd.pulses import ChirpedPulse
    T = DT * n_steps
    pulse = ChirpedPulse(tau_0=0.05 * T, e_start=0.0, e0=3.0, t0=0.3 * T)
    if model == "biexciton_photons":
        from pyaceqd_amd.four_level_system.linear import biexciton_photons as fn
    else:
        from pyaceqd_amd.two_level_system import tls as mod
        fn = getattr(mod, model)
    low = fn(0, T, pulse, dt=DT, lindblad=True, lower_only=True)
    return low.systems[0], low.grid


def run_map(sysd, grid):
    from pyaceqd_amd import engine
    t0 = time.perf_counter()
    dm = engine.dynmap_wide(sysd, grid)[0]
    call_s = time.perf_counter() - t0
    return dm, dict(kernel_ms=round(engine.dynmap_kernel_ms(), 4), call_s=round(call_s, 4), bytes=int(dm.nbytes))


def trace_job(sysd, grid):
    from pyaceqd_amd.engine import MTO, Trajectories
    N = sysd.dim
    N2 = N * N
    ket = lambda a, b: np.outer(np.eye(N)[a], np.eye(N)[b]).astype(complex)  # noqa: E731
    ops = [ket(a % N, a // N) for a in range(N2)]
    mtos = []
    for beta in range(N2):
        i, j = divmod(beta, N)
        mtos += [MTO(beta, 0, True, 1, ket(i, 0)), MTO(beta, 0, True, 2, ket(0, j))]
    return ket(0, 0), ops, Trajectories(np.zeros(N2, dtype=int), np.full(N2, grid.n_steps), mtos)


def run_trace(sysd, grid, job):
    from pyaceqd_amd import engine
    rho0, ops, tr = job
    t0 = time.perf_counter()
    dm = np.stack(engine.propagate(sysd, grid, rho0, ops, tr), axis=2)[1:]
    call_s = time.perf_counter() - t0
    plan = engine.Plan(sysd, grid, rho0, ops, tr)  # the same launch again, for its device events
    plan.execute()
    plan.synchronize()
    _, ms, _ = plan.timing()
    return dm, dict(kernel_ms=round(ms, 4), call_s=round(call_s, 4), bytes=int(dm.nbytes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="tls_two_sensor,biexciton_photons,tls_photons")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    from pyaceqd_amd import engine
    from pyaceqd_amd.engine import Grid

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for model in a.models.split(","):
        sysd, grid = build_system(model, a.steps)
        N = sysd.dim
        warm = Grid(grid.ta, grid.dt, 20, grid.n_sub)
        engine.dynmap_wide(sysd, warm)
        job = trace_job(sysd, grid) if N * N <= 256 else None
        if job is not None:
            engine.propagate(sysd, warm, job[0], job[1], trace_job(sysd, warm)[2])
        for rep in range(a.reps):
            dm, r = run_map(sysd, grid)
            emit(dict(model=model, run="map", N=N, steps=grid.n_steps, rep=rep, **r,
                      checksum=float(np.sum(np.abs(dm[-1])))))
            if job is not None:
                old, r = run_trace(sysd, grid, job)
                emit(dict(model=model, run="trace", N=N, steps=grid.n_steps, rep=rep, **r,
                          equal=bool(np.array_equal(old, dm))))
                del old
            del dm


if __name__ == "__main__":
    main()
