"""Time of calc_onetime_parallel_block on the periodic sweep by position (pqd_calc_onetime_parallel_block_wide,
csrc/mapchain_wide.hip) at the cavity and sensor models' sizes, in the manner of scripts/bench_mapchain_wide.py.

Shape (every dim): a period of n_tb = 1024 positions, n_map = 256 block maps (n_map < n_tb: the rest of a period is
dm_s; --n-map changes it, and with it the number of positions where the two cursors differ), nx_tau = 2
(n_tau = 2048), 256 trajectories whose trunk ends are 4 positions apart over the period (the ring cursor) and one at
t = tb (trunk end n_tb: the straight cursor, as Purity's add_tend point), 3072 positions in all.
Inputs: near-identity maps 1 + eps G (complex normal G, eps = 2e-3 / sqrt(n)); the block maps cycle through a pool of 8.
Per size one JSON line:
  call_s          median wall time of `reps` propagate_tau_module.calc_onetime_parallel_block(wide=True) calls after a
                  warm-up call: schedule, upload of the block maps and dm_s, kernels, download
  kernel_ms       device events around the kernels of the last call (pqd_mc_wide_timing), launches: their number
  steps, two_family, cols_per_step
                  from pqd_mc_wide_block_schedule: positions with a step launch, those among them where the two
                  cursors name different maps and both have a live column (two families in one launch), and the live
                  columns (trajectories in flight and the trunk state) per step
  us_per_launch   kernel_ms / launches (the steps, one weights launch and 257 spawn launches)
  fp64_share      8 n (n + 1) (column steps) flops / kernel time / 78.6 TF/s, the FP64 matrix peak
  onetime_us_per_launch, onetime_launches, onetime_cols_per_step
                  the yardstick of the per-position cost: calc_onetime_parallel (one cursor, one family) at the same n
                  with 257 trajectories one position apart and n_tau = 380 (a stack of 636 maps, 3.4 GB at dim 24):
                  its kernel_ms / launches (636 steps, one weights launch, 257 spawn launches), their number and its
                  live columns per step
  cpu_s, cpu_traj, cpu_s_scaled, cpu
                  the same block sweep for `cpu_traj` of the ring trajectories (every 256 / cpu_traj-th) and the
                  straight one through the reference's Fortran (oracle/_ref, `cpu` = "fortran") or, where that is
                  absent, the C oracle (`cpu` = "oracle"), on `threads` host threads;
                  cpu_s_scaled = cpu_s * 257 / (cpu_traj + 1) (trajectories are independent there)
  rel_diff_max    max|gpu - cpu| / max|cpu| over those trajectories
usage: python scripts/bench_mapchain_block_wide.py [--dims 8,16,18,24] [--n-map 256] [--reps 5] [--cpu-traj 32]
       [--threads 16] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# the reference's Fortran calls zgemv from inside its OpenMP loop over the trajectories: one BLAS thread per call, set
# before any BLAS is loaded (scripts/bench_mapchain_wide.py)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

FP64_MATRIX_PEAK = 78.6e12
N_TB, NX_TAU, N_RING, SPREAD = 1024, 2, 256, 4
ONETIME_N_TAU = 380


def near_identity(rng, n):
    return np.asfortranarray(np.eye(n) + 2e-3 / np.sqrt(n) * (rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))))


def inputs(dim, n_map):
    n = dim * dim
    rng = np.random.default_rng(dim)
    pool = [near_identity(rng, n) for _ in range(8)]
    dm_block = np.empty((n, n, n_map), dtype=np.complex128, order="F")
    for q in range(n_map):
        dm_block[:, :, q] = pool[q % 8]
    dm_s = near_identity(rng, n)
    ends = np.append(SPREAD * np.arange(N_RING), N_TB)
    time_full = 0.1 * np.arange(N_TB + 2)
    ts = time_full[ends]   # on the map grid: `time < ts` stops at the grid point, trunk end = ends
    rho = np.zeros(n, complex)
    rho[0] = 1
    ops = [np.asfortranarray(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim))) for _ in range(3)]
    return pool, dm_block, dm_s, rho, ops, time_full, ts


def timing(_lib):
    ms, nl = C.c_double(), C.c_int32()
    _lib.check(_lib.lib().pqd_mc_wide_timing(_lib.context().handle, C.byref(ms), C.byref(nl)))
    return ms.value, nl.value


def block_schedule(_lib, time_full, ts, n_map):
    rows = C.c_int32()
    a = (_lib.fptr(np.ascontiguousarray(time_full)), len(time_full), _lib.fptr(np.ascontiguousarray(ts)), len(ts), N_TB,
         NX_TAU, n_map)
    _lib.check(_lib.lib().pqd_mc_wide_block_schedule(*a, None, C.byref(rows), None, 0))
    sched = np.zeros((rows.value, 9), dtype=np.int32)
    _lib.check(_lib.lib().pqd_mc_wide_block_schedule(*a, None, C.byref(rows), _lib.iptr(sched), rows.value))
    return sched[:-1]   # the last row holds spawns only


def onetime_yardstick(gpu, _lib, pool, rho, ops, dim):
    """(kernel us per launch, launches, live columns per step) of calc_onetime_parallel with 257 trajectories at this n"""
    n, n_t = dim * dim, N_RING + 1
    ends = np.arange(n_t)
    n_maps = int(ends[-1]) + ONETIME_N_TAU
    dm = np.empty((n, n, n_maps), dtype=np.complex128, order="F")
    for q in range(n_maps):
        dm[:, :, q] = pool[q % 8]
    time_full = 0.1 * np.arange(n_maps + 1)
    for _ in range(2):
        gpu.calc_onetime_parallel(dm, rho, ONETIME_N_TAU, dim, *ops, time_full, time_full[ends])
    ms, nl = timing(_lib)
    return 1e3 * ms / nl, nl, (n_t * ONETIME_N_TAU + int(ends[-1])) / n_maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="8,16,18,24")
    ap.add_argument("--n-map", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-traj", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    os.environ["OMP_NUM_THREADS"] = str(a.threads)
    from oracle import fref, oracle
    from pyaceqd_amd import _lib
    from pyaceqd_amd.two_time import propagate_tau_module as gpu

    for dim in (int(d) for d in a.dims.split(",")):
        pool, dm_block, dm_s, rho, ops, time_full, ts = inputs(dim, a.n_map)
        n, n_t = dim * dim, len(ts)
        args = lambda t: (dm_block, dm_s, rho, N_TB, NX_TAU, dim, *ops, time_full, t)  # noqa: E731
        gpu.calc_onetime_parallel_block(*args(ts), wide=True)
        walls = []
        for _ in range(a.reps):
            got = None
            t0 = time.perf_counter()
            got = gpu.calc_onetime_parallel_block(*args(ts), wide=True)
            walls.append(time.perf_counter() - t0)
        ms, nl = timing(_lib)
        sched = block_schedule(_lib, time_full, ts, a.n_map)
        ring, straight = sched[:, 1] - sched[:, 0], sched[:, 4] - sched[:, 3] + sched[:, 5]
        steps = int(np.sum((ring > 0) | (straight > 0)))
        two = int(np.sum((ring > 0) & (straight > 0) & (sched[:, 2] != sched[:, 6])))
        col_steps = int(np.sum(ring) + np.sum(straight))
        one_us, one_nl, one_cols = onetime_yardstick(gpu, _lib, pool, rho, ops, dim)
        sub = np.append(np.arange(0, N_RING, N_RING // a.cpu_traj), N_RING)
        t0 = time.perf_counter()
        if fref.available():
            cpu, ref = "fortran", fref.calc_onetime_parallel_block(*args(ts[sub]))
        else:
            cpu, ref = "oracle", oracle.calc_onetime_parallel_block(*args(ts[sub]))
        cpu_s = time.perf_counter() - t0
        line = json.dumps(dict(
            dim=dim, n=n, n_t=n_t, n_tb=N_TB, nx_tau=NX_TAU, n_map=a.n_map, positions=len(sched),
            bytes=int(dm_block.nbytes + dm_s.nbytes), call_s=round(float(np.median(walls)), 4), kernel_ms=round(ms, 3),
            launches=nl, steps=steps, two_family=two, cols_per_step=round(col_steps / steps, 1),
            us_per_launch=round(1e3 * ms / nl, 2),
            fp64_share=round(8.0 * n * (n + 1) * col_steps / (ms * 1e-3) / FP64_MATRIX_PEAK, 4),
            onetime_us_per_launch=round(one_us, 2), onetime_launches=one_nl, onetime_cols_per_step=round(one_cols, 1), cpu=cpu, threads=a.threads,
            cpu_traj=len(sub), cpu_s=round(cpu_s, 3), cpu_s_scaled=round(cpu_s * n_t / len(sub), 2),
            rel_diff_max=float(np.max(np.abs(got[sub] - ref)) / np.max(np.abs(ref)))))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del dm_block, got, ref


if __name__ == "__main__":
    main()
