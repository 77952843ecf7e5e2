"""Time of calc_onetime_parallel on the sweep by position (pqd_calc_onetime_parallel above dim 6, csrc/mapchain_wide.hip)
at the cavity and sensor models' sizes, in the manner of scripts/bench_tlmap_wide.py.

Inputs: near-identity maps 1 + eps G (complex normal G, eps = 2e-3 / sqrt(n), as scripts/bench_mapchain.py); the stack
cycles through a pool of 8 such maps (filling 3.4 GB with fresh normal numbers would take longer than every timed call
together; the kernels read the stack, not the pool). 256 trajectories whose trunk ends are `spread` positions apart,
and a tau window as long as a 3.4 GB stack allows at each size:
  dim  8 (n =  64)   spread 4, n_tau 2000: 3020 maps, 0.20 GB
  dim 16 (n = 256)   spread 4, n_tau 1000: 2020 maps, 2.1 GB
  dim 18 (n = 324)   spread 4, n_tau 1000: 2020 maps, 3.4 GB
  dim 24 (n = 576)   spread 1, n_tau  380:  635 maps, 3.4 GB
Per size one JSON line:
  call_s          median wall time of 5 propagate_tau_module.calc_onetime_parallel calls after a warm-up call: schedule,
                  upload of the maps the sweep reads, kernels, download
  kernel_ms       device events around the kernels of the last call (pqd_mc_wide_timing), launches: their number
  us_per_launch   kernel_ms / launches
  fp64_share      8 n (n + 1) (column steps) flops / kernel time / 78.6 TF/s, the FP64 matrix peak; column steps: the
                  live columns summed over the positions (trajectories in flight and the trunk state)
  hbm_share       bytes of the maps read (twice: the weights pass and the steps) / kernel time / 8 TB/s
  cpu_s, cpu_traj, cpu_s_scaled, cpu
                  the same sweep for `cpu_traj` of the 256 trajectories (every 8th) through the reference's Fortran
                  (oracle/_ref, `cpu` = "fortran") or, where that is absent, the C oracle (`cpu` = "oracle"), on
                  `threads` host threads; cpu_s_scaled = cpu_s * 256 / cpu_traj (trajectories are independent there)
  rel_diff_max    max|gpu - cpu| / max|cpu| over those trajectories
usage: python scripts/bench_mapchain_wide.py [--dims 8,16,18,24] [--reps 5] [--cpu-traj 32] [--threads 16] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# the reference's Fortran calls zgemv from inside its OpenMP loop over the trajectories: a threaded OpenBLAS warns on
# every such call and runs them ten times slower. One BLAS thread per call, set before any BLAS is loaded
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

FP64_MATRIX_PEAK = 78.6e12
HBM_PEAK = 8.0e12
SHAPES = {8: (4, 2000), 16: (4, 1000), 18: (4, 1000), 24: (1, 380)}  # dim: (spread of the trunk ends, n_tau)
N_T = 256


def inputs(dim):
    spread, n_tau = SHAPES[dim]
    n = dim * dim
    ends = spread * np.arange(N_T)
    n_maps = int(ends[-1]) + n_tau
    rng = np.random.default_rng(dim)
    pool = [np.asfortranarray(np.eye(n) + 2e-3 / np.sqrt(n) * (rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))))
            for _ in range(8)]
    dm = np.empty((n, n, n_maps), dtype=np.complex128, order="F")
    for q in range(n_maps):
        dm[:, :, q] = pool[q % 8]
    time_full = 0.1 * np.arange(n_maps + 1)
    ts = time_full[ends]   # on the map grid: `time < ts` stops at the grid point, trunk end = ends
    rho = np.zeros(n, complex)
    rho[0] = 1
    ops = [np.asfortranarray(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim))) for _ in range(3)]
    return dm, rho, n_tau, ops, time_full, ts, ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="8,16,18,24")
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
        dm, rho, n_tau, ops, time_full, ts, ends = inputs(dim)
        n, n_maps = dim * dim, dm.shape[2]
        call = lambda t: gpu.calc_onetime_parallel(dm, rho, n_tau, dim, *ops, time_full, t)  # noqa: E731
        call(ts)
        walls = []
        for _ in range(a.reps):
            got = None
            t0 = time.perf_counter()
            got = call(ts)
            walls.append(time.perf_counter() - t0)
        ms, nl = C.c_double(), C.c_int32()
        _lib.check(_lib.lib().pqd_mc_wide_timing(_lib.context().handle, C.byref(ms), C.byref(nl)))
        col_steps = N_T * n_tau + int(ends[-1])
        sub = np.arange(0, N_T, N_T // a.cpu_traj)
        t0 = time.perf_counter()
        if fref.available():
            cpu, ref = "fortran", fref.calc_onetime_parallel(dm, rho, n_tau, dim, *ops, time_full, ts[sub])
        else:
            cpu, ref = "oracle", oracle.calc_onetime_parallel(dm, rho, n_tau, dim, *ops, time_full, ts[sub],
                                                              nthreads=a.threads)
        cpu_s = time.perf_counter() - t0
        line = json.dumps(dict(
            dim=dim, n=n, n_t=N_T, n_tau=n_tau, n_maps=n_maps, bytes=int(dm.nbytes), call_s=round(float(np.median(walls)), 4),
            kernel_ms=round(ms.value, 3), launches=nl.value, us_per_launch=round(1e3 * ms.value / nl.value, 2),
            fp64_share=round(8.0 * n * (n + 1) * col_steps / (ms.value * 1e-3) / FP64_MATRIX_PEAK, 4),
            hbm_share=round(2.0 * dm.nbytes / (ms.value * 1e-3) / HBM_PEAK, 4), cpu=cpu, threads=a.threads,
            cpu_traj=len(sub), cpu_s=round(cpu_s, 3), cpu_s_scaled=round(cpu_s * N_T / len(sub), 2),
            rel_diff_max=float(np.max(np.abs(got[sub] - ref)) / np.max(np.abs(ref)))))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del dm, got, ref


if __name__ == "__main__":
    main()
