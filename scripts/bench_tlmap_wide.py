"""Time of the time-localisation out[i] = dm[i] pinv(dm[i-1], 1e-12) (pqd_tl_dynmap_pseudo, csrc/tlmap_wide.hip) at the
sensor and cavity models' map sizes, modelled on scripts/bench_dynmap.py.

Inputs: the cumulative maps E(t_n, 0), n = 1 .. steps, of engine.dynmap_wide over 2,000 steps of 0.1 ps with
bench_dynmap.py's systems:
  tls_two_sensor     dim 8,  n = 64   (131 MB)
  biexciton_photons  dim 16, n = 256  (2.1 GB)
  tls_photons        dim 18, n = 324  (3.4 GB)
and `synthetic576`: 256 maps of n = 576 with complex normal entries (no model of dim 24 is needed for the limit).
Per size one JSON line, after a warm-up call on 3 maps:
  kernel_ms      device events around the kernel (pqd_tl_dynmap_timing)
  call_s         the whole tools.calc_tl_dynmap_pseudo call (upload, kernel, download)
  sweeps_max     the largest Jacobi sweep count over the maps (pqd_tl_dynmap_sweeps)
  host_subset, host_subset_s, host_s_scaled
                 the reference's loop (numpy.linalg.pinv(dm[i-1], rcond=1e-12) and the product) on `host_subset` maps
                 spread evenly over the set, with the process's BLAS threads (`threads`: OMP_NUM_THREADS), and that
                 time scaled to all n_maps - 1 maps
  rel_diff_max, rel_diff_median
                 max|gpu - numpy| / max|numpy| per map of the subset
  resid_gpu_max, resid_numpy_max
                 max|X dm[i-1] - dm[i]| / max|dm[i]| over the subset for X = the GPU's and numpy's time-local map: how
                 well each reproduces the step it stands for (both drop the directions below the cut)
  fp64_share_upper
                 (n_maps - 1) (sweeps_max 26 n^3 + 16 n^3) flops / kernel time / 78.6 TF/s: an upper bound of the share
                 of the FP64 vector peak (every map charged the largest sweep count, every pair a full rotation)
usage: python scripts/bench_tlmap_wide.py [--models tls_two_sensor,biexciton_photons,tls_photons,synthetic576]
       [--steps 2000] [--subset 32] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))

FP64_VECTOR_PEAK = 78.6e12


def maps_of(model, steps):
    if model == "synthetic576":
        rng = np.random.default_rng(576)
        return rng.normal(size=(256, 576, 576)) + 1j * rng.normal(size=(256, 576, 576))
    from bench_dynmap import build_system
    from pyaceqd_amd import engine
    sysd, grid = build_system(model, steps)
    return engine.dynmap_wide(sysd, grid)[0]


def gpu_run(dm):
    from pyaceqd_amd import _lib, tools
    times = np.arange(len(dm) + 1) * 0.1
    t0 = time.perf_counter()
    out = tools.calc_tl_dynmap_pseudo(dm, times)
    call_s = time.perf_counter() - t0
    ctx = _lib.context()
    ms, sw = C.c_double(0.0), C.c_int32(0)
    _lib.check(_lib.lib().pqd_tl_dynmap_timing(ctx.handle, C.byref(ms)))
    _lib.check(_lib.lib().pqd_tl_dynmap_sweeps(ctx.handle, C.byref(sw)))
    return out, ms.value, call_s, sw.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="tls_two_sensor,biexciton_photons,tls_photons,synthetic576")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--subset", type=int, default=32)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for model in a.models.split(","):
        dm = np.ascontiguousarray(maps_of(model, a.steps), dtype=np.complex128)
        n_maps, n = dm.shape[0], dm.shape[1]
        gpu_run(dm[:3])
        out, kernel_ms, call_s, sweeps = gpu_run(dm)
        idx = np.unique(np.linspace(1, n_maps - 1, min(a.subset, n_maps - 1)).astype(int))
        t0 = time.perf_counter()
        ref = [dm[i] @ np.linalg.pinv(dm[i - 1], rcond=1e-12) for i in idx]
        host_s = time.perf_counter() - t0
        diff = [float(np.max(np.abs(out[i] - r)) / np.max(np.abs(r))) for i, r in zip(idx, ref)]
        res = lambda X, i: float(np.max(np.abs(X @ dm[i - 1] - dm[i])) / np.max(np.abs(dm[i])))  # noqa: E731
        resid_gpu = max(res(out[i], i) for i in idx)
        resid_np = max(res(r, i) for i, r in zip(idx, ref))
        flops = (n_maps - 1) * (sweeps * 26.0 + 16.0) * float(n) ** 3
        emit(dict(model=model, n=n, n_maps=n_maps, kernel_ms=round(kernel_ms, 3), call_s=round(call_s, 4),
                  sweeps_max=sweeps, bytes=int(dm.nbytes), host_subset=len(idx), host_subset_s=round(host_s, 4),
                  host_s_scaled=round(host_s * (n_maps - 1) / len(idx), 2),
                  threads=os.environ.get("OMP_NUM_THREADS"), rel_diff_max=max(diff),
                  rel_diff_median=float(np.median(diff)), resid_gpu_max=resid_gpu, resid_numpy_max=resid_np,
                  fp64_share_upper=round(flops / (kernel_ms * 1e-3) / FP64_VECTOR_PEAK, 4)))
        del dm, out, ref


if __name__ == "__main__":
    main()
