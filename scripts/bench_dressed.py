"""Throughput of the dressed-state launch (csrc/dressed.hip and csrc/dressed_wide.hip through engine.dressed_states) at
the project's scan shapes.

One problem per (scan point, output time): H(t) is built and diagonalised on the device, the occupations are evaluated
against a density matrix per problem. Shapes (systems x output times):
  tls        two-level system, pulse-area scan           2,048 x  1,001
  bx_large   biexciton, pulse-area scan                  2,048 x 10,001
  bx_small   biexciton                                     256 x 10,001
  six        six-level dot in an in-plane field             32 x 10,001
  tlsph      tls_photons, dim 18 (dressed_wide.hip)        256 x  2,001
  bxph       biexciton_photons, dim 16 (dressed_wide.hip)  256 x  2,001
  sens24     tls_photon_two_sensor, dim 24 (")              32 x  2,001
Each shape runs with and without the eigenvector download (eigenvalues and occupations always come back) and prints
one JSON line per run:
  kernel_ms      median kernel duration from device events (pqd_dressed_timing), after a warm-up call, over enough
                 calls that the kernel durations add up to >= 0.3 s (at least 3 calls)
  call_ms        median wall time of the whole call: uploads (systems, rho), kernel, downloads
  bytes          what the kernel must read (rho) and write (eigenvalues, occupations, eigenvectors), from the shapes
  hbm_share      bytes / kernel time over the 8.0 TB/s HBM3E peak of the MI355X: the relevant bound, the arithmetic
                 is negligible
  eigh_*         numpy.linalg.eigh plus the occupation einsum on the same H(t) on the host (16 threads at most), on
                 `eigh_problems` of the problems (all of them up to --eigh-max); the only baseline there is
At dim 18 the eigenvectors are 5 KB per problem (2.7 GB for tlsph): with them call_ms is the download.
usage: python scripts/bench_dressed.py [--shapes tls,bx_large,bx_small,six,tlsph,bxph,sens24] [--eigh-max 400000]
                                       [--out FILE]            (default shapes: the four of dim <= 6)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

HBM_PEAK = 8.0e12  # bytes / s

SHAPES = {"tls": (2, 2048, 1001), "bx_large": (4, 2048, 10001), "bx_small": (4, 256, 10001), "six": (6, 32, 10001),
          "tlsph": (18, 256, 2001), "bxph": (16, 256, 2001), "sens24": (24, 32, 2001)}


def build_systems(name, n_sys, n_t, dt):
    """a pulse-area scan: every system the model's H0 and pulse channels, a Gaussian envelope scaled by its area"""
    from pyaceqd_amd import opgrammar
    from pyaceqd_amd.constants import hbar
    from pyaceqd_amd.engine import System
    from pyaceqd_amd.four_level_system.linear import biexciton_ops, biexciton_photons_ops
    from pyaceqd_amd.six_level_system.linear import sixls_ops
    from pyaceqd_amd.two_level_system.tls import tls_composite_ops
    cav = (3, 0.06, 0.12 / hbar, -2)   # a cavity mode of the models' defaults: levels, coupling, loss, detuning
    if name == "tls":
        N, system_op, inter = 2, ["0.2*|1><1|_2"], [["|1><0|_2", "x"]]
    elif name == "tlsph":
        N = 18
        system_op, _, _, inter = tls_composite_ops([cav, cav], [], 1 / 100, False, False, None, None)[:4]
    elif name == "sens24":
        N = 24
        system_op, _, _, inter = tls_composite_ops([cav], [(0, 0.01), (0, 0.01)], 1 / 100, False, False, None,
                                                   0.0001)[:4]
    elif name == "bxph":
        N = 16
        system_op, _, _, inter, _ = biexciton_photons_ops(2, 2, delta_xy=0.1, delta_b=4)
    elif name.startswith("bx"):
        N = 4
        system_op, _, _, inter, _ = biexciton_ops(delta_xy=0.1, delta_b=4)
    else:
        N = 6
        system_op, _, _, inter, _ = sixls_ops(delta_b=4, bx=2.0)
    H0 = sum(opgrammar.to_matrix(s, N) for s in system_op)
    T = dt * (n_t - 1)
    ts = dt * np.arange(n_t)
    env = np.exp(-0.5 * ((ts - 0.5 * T) / (0.1 * T)) ** 2) / (np.sqrt(2 * np.pi) * 0.1 * T) * np.exp(-1j * 0.3 * ts)
    systems = []
    for area in np.linspace(0.5, 20.0, n_sys):
        chans = [(-0.5 * np.pi * hbar * opgrammar.to_matrix(op, N), area * env * (0.8 if pol == "x" else 0.6))
                 for op, pol in inter]
        systems.append(System(dim=N, H0=H0, channels=chans, sample_t0=0.0, sample_dt=dt))
    return N, systems


def host_hamiltonians(systems, n_t, dt, idx):
    """H(t) of the problems idx (flat (system, time) indices); the samples sit on the grid, so no interpolation"""
    s_i, t_i = np.divmod(idx, n_t)
    H = np.repeat(np.asarray(systems[0].H0, dtype=complex)[None], len(idx), axis=0)   # one model: H0, X_p shared
    for c, (X, _) in enumerate(systems[0].channels):
        f = np.stack([sy.channels[c][1] for sy in systems])[s_i, t_i]
        H += f[:, None, None] * X[None] + f.conj()[:, None, None] * X.conj().T[None]
    return H


def run_shape(name, eigh_max):
    from pyaceqd_amd import engine
    from pyaceqd_amd.engine import Grid
    N, n_sys, n_t = SHAPES[name]
    dt = 0.05
    N_, systems = build_systems(name, n_sys, n_t, dt)
    grid = Grid(0.0, dt, n_t - 1)
    n_prob = n_sys * n_t
    rng = np.random.default_rng(3)
    B = rng.normal(size=(n_sys, 1, N, N)) + 1j * rng.normal(size=(n_sys, 1, N, N))
    R = B @ B.conj().transpose(0, 1, 3, 2)
    R /= np.trace(R, axis1=2, axis2=3)[..., None, None]
    rho = np.ascontiguousarray(np.broadcast_to(R, (n_sys, n_t, N, N)))
    results = []
    for vectors in (True, False):
        engine.dressed_states(systems, grid, rho=rho, want_vectors=vectors)  # warm-up
        k_ms, c_ms = [], []
        while len(k_ms) < 3 or (sum(k_ms) < 300.0 and len(k_ms) < 200):
            t0 = time.perf_counter()
            ev, vec, occ = engine.dressed_states(systems, grid, rho=rho, want_vectors=vectors)
            c_ms.append(1e3 * (time.perf_counter() - t0))
            k_ms.append(engine.dressed_kernel_ms())
        nbytes = n_prob * (16 * N * N + 8 * N + 8 * N + (16 * N * N if vectors else 0))
        kernel_ms = float(np.median(k_ms))
        results.append(dict(shape=name, N=N, n_sys=n_sys, n_t=n_t, problems=n_prob, vectors=vectors,
                            calls=len(k_ms), kernel_ms=round(kernel_ms, 4),
                            kernel_ms_min=round(float(np.min(k_ms)), 4), kernel_ms_max=round(float(np.max(k_ms)), 4),
                            call_ms=round(float(np.median(c_ms)), 3),
                            problems_per_s=round(n_prob / (1e-3 * kernel_ms)), bytes=nbytes,
                            hbm_share=round(nbytes / (1e-3 * kernel_ms) / HBM_PEAK, 4)))
    # host baseline on the same inputs, and a check that the two agree
    n_eigh = min(n_prob, eigh_max)
    idx = np.linspace(0, n_prob - 1, n_eigh).astype(np.int64)
    Hs = host_hamiltonians(systems, n_t, dt, idx)
    rho_s = rho.reshape(-1, N, N)[idx]
    t0 = time.perf_counter()
    w, U = np.linalg.eigh(Hs)
    t_eigh = time.perf_counter() - t0
    t0 = time.perf_counter()
    occ_h = np.einsum("pij,pkj,pik->pj", U, U.conj(), rho_s).real
    t_occ = time.perf_counter() - t0
    err_ev = float(np.max(np.abs(ev.reshape(-1, N)[idx] - w)))
    err_occ = float(np.max(np.abs(occ.reshape(-1, N)[idx] - occ_h)))
    for r in results:
        r.update(eigh_problems=n_eigh, eigh_s=round(t_eigh, 4), eigh_problems_per_s=round(n_eigh / t_eigh),
                 eigh_occ_s=round(t_occ, 4), eigh_full_shape_s=round(t_eigh * n_prob / n_eigh, 3),
                 speedup_kernel_vs_eigh=round((t_eigh * n_prob / n_eigh) / (1e-3 * r["kernel_ms"]), 1),
                 speedup_call_vs_eigh=round((t_eigh * n_prob / n_eigh) / (1e-3 * r["call_ms"]), 2),
                 max_abs_diff_evals=err_ev, max_abs_diff_occ=err_occ)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tls,bx_large,bx_small,six")
    ap.add_argument("--eigh-max", type=int, default=400000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        for r in run_shape(name, a.eigh_max):
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
