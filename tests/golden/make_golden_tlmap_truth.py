"""A multi-precision truth for the time-local maps at map sizes n <= 36 (tests/golden/mp_tlmap_truth.npz).

    python tests/golden/make_golden_tlmap_truth.py

Needs mpmath (1.3.0 when the file was made); no test does. Every case is one step of a chain: A = dm[i-1], E = dm[i],
rcond, and T = E pinv(A, rcond) with numpy's rule (singular values <= rcond * s_max dropped) from mpmath's svd_c of the
double-precision A at 60 digits, rounded to complex128 at the end; the 60-digit singular values are kept as float64.
The inputs come from tests/helpers.py (tl_graded, tl_semigroup_chain), which the GPU tests use as well:

  graded   Haar diag(s) Haar, s log-spaced from 1 to 1 / cond, cond 1e3, 1e6 and 1e9, n in 1, 2, 3, 5, 9, 16, 25, 35, 36
  rank     the same at cond 1e3 with the last five singular values 0, 0, 0, 1e-14, 1e-14, n = 9, 16, 36
  rcond6   the last three singular values 1e-8 and rcond = 1e-6, n = 9, 36
  chain    every 7th map (E = dm[7], dm[14], ...) of the 120-map Lindblad semigroup chains at N = 2, 3, 4, whose
           singular values decay through the cut until one is left

A candidate with a singular value within 1 % of the cut (helpers.tl_near_cut) has no defined answer and is dropped; the
script prints how many were. The file is written with fixed member dates, so it regenerates bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from npz_lzma import savez_lzma  # noqa: E402
from tests.helpers import tl_graded, tl_near_cut, tl_semigroup_chain  # noqa: E402

DPS = 60
SEED = 20261021
CONDS = ((1e3, "1e3"), (1e6, "1e6"), (1e9, "1e9"))
GRADED_N = (1, 2, 3, 5, 9, 16, 25, 35, 36)
CHAIN_SEEDS = {2: 204, 3: 325, 4: 403}   # those of tests/test_gpu_tlmap_small.py
CHAIN_EVERY = 7


def candidates():
    """(name, A, E, rcond) in a fixed order"""
    rng = np.random.default_rng(SEED)
    for cond, tag in CONDS:
        for n in GRADED_N:
            dm = tl_graded(rng, n, 2, cond=cond)
            yield f"graded_c{tag}_n{n}", dm[0], dm[1], 1e-12
    for n in (9, 16, 36):
        dm = tl_graded(rng, n, 2, tail=[0.0, 0.0, 0.0, 1e-14, 1e-14])
        yield f"rank_n{n}", dm[0], dm[1], 1e-12
    for n in (9, 36):
        dm = tl_graded(rng, n, 2, tail=[1e-8] * 3)
        yield f"rcond6_n{n}", dm[0], dm[1], 1e-6
    for N, seed in CHAIN_SEEDS.items():
        _, dm = tl_semigroup_chain(N, seed)
        for i in range(CHAIN_EVERY, len(dm), CHAIN_EVERY):
            yield f"chain_N{N}_i{i:03d}", dm[i - 1], dm[i], 1e-12


def truth(A, E, rcond):
    import mpmath as mp
    mp.mp.dps = DPS
    n = A.shape[0]
    U, S, Vh = mp.svd_c(mp.matrix(A.tolist()))           # A = U diag(S) Vh, S descending
    cut = mp.mpf(rcond) * max(S)
    kept = [j for j in range(n) if S[j] > cut]
    EV = mp.matrix(E.tolist()) * Vh.H                    # E V
    for j in range(n):
        w = 1 / S[j] if j in kept else mp.mpf(0)
        for r in range(n):
            EV[r, j] *= w
    T = EV * U.H
    T = np.array([[complex(T[r, c]) for c in range(n)] for r in range(n)], dtype=np.complex128)
    return T, np.array([float(S[j]) for j in range(n)]), len(kept)


def main():
    arrs, names, dropped = {}, [], []
    for name, A, E, rcond in candidates():
        if tl_near_cut(A, rcond):
            dropped.append(name)
            continue
        T, s, kept = truth(A, E, rcond)
        names.append(name)
        arrs[f"{name}_A"], arrs[f"{name}_E"], arrs[f"{name}_T"] = A, E, T
        arrs[f"{name}_s"], arrs[f"{name}_rcond"] = s, np.float64(rcond)
        print(f"{name}: n = {A.shape[0]}, kept {kept}, s_min / s_max {s[-1] / s[0]:.3e}", flush=True)
    arrs["names"] = np.array(names)
    out = os.path.join(HERE, "mp_tlmap_truth.npz")
    savez_lzma(out, **arrs)
    print(f"wrote {out}: {len(names)} cases, {os.path.getsize(out)} bytes; dropped {len(dropped)} near the cut: {dropped}")


if __name__ == "__main__":
    main()
