"""Bit-for-bit comparison of the small time-local-map kernel (csrc/tlmap.hip, n <= 36) between two libpqd builds.

usage: python scripts/compare_tlmap_builds.py LIB_A LIB_B [--log FILE]

One child process per library (one after the other, the library chosen through PQD_LIB) runs pqd_tl_dynmap_pseudo on
the inputs of cases 1-3 of tests/test_gpu_tlmap_small.py (every case of tests/golden/mp_tlmap_truth.npz as a two-map
chain with its rcond, four graded maps at every n from 1 to 36, the five 120-map semigroup chains) and saves the maps;
the parent compares every array with np.array_equal. Exit status 0: all equal; 1: a difference; 2: a child failed
(the run stops there: nothing more is started on the device)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def _inputs():
    from tests.helpers import tl_graded, tl_semigroup_chain
    from tests.test_gpu_tlmap_small import CHAIN_SEEDS, N_CHAIN, TRUTH
    for name, (A, E, _, rcond) in TRUTH.items():
        yield f"truth_{name}", np.stack([A, E]), rcond
    for n in range(1, 37):
        yield f"size_{n:02d}", tl_graded(np.random.default_rng(4000 + n), n, 4), 1e-12
    for N, seed in CHAIN_SEEDS.items():
        yield f"chain_N{N}", tl_semigroup_chain(N, seed, N_CHAIN)[1], 1e-12


def _child(path):
    from pyaceqd_amd import _lib
    L, ctx = _lib.lib(), _lib.context()
    arrs = {}
    for name, dm, rcond in _inputs():
        dm = np.ascontiguousarray(dm, dtype=np.complex128)
        out = np.empty_like(dm)
        _lib.check(L.pqd_tl_dynmap_pseudo(ctx.handle, _lib.cptr(dm), len(dm), dm.shape[1], rcond, _lib.cptr(out)))
        arrs[name] = out
    np.savez(path, **arrs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--log")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return _child(a.child)
    if len(a.libs) != 2:
        ap.error("two libraries")
    lines, outs = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for k, lib in enumerate(a.libs):
            path = os.path.join(tmp, f"out{k}.npz")
            env = dict(os.environ, PQD_LIB=os.path.abspath(lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "x", "--child", path], env=env, timeout=600)
            if r.returncode != 0:
                print(f"child for {lib} failed with status {r.returncode}")
                return 2
            with np.load(path) as z:
                outs.append({k: z[k] for k in z.files})
    bad = 0
    lines.append(f"A = {os.path.basename(a.libs[0])}\nB = {os.path.basename(a.libs[1])}")
    for name in outs[0]:
        x, y = outs[0][name], outs[1][name]
        same = x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
        bad += not same
        lines.append(f"{name:28s} {str(x.shape):16s} {'equal' if same else 'DIFFERENT'}")
    lines.append(f"{len(outs[0])} outputs, {sum(v.size for v in outs[0].values())} complex numbers, {bad} different")
    text = "\n".join(lines)
    print(text)
    if a.log:
        with open(a.log, "w") as f:
            f.write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
