"""Bit-for-bit comparison of the PT generator's factorizations between two libpqd builds.

usage: python scripts/compare_ptgen_builds.py LIB_A LIB_B [--only SUBSTRING[,SUBSTRING...]] [--log FILE]

For every case one child process per library (one after the other, the library chosen through PQD_LIB, the case's
PQD_PTG_* switches in its environment) computes the outputs from seeded inputs (built like tests/test_gpu_ptgen.py's
_rand; nothing depends on the process id or the time) and saves them; the parent compares every array with
np.array_equal: Q, R, perm and rank of a QR, X, V, sigma and sweeps of a Jacobi SVD, every tensor of the builder's
tail after six steps of the generator. The cases are chosen so that every kernel instance of csrc/ptgen.hip runs at
least once (the instance each one is there for is named in its id). Exit status 0: all equal; 1: a difference;
2: a child failed (the run stops there: nothing more is started on the device)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

PTG_VARS = ("SMALL", "WG", "BLOCKED", "QPERSIST", "PAIR", "QFB", "DIAG", "QSPIN", "JPERSIST", "JBLOCK", "JSPIN")


def _rand(rng, m, n, rank=None, scale=None):
    A = rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n))
    if rank is not None:
        A = (rng.normal(size=(m, rank)) + 1j * rng.normal(size=(m, rank))) @ (
            rng.normal(size=(rank, n)) + 1j * rng.normal(size=(rank, n)))
        A += 1e-14 * (rng.normal(size=(m, n)) + 1j * rng.normal(size=(m, n)))
    if scale is not None:
        A = A * scale[None, :]
    return A


def _cases():
    """id -> (kind, parameters, switches)"""
    c = {}

    def qr(tag, m, n, env, piv=None, rank=None):
        # piv: None plain, "abs": tolerance 1e-10 x the largest column norm, "rel": relative 1e-10 found on the device
        sw = ",".join(f"{k}={v}" for k, v in env.items())
        c[f"qr_{m}x{n}_{piv or 'plain'}_{sw}_{tag}"] = ("qr", dict(m=m, n=n, piv=piv, rank=rank), env)

    for m, n, qe in [(7, 5, 1), (5, 7, 1), (40, 30, 1), (100, 80, 2), (195, 39, 4), (300, 20, 8), (600, 13, 0)]:
        qr(f"small{qe}", m, n, {"SMALL": 1})
        qr(f"small{qe}", m, n, {"SMALL": 1}, piv="abs")
    for tag, env in [("step2_wg2", {"WG": 1}), ("step_wg2", {"WG": 1, "PAIR": 0}), ("step2_wave", {"WG": 0}),
                     ("step_wave", {"WG": 0, "PAIR": 0}), ("blocked", {"BLOCKED": 1}), ("qf_apply", {"QFB": 0})]:
        qr(tag, 300, 120, dict(SMALL=0, **env))
    qr("step2_wg4", 640, 273, {"SMALL": 0})
    qr("step2_wg8", 1205, 300, {"SMALL": 0})
    qr("step2_wg16", 3000, 200, {"SMALL": 0})
    qr("step2_wg2", 257, 64, {"SMALL": 0})
    qr("step2_wg1", 150, 150, {"SMALL": 0})
    pivoted = [("wg8", 1205, 300, "abs", 120), ("wg16", 3000, 200, "rel", None), ("wg4", 640, 273, "abs", None),
               ("wg2", 257, 64, "abs", 30), ("wg1", 150, 150, "abs", None)]
    for tag, m, n, piv, rank in pivoted:
        qr("step_" + tag, m, n, {"SMALL": 0, "WG": 1}, piv=piv, rank=rank)
        qr("persist_" + tag, m, n, {"SMALL": 0, "QPERSIST": 1}, piv=piv, rank=rank)
    qr("step_wave", 1205, 300, {"SMALL": 0, "WG": 0}, piv="abs", rank=120)
    for m, n in [(257, 64), (400, 250)]:
        qr("persist_plain", m, n, {"SMALL": 0, "QPERSIST": 2, "PAIR": 0, "BLOCKED": 0})

    def jac(tag, n, env):
        sw = ",".join(f"{k}={v}" for k, v in env.items())
        c[f"jacobi_{n}_{sw}_{tag}"] = ("jacobi", dict(n=n), env)

    jac("small", 9, {"SMALL": 1})
    jac("small", 40, {"SMALL": 1})
    for n, epl in [(9, 1), (91, 2), (130, 4), (300, 8), (600, 16)]:
        jac(f"block{epl}" if epl <= 8 else "persist16", n, {"SMALL": 0})
        jac(f"persist{epl}", n, {"SMALL": 0, "JBLOCK": 0})
    jac("rounds", 91, {"SMALL": 0, "JPERSIST": 0})
    c["generator_tls_6_steps"] = ("gen", {}, {})
    return c


def _child(case, out):
    kind, p, _ = _cases()[case]
    import torch
    from pyaceqd_amd import ptgen, ptgen_gpu

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.complex128, device="cuda")

    res = {}
    if kind == "qr":
        m, n = p["m"], p["n"]
        rng = np.random.default_rng(m * 1000 + n)
        if p["piv"] is None:
            W = _rand(rng, m, n)
            Qc, Rc, perm, k = ptgen_gpu.qr_cols(dev(W.T))
        else:
            W = _rand(rng, m, n, rank=p["rank"], scale=None if p["rank"] else np.logspace(0, -14, n))
            tol = -1e-10 if p["piv"] == "rel" else 1e-10 * np.max(np.linalg.norm(W, axis=0))
            Qc, Rc, perm, k = ptgen_gpu.qr_cols(dev(W.T), pivot=True, tol=tol, unperm=p["piv"] == "rel")
        res = dict(Q=Qc.cpu().numpy(), R=Rc.cpu().numpy(), perm=perm.cpu().numpy(), rank=np.array(k))
    elif kind == "jacobi":
        n = p["n"]
        X = _rand(np.random.default_rng(7 * n + 1), n, n)
        Xo, V, sig = ptgen_gpu.jacobi_cols(dev(X.T))
        res = dict(X=Xo.cpu().numpy(), V=V.cpu().numpy(), sigma=sig.cpu().numpy(),
                   sweeps=np.array(ptgen_gpu.LAST_SWEEPS))
    else:  # the tls case of scripts/bench_ptgen.py
        dt, t_mem = 0.1, 6.4
        K = int(round(t_mem / dt))
        eta, delta = ptgen.eta_coefficients(lambda w: ptgen.qd_phonon_J(w, ae=5.0), 4.0, dt, K)
        b = ptgen_gpu.GaussianPTBuilderGPU(np.diag([0.0, 1.0]), eta, delta, dt, 1e-8, 128, tail="qrcp")
        for _ in range(6):
            b.step()
        res = {f"tail{i:03d}": x.cpu().numpy() for i, x in enumerate(b.tail)}
        res["n_tail"] = np.array(len(b.tail))
    torch.cuda.synchronize()
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--only", default="")
    ap.add_argument("--log", default="")
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

    say(f"# A = {a.libs[0]}  B = {a.libs[1]}; one child process per case and library; np.array_equal on every output")
    n_diff = 0
    cases = {k: v for k, v in _cases().items() if any(t in k for t in a.only.split(","))}
    with tempfile.TemporaryDirectory() as tmp:
        for cid, (_, _, sw) in cases.items():
            got = []
            for i, lib in enumerate(libs):
                env = {k: v for k, v in os.environ.items() if not k.startswith("PQD_PTG_")}
                env["PQD_LIB"] = lib
                env.update({f"PQD_PTG_{k}": str(v) for k, v in sw.items()})
                assert all(k in PTG_VARS for k in sw)
                out = os.path.join(tmp, f"{i}.npz")
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cid, "--out", out],
                                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
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
            shapes = " ".join(f"{k}{tuple(A[k].shape)}" for k in sorted(A) if not k.startswith("tail")) or f"{len(A)} arrays"
            say(f"{'DIFFER ' + ','.join(bad) if bad else 'equal '} {cid}  [{shapes}]")
    say(f"# {len(cases)} cases, {n_diff} differ")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
