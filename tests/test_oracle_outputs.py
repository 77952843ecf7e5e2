"""The CPU oracle's output readout with dense operators and many outputs, pinned in higher precision. No GPU.

tests/test_gpu_output_readout.py holds every HIP readout to oracle.propagate with full complex non-Hermitian operators,
a non-Hermitian initial matrix and up to 256 outputs. Here the oracle's own readout is checked at those inputs: the run
with the N^2 operators |a><b| returns the reduced state, rho[b, a](n) = tr(|a><b| rho(n)), and
tr(O rho) = sum_ab O[a, b] rho[b, a] recombined in numpy.clongdouble must reproduce the oracle's dense-operator outputs,
per trajectory and per output column: max_n |dense - recombined| / max_n |recombined[:, k]|.

The two sides share the propagated state bit for bit and differ by one N^2-term sum in double against long double. The
worst column measured 7.8e-16; the bound is 1e-13 (100 x headroom for another libm or compiler, two orders inside the
1e-11 the GPU tests allow a PT sweep).
"""
import numpy as np
import pytest

from oracle import oracle
from tests import helpers as H

N_STEPS = 12


@pytest.mark.parametrize("N,chi,n_out", [(4, 32, 256), (6, 32, 29), (3, None, 65), (2, 16, 9)])
def test_dense_outputs_match_the_recombined_state(N, chi, n_out):
    sysd, grid = H.random_system(N, n_steps=N_STEPS, seed=300 + N)
    tr = H.readout_trajectories(N, N_STEPS, 4, seed=N)
    pt = None if chi is None else H.readout_pt(N, chi, seed=100 * chi + N)
    rho0 = H.dense_state(N, seed=N)
    ops = H.dense_ops(N, n_out, seed=10 + N)
    basis = [H.ketbra(N, a, b) for a in range(N) for b in range(N)]
    dense = oracle.propagate(sysd, grid, rho0, ops, tr, pt=pt)
    state = oracle.propagate(sysd, grid, rho0, basis, tr, pt=pt)
    O = np.array(ops, dtype=np.clongdouble).reshape(n_out, N * N)  # O[k, a N + b]; state[n, a N + b] = rho[b, a](n)
    want = [np.asarray(s, dtype=np.clongdouble) @ O.T for s in state]
    assert want[0].dtype == np.clongdouble and want[0].shape == dense[0].shape
    err, ratio = H.column_errors([np.asarray(d, dtype=np.clongdouble) for d in dense], want)
    print(f"N={N} chi={chi} n_out={n_out}: worst column {float(err.max()):.3e}, smallest column ratio {ratio:.3f}")
    assert err.shape == (tr.n_traj, n_out)
    assert ratio > 0.05
    assert float(err.max()) < 1e-13
