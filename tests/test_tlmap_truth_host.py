"""The references of the small time-local-map kernel (csrc/tlmap.hip) against a multi-precision truth, on the CPU.

tests/golden/mp_tlmap_truth.npz (make_golden_tlmap_truth.py) holds, per case, A = dm[i-1], E = dm[i], rcond and
T = E pinv(A, rcond) from a 60-digit SVD of the same double-precision inputs. Errors are max|X - T| / max|T| in units of
    u = eps (|T|_2 |A|_2 + |E|_2) / s_min_kept / max|T|          (helpers.tl_unit),
the first-order change of T under eps-sized backward errors in A and E. Checked here, for every case:
  * numpy's pinv, the reference of the GPU tests where there is no truth, is within 2 u of the truth;
  * oracle.tl_dynmap_pseudo is that expression;
  * helpers.tl_jacobi_restated, the kernel's algorithm in numpy, is within 2 u as well, so the method, as opposed to
    its HIP text, meets the bound the GPU tests hold the kernel to (4 u), and its sweep counts are the expected ones.

Agreement of two LAPACK routes (gesdd, gesvd) is not used as evidence of accuracy: both go through the same
bidiagonalisation, agree with each other to 6e-15 at every condition number and are eps * cond from the truth together.
"""
import os

import numpy as np
import pytest

from oracle import oracle
from tests.helpers import EPS, tl_graded, tl_jacobi_restated, tl_kept, tl_near_cut, tl_rel, tl_rr_pairs, tl_unit


@pytest.fixture(scope="module")
def cases(golden_dir):
    with np.load(os.path.join(golden_dir, "mp_tlmap_truth.npz"), allow_pickle=False) as z:
        return [(str(k), z[f"{k}_A"], z[f"{k}_E"], z[f"{k}_T"], z[f"{k}_s"], float(z[f"{k}_rcond"]))
                for k in z["names"]]


def test_fixture_covers_what_it_should(cases):
    names = [c[0] for c in cases]
    assert len(names) == len(set(names)) >= 60
    for tag in ("1e3", "1e6", "1e9"):
        for n in (1, 2, 3, 5, 9, 16, 25, 35, 36):
            assert f"graded_c{tag}_n{n}" in names
    for k in ("rank_n9", "rank_n16", "rank_n36", "rcond6_n9", "rcond6_n36"):
        assert k in names
    for N in (2, 3, 4):
        kept = [tl_kept(A, rc)[1] for k, A, E, T, s, rc in cases if k.startswith(f"chain_N{N}_")]
        assert len(kept) >= 15 and kept[0] == N * N and kept[-1] == 1    # the whole crossing, down to rank 1
        assert all(a >= b for a, b in zip(kept, kept[1:]))
    for k, A, E, T, s, rc in cases:
        assert A.shape == E.shape == T.shape == (len(s), len(s)) and len(s) <= 36
        assert not tl_near_cut(A, rc), k
        # the stored 60-digit singular values: descending, and numpy's are within a few eps s_max of them
        assert np.all(np.diff(s) <= 0)
        assert np.max(np.abs(tl_kept(A, rc)[0] - s)) <= 8 * EPS * s[0], k
        assert tl_kept(A, rc)[1] == int(np.count_nonzero(s > rc * s[0])), k


def test_numpy_pinv_is_within_2u_of_the_truth_and_is_the_oracle(cases):
    worst = (0.0, "")
    for k, A, E, T, s, rc in cases:
        ref = E @ np.linalg.pinv(A, rcond=rc)
        assert np.array_equal(oracle.tl_dynmap_pseudo(np.stack([A, E]), rcond=rc)[1], ref), k
        r = tl_rel(ref, T) / tl_unit(A, E, T, rc)
        worst = max(worst, (r, k))
        assert r <= 2.0, (k, r)
    print(f"numpy pinv vs truth: worst {worst[0]:.2f} u at {worst[1]}")


def test_restated_jacobi_is_within_2u_of_the_truth(cases):
    worst, most = (0.0, ""), (0, "")
    for k, A, E, T, s, rc in cases:
        out, sweeps = tl_jacobi_restated(np.stack([A, E]), rc)
        assert np.array_equal(out[0], A)
        r = tl_rel(out[1], T) / tl_unit(A, E, T, rc)
        worst, most = max(worst, (r, k)), max(most, (int(sweeps[1]), k))
        assert r <= 2.0, (k, r)
        assert 1 <= sweeps[1] <= 30, (k, sweeps)
    print(f"restated Jacobi vs truth: worst {worst[0]:.2f} u at {worst[1]}; most sweeps {most[0]} at {most[1]}")


def test_unit_and_band_helpers():
    # n = 1: T = E / A, u = 2 eps whatever the values
    A, E = np.array([[0.3 - 0.4j]]), np.array([[2.0 + 1.0j]])
    assert tl_unit(A, E, E / A, 1e-12) == pytest.approx(2 * EPS, rel=1e-12)
    # a diagonal map: the unit scales with 1 / s_min_kept, and a dropped value does not count
    A = np.diag([1.0, 1e-3, 1e-14]).astype(complex)
    T = np.diag([1.0, 1e3, 0.0]).astype(complex)
    assert tl_unit(A, np.eye(3, dtype=complex), T, 1e-12) == pytest.approx(EPS * (1e3 + 1.0) / 1e-3 / 1e3, rel=1e-12)
    with pytest.raises(ValueError):
        tl_unit(np.zeros((2, 2), dtype=complex), A[:2, :2], np.zeros((2, 2)), 1e-12)
    for s3, near in ((1.005e-12, True), (0.995e-12, True), (1.02e-12, False), (0.98e-12, False), (0.0, False)):
        assert tl_near_cut(np.diag([1.0, 0.5, s3]).astype(complex), 1e-12) is near, s3
    assert tl_near_cut(np.diag([1.0, 0.0]).astype(complex), 0.0) is False
    assert tl_near_cut(np.diag([1.0, 1.0]).astype(complex), 1.0) is True


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 35, 36])
def test_tournament_meets_every_pair_once(n):
    rounds = tl_rr_pairs(n)
    assert len(rounds) == n + (n & 1) - 1
    seen = []
    for ps, qs in rounds:
        cols = list(ps) + list(qs)
        assert len(cols) == len(set(cols)) and len(ps) == n // 2    # disjoint pairs; odd n: one column sits out
        assert all(0 <= p < q < n for p, q in zip(ps, qs))
        seen += list(zip(ps, qs))
    assert len(seen) == len(set(seen)) == n * (n - 1) // 2


def test_restated_jacobi_reports_a_sweep_limit_and_skips_nan():
    dm = tl_graded(np.random.default_rng(5), 16, 3)
    full, sweeps = tl_jacobi_restated(dm, 1e-12)
    assert sweeps[0] == 0 and np.all(sweeps[1:] > 4)
    cut, few = tl_jacobi_restated(dm, 1e-12, max_sweeps=4)
    assert list(few) == [0, 4, 4] and tl_rel(cut, full) > 1e-9      # not converged: a different result
    bad = dm.copy()
    bad[1, 3, 5] = np.nan
    out, sweeps = tl_jacobi_restated(bad, 1e-12)
    assert np.array_equal(out[0], full[0]) and np.all(sweeps[1:] <= 30)
    assert not np.all(np.isfinite(out[1])) and not np.all(np.isfinite(out[2]))
