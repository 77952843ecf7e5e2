"""Golden vectors for the dressed-state consumer above dim 6 (tests/golden/pyref_dressed_wide.npz).

Run in the build container only (imports the reference from /root/reference):
    python tests/golden/make_golden_dressed_wide.py

As make_golden_dressed.py, for the cavity models' sizes: the REFERENCE's own `_dressed_states`
(pyaceqd/general_system/general_dressed_states.py:46-183, matplotlib on Agg, plot=False) on seeded synthetic inputs with
n_t = 3, once with the composite dim=[2, 3, 3] (what tls_photons_dressed_states passes, tls.py:207-212) and once with
the plain dim=18 (biexciton_photons_extended_dressed_states, linear.py:157-159). Recorded per case: the returned tuple
for the default colours, for RGBA colours with return_eigenvectors, and for visible_states. Data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_ROOT  # noqa: E402
from make_golden_dressed import record  # noqa: E402

N_T = 3
CASES = {"c233": [2, 3, 3], "p18": 18}
ALPHAS = ["", "80", "FF", "40", "C0", "00", "20", "e0", "10"]


def rgba(plain):
    """the equally spaced colours with a cycle of alpha bytes appended (none, half, opaque, ..., transparent)"""
    return [c + ALPHAS[k % len(ALPHAS)] for k, c in enumerate(plain)]


def inputs(n, rng):
    data = np.zeros((1 + n + n * n, N_T), dtype=complex)
    data[0] = 0.5 * np.arange(N_T)
    rho = np.zeros((N_T, n, n), dtype=complex)
    for k in range(N_T):
        M = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
        w, V = np.linalg.eigh(3.0 * (M + M.conj().T))
        assert np.all(np.abs(V[0]) > 1e-6)
        data[1: 1 + n, k] = w
        data[1 + n:, k] = V.T.reshape(n * n)      # row 1 + n + i n + j = component j of eigenvector i
        B = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
        R = B @ B.conj().T
        rho[k] = R / np.trace(R).real
    return data, rho


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF_ROOT)
    from pyaceqd.general_system import general_dressed_states as G
    rng = np.random.default_rng(20261019)
    arrs = {}
    for key, dim in CASES.items():
        n = int(np.prod(dim))
        data, rho = inputs(n, rng)
        arrs[f"{key}_data"], arrs[f"{key}_rho_in"] = data, rho
        plain = G.select_equally_spaced_colors(n)
        arrs[f"{key}_spaced_colors"] = np.array(plain, dtype="U7")
        record(arrs, f"{key}_plain", G._dressed_states(dim, data, rho, plain, "unused", plot=False))
        record(arrs, f"{key}_rgba", G._dressed_states(dim, data, rho, rgba(plain), "unused", plot=False,
                                                      return_eigenvectors=True))
        record(arrs, f"{key}_visible", G._dressed_states(dim, data, rho, rgba(plain), "unused", plot=False,
                                                         visible_states=[0, 7, n - 1]))
    np.savez_compressed(os.path.join(HERE, "pyref_dressed_wide.npz"), **arrs)
    print("wrote pyref_dressed_wide.npz:", len(arrs), "arrays")


if __name__ == "__main__":
    main()
