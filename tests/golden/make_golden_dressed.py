"""Golden vectors for the dressed-state consumer (tests/golden/pyref_dressed.npz).

Run in the build container only (imports the reference from /root/reference):
    python tests/golden/make_golden_dressed.py

Outputs are the REFERENCE's own `_dressed_states` (pyaceqd/general_system/general_dressed_states.py:46-183, matplotlib
on Agg, plot=False) on seeded synthetic inputs for dim 2, 4 and 6 with n_t = 7: `data` is the (1 + n + n^2, n_t) table
the reference reads from timedep_eigenstates (eigenpairs of a random Hermitian matrix per time, from numpy eigh; the
first components are non-zero, as the reference's phase expression needs), `rho` a random positive matrix of trace 1 per
time. Recorded per dim: every element of the returned tuple (the `s_colors` strings included) for the default colours,
for RGBA colours with return_eigenvectors, for visible_states, and whether the two error paths returned None; and the
two colour helpers.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_ROOT  # noqa: E402

N_T = 7
RGBA = {2: ["#0000FF80", "#FF0000FF"],
        4: ["#0000FF", "#00CC3340", "#F9A627C0", "#FF000000"],
        6: ["#0000cf", "#45b0ee80", "#ff0022", "#9966cc20", "#009e00", "#ffde39e0"]}


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


def record(arrs, key, res):
    names = ("t", "populations", "e_values", "ds_occ", "s_colors", "n_colors", "e_vectors", "rho")
    for name, v in zip(names, res):
        arrs[f"{key}_{name}"] = np.array(v) if name != "s_colors" else np.array(v, dtype="U9")


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF_ROOT)
    from pyaceqd.general_system import general_dressed_states as G
    rng = np.random.default_rng(20260109)
    arrs = {}
    for n in (2, 4, 6):
        data, rho = inputs(n, rng)
        arrs[f"d{n}_data"], arrs[f"d{n}_rho_in"] = data, rho
        plain = G.select_equally_spaced_colors(n)
        arrs[f"d{n}_spaced_colors"] = np.array(plain, dtype="U7")
        record(arrs, f"d{n}_plain", G._dressed_states(n, data, rho, plain, "unused", plot=False))
        record(arrs, f"d{n}_rgba", G._dressed_states(n, data, rho, RGBA[n], "unused", plot=False,
                                                      return_eigenvectors=True))
        record(arrs, f"d{n}_visible", G._dressed_states(n, data, rho, RGBA[n], "unused", plot=False,
                                                         visible_states=[0, n - 1]))
        arrs[f"d{n}_bad_colors_none"] = np.array(G._dressed_states(n, data, rho, plain[:-1], "unused") is None)
        arrs[f"d{n}_bad_visible_none"] = np.array(
            G._dressed_states(n, data, rho, plain, "unused", visible_states=[0, n]) is None)
    codes = ["#0000FF", "00CC33", "#F9A62780", "#ffde39e0", "#000000", "#FFFFFFFF"]
    arrs["hex_codes"] = np.array(codes, dtype="U9")
    arrs["hex_rgba"] = np.array([G.hex_to_rgba(c) for c in codes], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "pyref_dressed.npz"), **arrs)
    print("wrote pyref_dressed.npz:", len(arrs), "arrays")


if __name__ == "__main__":
    main()
