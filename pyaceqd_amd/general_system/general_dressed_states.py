"""Dressed states of the driven system (pyaceqd/general_system/general_dressed_states.py:26-183), on libpqd.

`dressed_states` and `_dressed_states` take the reference's parameters and return its tuple
`t, populations, e_values, ds_occ, s_colors, n_colors[, e_vectors, rho]`. The reference runs a second binary
(`timedep_eigenstates`) for the eigenpairs and loops over times and states in Python; here the eigenpairs come from one
kernel launch (`system(..., dressedstates=True)` -> pqd_dressed_states) and the loops are array expressions.
Plotting is out of scope: `plot`, `t_lim`, `e_lim` and `filename` are accepted and ignored, as in
two_level_system/rabi_rotations.py. `print_states` prints the composition table with plain formatting.

Beyond the reference: `dressed_states(..., trajectories=[{"pulses": ...}, ...])` returns one tuple per drive from two
launches in total: the batched propagation for rho and one dressed-state launch that also evaluates the occupations on
the device.
"""
import colorsys

import numpy as np

from ..tools import basis_states, compose_dm, output_ops_dm

WIDE_MAX_DIM = 24      # pqd_dressed_states_wide, and the propagation without a PT, stop here
_PLAN_MAX_OPS = 256    # output operators one propagation call takes (pqd_host.cpp: "n_out ... not in [1, 256]")


def hex_to_rgba(hex_code):
    """'#RRGGBB' or '#RRGGBBAA' -> (r, g, b, a) in 0..255; alpha 255 when absent"""
    digits = hex_code.lstrip("#")
    if len(digits) == 6:
        digits += "FF"
    v = int(digits, 16)
    return tuple((v >> s) & 255 for s in (24, 16, 8, 0))


def select_equally_spaced_colors(n):
    """n hex colours at equally spaced hues (lightness 0.5, saturation 1)"""
    return ["#{:02X}{:02X}{:02X}".format(*(int(255 * c) for c in colorsys.hls_to_rgb(k / n, 0.5, 1.0)))
            for k in range(n)]


def _split_table(data, n):
    """(1 + n + n^2, n_t) dressed-state table -> t, e_values (n_t, n), e_vectors (n_t, n, n) [time, state, component]"""
    data = np.asarray(data)
    t = data[0].real
    e_values = np.array(data[1: 1 + n].real.T, dtype=float)
    e_vectors = np.array(data[1 + n: 1 + n + n * n].T.reshape(len(t), n, n), dtype=np.complex128)
    return t, e_values, e_vectors


def _print_states(dim, t, e_values, e_vectors, when):
    i = int(np.argmin(np.abs(t - when)))
    head = ["t:{:.2f}".format(t[i])] + basis_states(dim) + ["Energy"]
    rows = [["ds" + str(j + 1)] + ["{:.2f}".format(x) for x in np.abs(e_vectors[i, j]) ** 2]
            + ["{:.2f}".format(e_values[i, j])] for j in range(e_values.shape[1])]
    width = [max(len(r[c]) for r in [head] + rows) for c in range(len(head))]
    for r in [head, ["-" * w for w in width]] + rows:
        print("  ".join(x.rjust(w) for x, w in zip(r, width)))


def _colours(e_vectors, colors, visible_states):
    """per (state, time) colour from the composition |component|^2: '#rrggbbaa' strings and gnuplot's integers"""
    n = e_vectors.shape[1]
    rgba = np.array([hex_to_rgba(c) for c in colors], dtype=float) / 255.0   # (n, 4)
    alpha = np.zeros(n)
    alpha_gp = np.zeros(n)
    if visible_states is None:
        alpha = rgba[:, 3].copy()
        alpha_gp = 1 - rgba[:, 3]
    else:
        alpha[visible_states] = 1
        alpha_gp[visible_states] = 0
    # A channel value is int(clip(dot(channel, |v|^2)) * 255): a truncation, so the last bit of the dot decides at
    # a boundary (an opaque state gives 254 or 255). The weights and the dots are therefore taken per (time, state)
    # row with the calls the reference makes (numpy's array-wide abs and a matrix product round differently in the
    # last place); everything after them is array arithmetic
    chan = [np.ascontiguousarray(c) for c in (rgba[:, 0], rgba[:, 1], rgba[:, 2], alpha, alpha_gp)]
    mixed = np.empty((5,) + e_vectors.shape[:2])
    for i in range(e_vectors.shape[0]):
        for j in range(n):
            e = np.abs(e_vectors[i, j]) ** 2
            mixed[:, i, j] = [np.dot(c, e) for c in chan]
    q = (np.clip(mixed, 0, 1) * 255).astype(np.int64)                        # truncation, as int()
    r, g, b, a, agp = q
    n_colors = (65536 * r + 256 * g + b + agp * 16777216).T.astype(float)     # (state, n_t)
    s_colors = [["#{:02x}{:02x}{:02x}{:02x}".format(r[i, j], g[i, j], b[i, j], a[i, j]) for i in range(q.shape[1])]
                for j in range(n)]
    return s_colors, n_colors


def _occupations(e_vectors, rho):
    """ds_occ[t, j] = Re sum_ik v_j[i] conj(v_j[k]) rho[t, i, k]: the reference's formula, taken literally on the
    array compose_dm returns (which holds <|i><k|>)"""
    return np.einsum("tji,tjk,tik->tj", e_vectors, e_vectors.conj(), rho).real


def _dressed_states(dim, data, rho, colors, filename, plot=False, t_lim=None, e_lim=None, visible_states=None,
                    return_eigenvectors=False, print_states=None, _ds_occ=None):
    """general_dressed_states.py:46-183 without the figures. `data`: the (1 + n + n^2, n_t) table of
    system(..., dressedstates=True); `rho`: (n_t, n, n) from compose_dm. _ds_occ: occupations already evaluated on the
    device for these eigenvectors (the batched form), used in place of the host expression."""
    n = int(np.prod(dim))
    t, e_values, e_vectors = _split_table(data, n)
    # the reference rotates every eigenvector of a time by the phase of e_vectors[t, 0, 0] when its test
    # `np.imag(x != 0 or x < 0)` is truthy; np.imag of that bool is 0, so nothing is ever rotated. The eigenvectors
    # stay as the solver delivered them (libpqd: first component above 1e-12 real and positive)
    if print_states is not None:
        _print_states(dim, t, e_values, e_vectors, print_states)
    if len(colors) != n:
        print("Error: Number of colors does not match number of dressed states.")
        return
    if visible_states is not None and np.max(visible_states) > n - 1:
        print("Error: Visible states out of bounds.")
        return
    s_colors, n_colors = _colours(e_vectors, colors, visible_states)
    ds_occ = _occupations(e_vectors, rho) if _ds_occ is None else np.asarray(_ds_occ, dtype=float)
    populations = np.diagonal(rho, axis1=1, axis2=2)
    if return_eigenvectors:
        return t, populations, e_values, ds_occ, s_colors, n_colors, e_vectors, rho
    return t, populations, e_values, ds_occ, s_colors, n_colors


def dressed_states(system, dim, t_start, t_end, *pulses, plot=True, t_lim=None, e_lim=None, filename="dressed",
                   firstonly=False, colors=None, visible_states=None, return_eigenvectors=False, print_states=None,
                   no_pulse=False, **options):
    """general_dressed_states.py:26-44: propagate for rho (all pulses; firstonly only shapes the diagonalised H), then
    diagonalise H(t) (without the pulses when no_pulse) and compose the reference's tuple.

    With trajectories=[{"pulses": (...)}, ...] (per-drive specs as system_ace_stream takes them): a list of tuples, one
    per spec, from two launches: one batched propagation and one dressed-state launch with the occupations evaluated
    on the device.

    prod(dim) in 7..24 (the cavity and sensor models) takes `_dressed_wide`: the same tuple(s) from the Hilbert-space
    propagation and pqd_dressed_states_wide. Above 24: NotImplementedError."""
    n = int(np.prod(dim))
    if n > WIDE_MAX_DIM:
        raise NotImplementedError(f"dressed states need dim <= {WIDE_MAX_DIM}, this system has dim {n}")
    options["output_ops"] = output_ops_dm(dim)
    if colors is None:
        colors = select_equally_spaced_colors(n=n)
    common = dict(colors=colors, filename=filename, plot=plot, t_lim=t_lim, e_lim=e_lim,
                  visible_states=visible_states, return_eigenvectors=return_eigenvectors, print_states=print_states)
    specs = options.get("trajectories")
    if n > 6:
        return _dressed_wide(system, dim, n, t_start, t_end, pulses, specs, firstonly, no_pulse, options, common)
    if specs is None:
        _, rho = compose_dm(system(t_start, t_end, *pulses, **options), dim=n)
        options["dressedstates"] = True
        options["firstonly"] = firstonly
        data = system(t_start, t_end, *([] if no_pulse else pulses), **options)
        return _dressed_states(dim=dim, data=data, rho=rho, **common)
    return _dressed_batch(system, dim, n, t_start, t_end, pulses, specs, firstonly, no_pulse, options, common)


def _dressed_batch(system, dim, n, t_start, t_end, pulses, specs, firstonly, no_pulse, options, common):
    # launch 1: the batched propagation, one trajectory per spec
    rhos = [compose_dm(r, dim=n)[1] for r in system(t_start, t_end, *pulses, **options)]
    # launch 2: every spec's H(t) diagonalised, the occupations evaluated against its rho on the device
    ds_specs = [dict(s, pulses=()) for s in specs] if no_pulse else specs
    opts = dict(options, trajectories=ds_specs, dressedstates=True, firstonly=firstonly, dressed_rho=rhos)
    runs = system(t_start, t_end, *([] if no_pulse else pulses), **opts)
    return [_dressed_states(dim=dim, data=data, rho=rho, _ds_occ=occ, **common)
            for (data, occ), rho in zip(runs, rhos)]


def _propagate_dm(system, t_start, t_end, pulses, options):
    """the propagation with output_ops_dm's n (n + 1) / 2 operators, in ceil(n (n + 1) / 512) calls on slices of the
    operator list (one up to n = 22, two at 23 and 24), the rows reassembled into one table (per trajectory)"""
    ops = options["output_ops"]
    n_calls = -(-len(ops) // _PLAN_MAX_OPS)
    if n_calls == 1:
        return system(t_start, t_end, *pulses, **options)
    size = -(-len(ops) // n_calls)
    parts = [system(t_start, t_end, *pulses, **dict(options, output_ops=ops[k: k + size]))
             for k in range(0, len(ops), size)]
    if options.get("trajectories") is None:
        return np.concatenate([parts[0]] + [q[1:] for q in parts[1:]])
    return [np.concatenate([qs[0]] + [q[1:] for q in qs[1:]]) for qs in zip(*parts)]


def _dressed_wide(system, dim, n, t_start, t_end, pulses, specs, firstonly, no_pulse, options, common):
    """dim 7..24. `dressedstates=True` stays a dim <= 6 switch (the reference calls it internal to these functions);
    H(t) comes from the model's own lowering instead (lower_only=True: no device, no PT), one System per spec, and
    one dressed-state launch diagonalises all of them and evaluates the occupations against the propagated rho."""
    from .. import _lib, engine
    tables = _propagate_dm(system, t_start, t_end, pulses, options)
    rhos = [compose_dm(r, dim=n)[1] for r in (tables if specs is not None else [tables])]
    opts = dict(options, lower_only=True, firstonly=firstonly)
    if specs is not None and no_pulse:
        opts["trajectories"] = [dict(s, pulses=()) for s in specs]
    low = system(t_start, t_end, *([] if no_pulse else pulses), **opts)
    # one problem set per trajectory, with its density matrices (rows past a shorter trajectory's end stay 0)
    rho_all = np.zeros((len(low.traj_sys), low.grid.n_steps + 1, n, n), dtype=complex)
    for k, r in enumerate(rhos):
        if r.shape != (low.n_t[k], n, n):
            raise ValueError(f"trajectory {k}: rho has shape {r.shape}, expected {(low.n_t[k], n, n)}")
        rho_all[k, :low.n_t[k]] = r
    ev, vec, occ = engine.dressed_states([low.systems[i] for i in low.traj_sys], low.grid, rho=rho_all,
                                         ctx=_lib.context(options.get("device")))
    res = []
    for k, rho in enumerate(rhos):
        m = low.n_t[k]
        tab = engine.dressed_table(low.grid.times[:m], ev[k][:m], vec[k][:m])
        res.append(_dressed_states(dim=dim, data=tab, rho=rho, _ds_occ=occ[k][:m], **common))
    return res if specs is not None else res[0]
