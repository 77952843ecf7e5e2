"""Four-level biexciton cascade G/X/Y/B (pyaceqd/four_level_system/linear.py:8-39), on libpqd.

|0> = G, |1> = X, |2> = Y, |3> = B. Same signature, defaults and operator strings as the
reference `biexciton`: binding energy delta_b on |3><3|, fine-structure splitting delta_xy,
x/y-polarised ladder couplings, boson operator 1*(|1><1|+|2><2|) + 2*|3><3|, four decay channels.

Below it the cavity and sensor variants biexciton_photons, biexciton_photons_extended and biexciton_sensors
(linear.py:45-206), dim 16 and 18: they propagate without phonons only (general_system.system_ace_stream).
"""
from ..general_system.general_system import system_ace_stream
from .. import constants

hbar = constants.hbar
temp_dir = constants.temp_dir

_FWD = ("trajectories", "n_sub", "device", "rho0", "get_M_t", "pulse_sampling", "trapz", "dressed_rho",
        "lower_only", "wide_pt", "wide_maps", "calc_dynmap")


def biexciton_ops(delta_xy=0, shift_x=True, coupl_xy=0, delta_b=4, gamma_e=1/100, gamma_b=None, lindblad=False,
                  rf=False):
    """The strings the reference writes for this model (four_level_system/linear.py:13-33)."""
    if shift_x:
        system_op = ["{}*|3><3|_4".format(-delta_b), "{}*|1><1|_4".format(-delta_xy / 2),
                     "{}*|2><2|_4".format(delta_xy / 2)]
    else:
        system_op = ["{}*|3><3|_4".format(-delta_b), "{}*|2><2|_4".format(delta_xy)]
    boson_op = "1*(|1><1|_4 + |2><2|_4) + 2*|3><3|_4"
    lindblad_ops = []
    if lindblad:
        gb = gamma_e if gamma_b is None else gamma_b
        lindblad_ops = [["|0><1|_4", gamma_e], ["|0><2|_4", gamma_e], ["|1><3|_4", gb], ["|2><3|_4", gb]]
    interaction_ops = [["|1><0|_4+|3><1|_4", "x"], ["|2><0|_4+|3><2|_4", "y"]]
    if coupl_xy != 0:
        system_op += ["{}*|1><2|_4".format(coupl_xy), "{}*|2><1|_4".format(coupl_xy)]
    rf_op = "|1><1|_4 + |2><2|_4 + 2*|3><3|_4" if rf else None
    return system_op, boson_op, lindblad_ops, interaction_ops, rf_op


def biexciton(t_start, t_end, *pulses, dt=0.5, delta_xy=0, shift_x=True, coupl_xy=0, delta_b=4, gamma_e=1/100,
              gamma_b=None, phonons=False, ae=3.0, temperature=4, verbose=False, lindblad=False, temp_dir=temp_dir,
              pt_file=None, suffix="", multitime_op=None, pulse_file_x=None, pulse_file_y=None, prepare_only=False,
              output_ops=["|0><0|_4", "|1><1|_4", "|2><2|_4", "|3><3|_4"], initial="|0><0|_4", t_mem=20.48,
              dressedstates=False, rf=False, rf_file=None, firstonly=False, use_infinite=False, calc_dynmap=False,
              **options):
    system_op, boson_op, lindblad_ops, interaction_ops, rf_op = biexciton_ops(
        delta_xy, shift_x, coupl_xy, delta_b, gamma_e, gamma_b, lindblad, rf)
    fwd = {k: options[k] for k in _FWD if k in options}
    return system_ace_stream(
        t_start, t_end, *pulses, dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature,
        verbose=verbose, temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
        system_prefix="b_linear", threshold="10", threshold_ratio="0.3", buffer_blocksize="-1", dict_zero="16",
        precision="12", boson_e_max=7, system_op=system_op, pulse_file_x=pulse_file_x, pulse_file_y=pulse_file_y,
        boson_op=boson_op, initial=initial, lindblad_ops=lindblad_ops, interaction_ops=interaction_ops,
        output_ops=output_ops, prepare_only=prepare_only, dressedstates=dressedstates, rf_op=rf_op, rf_file=rf_file,
        firstonly=firstonly, use_infinite=use_infinite, calc_dynmap=calc_dynmap, **fwd)


# ---------------------------------------------------------------------------------------------------------------
# Biexciton with cavity modes or sensors (pyaceqd/four_level_system/linear.py:45-206): dim 16 or 18, so only the
# propagation without phonons exists for them (general_system.system_ace_stream). Same operator content, rates and
# order as the reference's param lines (tests/test_params_cavity_golden.py).
# ---------------------------------------------------------------------------------------------------------------
def _qd(op, d1, d2):
    """a quantum-dot operator on the first factor of the 4 x d1 x d2 product space"""
    return "{} otimes Id_{} otimes Id_{}".format(op, d1, d2)


def _run_biexciton(prefix, ops, t_start, t_end, pulses, options, **kw):
    system_op, boson_op, lindblad_ops, interaction_ops, rf_op = ops
    fwd = {k: options[k] for k in _FWD if k in options}
    return system_ace_stream(
        t_start, t_end, *pulses, system_prefix=prefix, threshold="10", threshold_ratio="0.3", buffer_blocksize="-1",
        dict_zero="16", precision="12", boson_e_max=7, system_op=system_op, boson_op=boson_op,
        lindblad_ops=lindblad_ops, interaction_ops=interaction_ops, rf_op=rf_op, **kw, **fwd)


def biexciton_photons(t_start, t_end, *pulses, dt=0.5, delta_xy=0, delta_b=4, gamma_e=1/100, cav_coupl=0.06,
                      cav_loss=0.12/hbar, delta_cx=-2, gamma_b=None, phonons=False, ae=3.0, temperature=4,
                      verbose=False, lindblad=False, temp_dir=temp_dir, pt_file=None, suffix="", multitime_op=None,
                      pulse_file_x=None, pulse_file_y=None, prepare_only=False, output_ops=None, initial=None,
                      t_mem=20.48, dressedstates=False, rf=False, rf_file=None, firstonly=False, n_phot1=1, n_phot2=1,
                      **options):
    """Biexciton in an x- and a y-polarised cavity mode (dim 4 (n_phot1 + 1) (n_phot2 + 1), 16 by default;
    linear.py:45-103): the x mode couples G-X and X-B, the y mode G-Y and Y-B."""
    n1, n2 = n_phot1 + 1, n_phot2 + 1
    if initial is None:
        initial = "|0><0|_4 otimes |0><0|_{} otimes |0><0|_{}".format(n1, n2)
    if output_ops is None:
        output_ops = [_qd("|{0}><{0}|_4".format(k), n1, n2) for k in range(4)]
    if rf and pulse_file_x is not None and rf_file is None:
        print("Error: pulse file is given, but no file for rotating frame")
        return 0
    ops = biexciton_photons_ops(n1, n2, delta_xy, delta_b, gamma_e, gamma_b, cav_coupl, cav_loss, delta_cx, lindblad, rf)
    return _run_biexciton("b_linear_cavity", ops, t_start, t_end, pulses, options, dt=dt, phonons=phonons, t_mem=t_mem,
                          ae=ae, temperature=temperature, verbose=verbose, temp_dir=temp_dir, pt_file=pt_file,
                          suffix=suffix, multitime_op=multitime_op, pulse_file_x=pulse_file_x,
                          pulse_file_y=pulse_file_y, initial=initial, output_ops=output_ops,
                          prepare_only=prepare_only, dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly)


def biexciton_photons_ops(n1, n2, delta_xy=0, delta_b=4, gamma_e=1/100, gamma_b=None, cav_coupl=0.06,
                          cav_loss=0.12/hbar, delta_cx=-2, lindblad=False, rf=False):
    """The strings the reference writes for biexciton_photons with n1 and n2 levels in the x and y mode
    (four_level_system/linear.py:58-94): system_op, boson_op, lindblad_ops, interaction_ops, rf_op."""
    q = lambda op: _qd(op, n1, n2)  # noqa: E731
    system_op = [q("-{}*|3><3|_4".format(delta_b)), q("-{}*|1><1|_4".format(delta_xy / 2)),
                 q("{}*|2><2|_4".format(delta_xy / 2))]
    boson_op = " + ".join([q("|1><1|_4"), q("|2><2|_4"), q("2*|3><3|_4")])
    lindblad_ops = []
    if lindblad:
        gb = gamma_e if gamma_b is None else gamma_b
        lindblad_ops = [[q("|0><1|_4"), gamma_e], [q("|0><2|_4"), gamma_e], [q("|1><3|_4"), gb], [q("|2><3|_4"), gb]]
    interaction_ops = [[q("|1><0|_4") + " +" + q("|3><1|_4") + " ", "x"], [q("|2><0|_4") + " +" + q("|3><2|_4") + " ", "y"]]
    mode_x = lambda dot, op: "{} otimes {}_{} otimes Id_{}".format(dot, op, n1, n2)  # noqa: E731
    mode_y = lambda dot, op: "{} otimes Id_{} otimes {}_{}".format(dot, n1, op, n2)  # noqa: E731
    lindblad_ops += [[mode_x("Id_4", "b"), cav_loss], [mode_y("Id_4", "b"), cav_loss]]
    system_op += [" {} * ({})".format(delta_cx, mode_x("Id_4", "n")), " {} * ({})".format(delta_cx, mode_y("Id_4", "n"))]
    for mode, lo, hi in ((mode_x, 0, 1), (mode_x, 1, 3), (mode_y, 0, 2), (mode_y, 2, 3)):  # the dot transitions a mode drives
        system_op.append("{} * ({} + {})".format(cav_coupl, mode("|{}><{}|_4".format(hi, lo), "b"),
                                                 mode("|{}><{}|_4".format(lo, hi), "bdagger")))
    rf_op = " + ".join([q("|1><1|_4"), mode_x("Id_4", "n"), mode_y("Id_4", "n")]) if rf else None
    return system_op, boson_op, lindblad_ops, interaction_ops, rf_op


# biexciton_photons_extended: the 18 states with at most two excitations in the cavity modes of a dot state,
# |dot, n_x, n_y>: G with (0,0) (1,0) (0,1) (1,1) (2,0) (0,2) = 0..5, then X, Y, B with (0,0) (1,0) (0,1) (1,1) each
_EXT_PHOT = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2)]
_EXT = {(d, ph): (k if d == 0 else 6 + 4 * (d - 1) + k)
        for d in range(4) for k, ph in enumerate(_EXT_PHOT[:6 if d == 0 else 4])}


def _ext_sum(terms):
    """sum of f |a><b|_18 strings from (a, b, squared factor) triples, ordered by (a, b)"""
    fmt = lambda a, b, f2: ("|{}><{}|_18" if f2 == 1 else "sqrt({2})*|{0}><{1}|_18").format(a, b, f2)  # noqa: E731
    return " + ".join(fmt(*t) for t in sorted(terms))


def _ext_dot(lo, hi):
    """|lo><hi| on the dot for every photon configuration both dot states have"""
    return [(_EXT[(lo, ph)], _EXT[(hi, ph)], 1) for ph in _EXT_PHOT if (lo, ph) in _EXT and (hi, ph) in _EXT]


def _ext_mode(mode):
    """annihilator of cavity mode 0 (x) or 1 (y): sqrt(n) |.., n - 1><.., n|"""
    out = []
    for (d, ph), k in _EXT.items():
        if ph[mode] > 0:
            lower = tuple(n - (1 if m == mode else 0) for m, n in enumerate(ph))
            if (d, lower) in _EXT:
                out.append((_EXT[(d, lower)], k, ph[mode]))
    return out


def _ext_coupling(mode, pairs):
    """dot lowering hi -> lo with a photon created in `mode`, where the state exists, plus the adjoint"""
    out = []
    for lo, hi in pairs:
        for ph in _EXT_PHOT:
            more = tuple(n + (1 if m == mode else 0) for m, n in enumerate(ph))
            if (hi, ph) in _EXT and (lo, more) in _EXT:
                a, b = _EXT[(lo, more)], _EXT[(hi, ph)]
                out += [(a, b, more[mode]), (b, a, more[mode])]
    return out


def biexciton_photons_extended(
        t_start, t_end, *pulses, dt=0.5, delta_xy=0, delta_b=4, gamma_e=1/100, cav_coupl=0.06, cav_loss=0.12/hbar,
        delta_cx=-2, gamma_b=None, phonons=False, ae=3.0, temperature=4, verbose=False, lindblad=False,
        temp_dir=temp_dir, pt_file=None, suffix="", multitime_op=None, pulse_file_x=None, pulse_file_y=None,
        prepare_only=False,
        output_ops=["|0><0|_18 + |1><1|_18 + |2><2|_18 + |3><3|_18 + |4><4|_18 + |5><5|_18",
                    "|6><6|_18 + |7><7|_18 + |8><8|_18 + |9><9|_18",
                    "|10><10|_18 + |11><11|_18 + |12><12|_18 + |13><13|_18",
                    "|14><14|_18 + |15><15|_18 + |16><16|_18 + |17><17|_18"],
        initial="|0><0|_18", t_mem=20.48, dressedstates=False, rf=False, rf_file=None, firstonly=False, **options):
    """Biexciton in two cavity modes on the 18 states with at most two cavity excitations (|G,2,0> and |G,0,2>
    included; linear.py:111-155)."""
    dot_e = [0.0, -delta_xy / 2, delta_xy / 2, -delta_b]
    system_op = []
    for (d, ph), k in sorted(_EXT.items(), key=lambda it: it[1]):
        if k > 0:
            system_op.append("{}*|{}><{}|_18".format(dot_e[d] + sum(ph) * delta_cx, k, k))
    boson_op = " + ".join("{}*|{}><{}|_18".format(2 if d == 3 else 1, k, k) for (d, _), k in _EXT.items() if d > 0)
    lindblad_ops = []
    if lindblad:
        gb = gamma_e if gamma_b is None else gamma_b
        lindblad_ops = [[_ext_sum(_ext_dot(0, 1)), gamma_e], [_ext_sum(_ext_dot(0, 2)), gamma_e],
                        [_ext_sum(_ext_dot(1, 3)), gb], [_ext_sum(_ext_dot(2, 3)), gb]]
    flip = lambda terms: [(b, a, f) for a, b, f in terms]  # noqa: E731
    interaction_ops = [[_ext_sum(flip(_ext_dot(0, 1)) + flip(_ext_dot(1, 3))), "x"],
                       [_ext_sum(flip(_ext_dot(0, 2)) + flip(_ext_dot(2, 3))), "y"]]
    lindblad_ops += [[_ext_sum(_ext_mode(0)), cav_loss], [_ext_sum(_ext_mode(1)), cav_loss]]
    system_op.append("{} * ( {})".format(cav_coupl, _ext_sum(_ext_coupling(0, [(0, 1), (1, 3)]))))
    system_op.append("{} * ( {})".format(cav_coupl, _ext_sum(_ext_coupling(1, [(0, 2), (2, 3)]))))
    rf_op = None
    if rf:  # the number of excitations (dot and photons) of each state
        rf_op = " + ".join("{}*|{}><{}|_18".format((0, 1, 1, 2)[d] + sum(ph), k, k) for (d, ph), k in _EXT.items() if k)
    return _run_biexciton("b_linear_cavity_extended", (system_op, boson_op, lindblad_ops, interaction_ops, rf_op),
                          t_start, t_end, pulses, options, dt=dt, phonons=phonons, t_mem=t_mem, ae=ae,
                          temperature=temperature, verbose=verbose, temp_dir=temp_dir, pt_file=pt_file, suffix=suffix,
                          multitime_op=multitime_op, pulse_file_x=pulse_file_x, pulse_file_y=pulse_file_y,
                          initial=initial, output_ops=output_ops, prepare_only=prepare_only,
                          dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly)


def biexciton_sensors(t_start, t_end, *pulses, dt=0.1, delta_xy=0, shift_x=True, delta_s1=0, delta_s2=0,
                      epsilon=0.0001, linewidth1=0.01, linewidth2=None, delta_b=4, gamma_e=1/100, gamma_b=None,
                      phonons=False, ae=3.0, temperature=4, verbose=False, lindblad=False, temp_dir=temp_dir,
                      pt_file=None, suffix="", multitime_op=None, pulse_file_x=None, pulse_file_y=None,
                      prepare_only=False,
                      output_ops=["|0><0|_4 otimes Id_2 otimes Id_2", "|1><1|_4 otimes Id_2 otimes Id_2",
                                  "|2><2|_4 otimes Id_2 otimes Id_2", "|3><3|_4 otimes Id_2 otimes Id_2"],
                      initial="|0><0|_4 otimes |0><0|_2 otimes |0><0|_2", t_mem=12.8, dressedstates=False, rf=False,
                      rf_file=None, firstonly=False, **options):
    """Biexciton read out by two sensors (dim 16; linear.py:161-206): sensor 1 reads the y transitions (G-Y, Y-B),
    sensor 2 the x transitions (G-X, X-B)."""
    q = lambda op: _qd(op, 2, 2)  # noqa: E731
    bare, boson_bare, lind_bare, inter_bare, rf_bare = biexciton_ops(delta_xy, shift_x, 0, delta_b, gamma_e, gamma_b,
                                                                     lindblad, rf)
    system_op = [q(s) for s in bare]
    boson_op = "1*({} + {}) + 2*({}) ".format(q("|1><1|_4"), q("|2><2|_4"), q("|3><3|_4"))
    lindblad_ops = [[q(o), r] for o, r in lind_bare]
    interaction_ops = [[" +".join(q(t) for t in o.split("+")), pol] for o, pol in inter_bare]
    rf_op = "{} + {} + 2*({})".format(q("|1><1|_4"), q("|2><2|_4"), q("|3><3|_4")) if rf else None
    s1 = lambda dot, sen: "{} otimes {} otimes Id_2".format(dot, sen)  # noqa: E731
    s2 = lambda dot, sen: "{} otimes Id_2 otimes {}".format(dot, sen)  # noqa: E731
    system_op += ["{} * ({})".format(delta_s1, s1("Id_4", "|1><1|_2")), "{} * ({})".format(delta_s2, s2("Id_4", "|1><1|_2"))]
    for site, lo, hi in ((s1, 0, 2), (s1, 2, 3), (s2, 0, 1), (s2, 1, 3)):
        system_op.append("{} * ({} + {})".format(epsilon, site("|{}><{}|_4".format(hi, lo), "|0><1|_2"),
                                                 site("|{}><{}|_4".format(lo, hi), "|1><0|_2")))
    lindblad_ops += [[s1("Id_4", "|0><1|_2"), linewidth1],
                     [s2("Id_4", "|0><1|_2"), linewidth1 if linewidth2 is None else linewidth2]]
    return _run_biexciton("b_linear_sensor", (system_op, boson_op, lindblad_ops, interaction_ops, rf_op), t_start,
                          t_end, pulses, options, dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature,
                          verbose=verbose, temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
                          pulse_file_x=pulse_file_x, pulse_file_y=pulse_file_y, initial=initial, output_ops=output_ops,
                          prepare_only=prepare_only, dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly)


def biexciton_dressed_states(t_start, t_end, *pulses, plot=True, t_lim=None, e_lim=None,
                             colors=["#0000FF", "#00CC33", "#F9A627", "#FF0000"], filename="biexciton_dressed",
                             firstonly=False, visible_states=None, return_eigenvectors=False, **options):
    """Dressed states of the driven biexciton cascade (pyaceqd/four_level_system/linear.py:41-43): the reference's
    tuple t, populations, e_values, ds_occ, s_colors, n_colors[, e_vectors, rho]."""
    from ..general_system.general_dressed_states import dressed_states
    return dressed_states(biexciton, 4, t_start, t_end, *pulses, filename=filename, t_lim=t_lim, e_lim=e_lim,
                          plot=plot, firstonly=firstonly, colors=colors, visible_states=visible_states,
                          return_eigenvectors=return_eigenvectors, **options)


def biexciton_photons_dressed_states(t_start, t_end, *pulses, plot=True, t_lim=None, e_lim=None,
                                     filename="biexciton_photons_dressed", firstonly=False, visible_states=None,
                                     **options):
    """Dressed states of the biexciton in two cavity modes (pyaceqd/four_level_system/linear.py:105-109), dim
    [4, n_phot1 + 1, n_phot2 + 1]: the reference's tuple, equally spaced colours. The reference needs n_phot1 and
    n_phot2 among the options (KeyError otherwise); absent, biexciton_photons' defaults (1, 1: dim 16) are taken."""
    from ..general_system.general_dressed_states import dressed_states
    dim = [4, options.get("n_phot1", 1) + 1, options.get("n_phot2", 1) + 1]
    return dressed_states(biexciton_photons, dim, t_start, t_end, *pulses, filename=filename, plot=plot, t_lim=t_lim,
                          e_lim=e_lim, firstonly=firstonly, colors=None, visible_states=visible_states, **options)


def biexciton_photons_extended_dressed_states(t_start, t_end, *pulses, plot=True, t_lim=None, e_lim=None,
                                              filename="biexciton_photons_extended_dressed", firstonly=False,
                                              visible_states=None, **options):
    """Dressed states of the 18-state biexciton-cavity model with two excitations in total
    (pyaceqd/four_level_system/linear.py:157-159): the reference's tuple, equally spaced colours."""
    from ..general_system.general_dressed_states import dressed_states
    return dressed_states(biexciton_photons_extended, 18, t_start, t_end, *pulses, filename=filename, t_lim=t_lim,
                          e_lim=e_lim, plot=plot, firstonly=firstonly, colors=None, visible_states=visible_states,
                          **options)
