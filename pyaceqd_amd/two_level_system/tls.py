"""Two-level quantum dot (pyaceqd/two_level_system/tls.py:16-77), on libpqd.

Same signature and defaults as the reference `tls`; the operator strings are identical (H on
|1><1|_2 via e_x, x-polarised pulse coupling |1><0|_2, boson operator phonon_factor*|1><1|_2,
radiative decay |0><1|_2, optional pure dephasing). Unknown keywords (`trajectories`, `n_sub`,
`device`) are forwarded to system_ace_stream so the two-time sweeps can batch trajectories.

Below it the reference's cavity and sensor variants (tls_one_sensor, tls_two_sensor, tls_photon, tls_photons,
tls_photon_sensor, tls_photon_two_sensor; pyaceqd/two_level_system/tls.py:89-349), dim 4 to 24: without phonons they
propagate at any of these sizes, everything else stops at dim 6. `phonons=True` above dim 6 is an opt-in: the forwarded
keyword `wide_pt=True` (or PQD_WIDE_PT=1), see system_ace_stream. `calc_dynmap=True` and `get_M_t` above dim 6 are an
opt-in too: the forwarded keyword `wide_maps=True` (or PQD_WIDE_MAPS=1).
"""
from ..general_system.general_system import system_ace_stream
from .. import constants

hbar = constants.hbar
temp_dir = constants.temp_dir

_FWD = ("trajectories", "n_sub", "device", "pulse_sampling", "trapz", "dressed_rho", "lower_only", "wide_pt",
        "wide_maps", "calc_dynmap", "get_M_t", "rho0")  # the last three: for the wrappers whose signature lacks them
# (rho0: the tl_* correlation sweeps hand every system their rho0; the cavity and sensor wrappers used to drop it)


def tls(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, phonons=False, t_mem=6.4, ae=5.0, temperature=4,
        verbose=False, lindblad=False, temp_dir=temp_dir, pt_file=None, suffix="", multitime_op=None,
        pulse_file=None, pulse_file_x=None, prepare_only=False,
        output_ops=["|0><0|_2", "|1><1|_2", "|0><1|_2", "|1><0|_2"], phonon_factor=1.0, LO_params=None,
        dressedstates=False, rf=False, rf_file=None, firstonly=False, dephasing=None, J_to_file=None, J_file=None,
        factor_ah=None, use_infinite=True, threshold=8, calc_dynmap=False, rho0=None, e_x=0, get_M_t=None,
        initial="|0><0|_2", **options):
    system_op = ["({}*|1><1|_2)".format(e_x)] if e_x != 0 else None
    boson_op = "{:.3f}*|1><1|_2".format(phonon_factor)
    lindblad_ops = [["|0><1|_2", gamma_e]] if lindblad else []
    if dephasing is not None:
        lindblad_ops.append(["|0><0|_2-|1><1|_2", dephasing])
    interaction_ops = [["|1><0|_2", "x"]]
    rf_op = "|1><1|_2" if rf else None
    if pulse_file is None and pulse_file_x is not None:
        pulse_file = pulse_file_x
    fwd = {k: options[k] for k in _FWD if k in options}
    return system_ace_stream(
        t_start, t_end, *pulses, dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature,
        verbose=verbose, temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
        pulse_file_x=pulse_file, system_prefix="tls", threshold=str(int(threshold)), threshold_ratio="0.3",
        buffer_blocksize="-1", dict_zero="16", precision="12", boson_e_max=7, system_op=system_op,
        boson_op=boson_op, initial=initial, lindblad_ops=lindblad_ops, interaction_ops=interaction_ops,
        output_ops=output_ops, prepare_only=prepare_only, LO_params=LO_params, dressedstates=dressedstates,
        rf_op=rf_op, rf_file=rf_file, firstonly=firstonly, J_to_file=J_to_file, J_file=J_file,
        factor_ah=factor_ah, use_infinite=use_infinite, calc_dynmap=calc_dynmap, rho0=rho0, get_M_t=get_M_t, **fwd)


# ---------------------------------------------------------------------------------------------------------------
# Two-level system with cavity modes and sensors (pyaceqd/two_level_system/tls.py:89-349). The Hilbert space is a
# tensor product: site 0 the two-level system, then the cavity modes (n_phot + 1 levels each), then the two-level
# sensors. dim = 4 .. 24: above 6 only the propagation without phonons exists (general_system.system_ace_stream).
# All six models are one construction (tls_composite_ops) with the reference's operator strings, in its order:
#   H:        cavity detunings, Jaynes-Cummings couplings, sensor detunings, sensor couplings
#   Lindblad: radiative decay (lindblad=True), cavity losses, sensor losses
# A sensor couples to the first cavity mode where there is one, else to the two-level system itself.
# ---------------------------------------------------------------------------------------------------------------
def _sites(dims, ops):
    """the product operator with ops[k] on site k and the identity elsewhere"""
    return " otimes ".join(ops.get(k, "Id_{}".format(d)) for k, d in enumerate(dims))


def tls_composite_ops(cavs, sensors, gamma_e, lindblad, rf, laser_cav_coupl, epsilon):
    """cavs: [(levels, coupling, loss, detuning)], sensors: [(detuning, linewidth)].
    Returns system_op, boson_op, lindblad_ops, interaction_ops, rf_op, initial, output_ops."""
    dims = [2] + [c[0] for c in cavs] + [2] * len(sensors)
    nc = len(cavs)
    on = lambda **ops: _sites(dims, {int(k[1:]): v for k, v in ops.items()})  # noqa: E731  on(s0=.., s2=..)
    boson_op = on(s0="|1><1|_2")
    initial = _sites(dims, {k: "|0><0|_{}".format(d) for k, d in enumerate(dims)})
    output_ops = [on(s0="|0><0|_2"), on(s0="|1><1|_2")]
    lindblad_ops = [[on(s0="|0><1|_2"), gamma_e]] if lindblad else []
    interaction_ops = [[on(s0="|1><0|_2"), "x"]]
    if laser_cav_coupl is not None:
        interaction_ops.append(["{}*({})".format(laser_cav_coupl, on(s1="bdagger_{}".format(dims[1]))), "x"])
    rf_op = None
    if rf:
        rf_op = " + ".join([on(s0="|1><1|_2")] + [_sites(dims, {1 + k: "n_{}".format(dims[1 + k])}) for k in range(nc)])
    system_op = []
    for k, (n, _, _, delta) in enumerate(cavs):
        system_op.append(" {} * ({})".format(delta, _sites(dims, {1 + k: "n_{}".format(n)})))
    for k, (n, g, _, _) in enumerate(cavs):
        system_op.append(" {} * ({} + {})".format(g, _sites(dims, {0: "|1><0|_2", 1 + k: "b_{}".format(n)}),
                                                  _sites(dims, {0: "|0><1|_2", 1 + k: "bdagger_{}".format(n)})))
    for k, (n, _, loss, _) in enumerate(cavs):
        lindblad_ops.append([_sites(dims, {1 + k: "b_{}".format(n)}), loss])
    for k, (delta, _) in enumerate(sensors):
        system_op.append("{} * ({})".format(delta, _sites(dims, {1 + nc + k: "|1><1|_2"})))
    # the emitter a sensor reads: raising / lowering operator of the first cavity mode, or of the two-level system
    up, down = ("bdagger_{}".format(dims[1]), "b_{}".format(dims[1])) if nc else ("|1><0|_2", "|0><1|_2")
    src = 1 if nc else 0
    for k in range(len(sensors)):
        system_op.append("{} * ({} + {})".format(epsilon, _sites(dims, {src: up, 1 + nc + k: "|0><1|_2"}),
                                                 _sites(dims, {src: down, 1 + nc + k: "|1><0|_2"})))
    for k, (_, width) in enumerate(sensors):
        lindblad_ops.append([_sites(dims, {1 + nc + k: "|0><1|_2"}), width])
    return system_op, boson_op, lindblad_ops, interaction_ops, rf_op, initial, output_ops


def _run_composite(prefix, built, t_start, t_end, pulses, options, initial, output_ops, pulse_file, **kw):
    system_op, boson_op, lindblad_ops, interaction_ops, rf_op, initial0, output_ops0 = built
    fwd = {k: options[k] for k in _FWD if k in options}
    if pulse_file is None:
        # Purity and Indistinguishability hand every system its pulse train as pulse_file_x (tls takes it the same way);
        # the wrappers that name the argument pulse_file used to drop it with the other unknown keywords
        pulse_file = options.get("pulse_file_x")
    return system_ace_stream(
        t_start, t_end, *pulses, pulse_file_x=pulse_file, system_prefix=prefix, threshold="10", threshold_ratio="0.3",
        buffer_blocksize="-1", dict_zero="16", precision="12", boson_e_max=7, system_op=system_op, boson_op=boson_op,
        initial=initial0 if initial is None else initial, lindblad_ops=lindblad_ops, interaction_ops=interaction_ops,
        output_ops=output_ops0 if output_ops is None else output_ops, rf_op=rf_op, **kw, **fwd)


def _rf_needs_file(rf, pulse_file, rf_file):
    """the reference's check (tls.py:183-185): a pulse file in the rotating frame needs the frame's file too"""
    if rf and pulse_file is not None and rf_file is None:
        print("Error: pulse file is given, but no file for rotating frame")
        return True
    return False


def tls_two_sensor(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, phonons=False, t_mem=10, ae=3.0, delta_s1=0,
                   delta_s2=0, epsilon=0.0001, linewidth1=0.01, linewidth2=None, temperature=1, verbose=False,
                   lindblad=False, temp_dir=temp_dir, pt_file=None, suffix="", multitime_op=None, pulse_file=None,
                   prepare_only=False,
                   output_ops=["|0><0|_2 otimes Id_2 otimes Id_2", "|1><1|_2 otimes Id_2 otimes Id_2"], initial=None,
                   dressedstates=False, rf=False, rf_file=None, firstonly=False, calc_dynmap=False,
                   use_infinite=False, get_M_t=None, **options):
    """Two-level system read out by two sensors (dim 8; tls.py:89-124)."""
    sensors = [(delta_s1, linewidth1), (delta_s2, linewidth1 if linewidth2 is None else linewidth2)]
    built = tls_composite_ops([], sensors, gamma_e, lindblad, rf, None, epsilon)
    return _run_composite("tls_two_sensor", built, t_start, t_end, pulses, options, initial, output_ops, pulse_file,
                          dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature, verbose=verbose,
                          temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
                          prepare_only=prepare_only, dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly,
                          use_infinite=use_infinite, calc_dynmap=calc_dynmap, get_M_t=get_M_t)


def tls_one_sensor(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, phonons=False, t_mem=10, ae=3.0, delta_s1=0,
                   epsilon=0.0001, linewidth1=0.01, temperature=1, verbose=False, lindblad=False, temp_dir=temp_dir,
                   pt_file=None, suffix="", multitime_op=None, pulse_file=None, prepare_only=False,
                   output_ops=["|0><0|_2 otimes Id_2", "|1><1|_2 otimes Id_2"], initial=None, dressedstates=False,
                   rf=False, rf_file=None, firstonly=False, calc_dynmap=False, use_infinite=False, get_M_t=None,
                   **options):
    """Two-level system read out by one sensor (dim 4; tls.py:126-157)."""
    built = tls_composite_ops([], [(delta_s1, linewidth1)], gamma_e, lindblad, rf, None, epsilon)
    return _run_composite("tls_one_sensor", built, t_start, t_end, pulses, options, initial, output_ops, pulse_file,
                          dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature, verbose=verbose,
                          temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
                          prepare_only=prepare_only, dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly,
                          use_infinite=use_infinite, calc_dynmap=calc_dynmap, get_M_t=get_M_t)


def tls_photons(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, cav_coupl1=0.06, cav_loss1=0.12/hbar, delta_cx1=-2,
                cav_coupl2=None, cav_loss2=None, delta_cx2=-2, phonons=False, t_mem=10, ae=5.0, temperature=4,
                verbose=False, lindblad=False, temp_dir=temp_dir, pt_file=None, suffix="", multitime_op=None,
                n_phot1=2, n_phot2=2, laser_cav_coupl=None, pulse_file=None, prepare_only=False, output_ops=None,
                dressedstates=False, rf=False, rf_file=None, firstonly=False, initial=None, **options):
    """Two-level system in two cavity modes (dim 2 (n_phot1 + 1) (n_phot2 + 1), 18 by default; tls.py:159-205)."""
    if _rf_needs_file(rf, pulse_file, rf_file):
        return 0
    cavs = [(n_phot1 + 1, cav_coupl1, cav_loss1, delta_cx1),
            (n_phot2 + 1, cav_coupl1 if cav_coupl2 is None else cav_coupl2,
             cav_loss1 if cav_loss2 is None else cav_loss2, delta_cx2)]
    built = tls_composite_ops(cavs, [], gamma_e, lindblad, rf, laser_cav_coupl, None)
    return _run_composite("tls_cavity", built, t_start, t_end, pulses, options, initial, output_ops, pulse_file,
                          dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature, verbose=verbose,
                          temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
                          prepare_only=prepare_only, dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly)


def tls_photon(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, cav_coupl1=0.06, cav_loss1=0.12/hbar, delta_cx1=-2,
               phonons=False, t_mem=10, ae=5.0, temperature=4, verbose=False, lindblad=False, temp_dir=temp_dir,
               pt_file=None, suffix="", multitime_op=None, n_phot1=2, laser_cav_coupl=None, pulse_file_x=None,
               prepare_only=False, output_ops=None, dressedstates=False, rf=False, rf_file=None, firstonly=False,
               initial=None, use_infinite=True, calc_dynmap=False, rho0=None, **options):
    """Two-level system in one cavity mode (dim 2 (n_phot1 + 1), 6 by default; tls.py:214-250)."""
    if _rf_needs_file(rf, pulse_file_x, rf_file):
        return 0
    built = tls_composite_ops([(n_phot1 + 1, cav_coupl1, cav_loss1, delta_cx1)], [], gamma_e, lindblad, rf,
                               laser_cav_coupl, None)
    return _run_composite("tls_cavity", built, t_start, t_end, pulses, options, initial, output_ops, pulse_file_x,
                          dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature, verbose=verbose,
                          temp_dir=temp_dir, pt_file=pt_file, suffix=suffix, multitime_op=multitime_op,
                          prepare_only=prepare_only, dressedstates=dressedstates, rf_file=rf_file, firstonly=firstonly,
                          use_infinite=use_infinite, calc_dynmap=calc_dynmap, rho0=rho0)


def tls_photon_sensor(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, cav_coupl1=0.06, cav_loss1=0.12/hbar,
                      delta_cx1=-2, phonons=False, delta_s1=0, epsilon=0.0001, linewidth1=0.01, t_mem=10, ae=5.0,
                      temperature=4, verbose=False, lindblad=False, temp_dir=temp_dir, pt_file=None, suffix="",
                      multitime_op=None, n_phot1=2, laser_cav_coupl=None, pulse_file_x=None, prepare_only=False,
                      output_ops=None, dressedstates=False, rf=False, rf_file=None, firstonly=False, initial=None,
                      use_infinite=True, calc_dynmap=False, **options):
    """Two-level system in a cavity mode whose field one sensor reads (dim 4 (n_phot1 + 1), 12 by default;
    tls.py:252-296)."""
    if _rf_needs_file(rf, pulse_file_x, rf_file):
        return 0
    built = tls_composite_ops([(n_phot1 + 1, cav_coupl1, cav_loss1, delta_cx1)], [(delta_s1, linewidth1)], gamma_e,
                               lindblad, rf, laser_cav_coupl, epsilon)
    return _run_composite("tls_cavity_sensor", built, t_start, t_end, pulses, options, initial, output_ops,
                          pulse_file_x, dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature,
                          verbose=verbose, temp_dir=temp_dir, pt_file=pt_file, suffix=suffix,
                          multitime_op=multitime_op, prepare_only=prepare_only, dressedstates=dressedstates,
                          rf_file=rf_file, firstonly=firstonly, use_infinite=use_infinite, calc_dynmap=calc_dynmap)


def tls_photon_two_sensor(t_start, t_end, *pulses, dt=0.1, gamma_e=1/100, cav_coupl1=0.06, cav_loss1=0.12/hbar,
                          delta_cx1=-2, phonons=False, delta_s1=0, delta_s2=None, epsilon=0.0001, linewidth1=0.01,
                          linewidth2=None, t_mem=10, ae=5.0, temperature=4, verbose=False, lindblad=False,
                          temp_dir=temp_dir, pt_file=None, suffix="", multitime_op=None, n_phot1=2,
                          laser_cav_coupl=None, pulse_file_x=None, prepare_only=False, output_ops=None,
                          dressedstates=False, rf=False, rf_file=None, firstonly=False, initial=None,
                          use_infinite=True, **options):
    """Two-level system in a cavity mode read by two sensors (dim 8 (n_phot1 + 1), 24 by default; tls.py:298-349)."""
    if _rf_needs_file(rf, pulse_file_x, rf_file):
        return 0
    sensors = [(delta_s1, linewidth1),
               (delta_s1 if delta_s2 is None else delta_s2, linewidth1 if linewidth2 is None else linewidth2)]
    built = tls_composite_ops([(n_phot1 + 1, cav_coupl1, cav_loss1, delta_cx1)], sensors, gamma_e, lindblad, rf,
                               laser_cav_coupl, epsilon)
    return _run_composite("tls_cavity_two_sensor", built, t_start, t_end, pulses, options, initial, output_ops,
                          pulse_file_x, dt=dt, phonons=phonons, t_mem=t_mem, ae=ae, temperature=temperature,
                          verbose=verbose, temp_dir=temp_dir, pt_file=pt_file, suffix=suffix,
                          multitime_op=multitime_op, prepare_only=prepare_only, dressedstates=dressedstates,
                          rf_file=rf_file, firstonly=firstonly, use_infinite=use_infinite)


def tls_dressed_states(t_start, t_end, *pulses, plot=True, t_lim=None, e_lim=None, filename="tls_dressed",
                       firstonly=False, colors=["#0000FF", "#FF0000"], visible_states=None,
                       return_eigenvectors=False, **options):
    """Dressed states of the driven two-level system (pyaceqd/two_level_system/tls.py:79-87): the reference's tuple
    t, populations, e_values, ds_occ, s_colors, n_colors[, e_vectors, rho]. RGBA colours hide states as
    visible_states does, e.g. ["#0000FF00", "#FF0000FF"]. trajectories=[{"pulses": ...}, ...] gives one tuple per
    drive (general_dressed_states.dressed_states)."""
    from ..general_system.general_dressed_states import dressed_states
    return dressed_states(tls, 2, t_start, t_end, *pulses, filename=filename, plot=plot, t_lim=t_lim, e_lim=e_lim,
                          firstonly=firstonly, colors=colors, visible_states=visible_states,
                          return_eigenvectors=return_eigenvectors, **options)


def tls_photons_dressed_states(t_start, t_end, *pulses, plot=True, t_lim=None, e_lim=None,
                               filename="tls_photons_dressed", firstonly=False, visible_states=None, print_states=None,
                               **options):
    """Dressed states of the two-level system in two cavity modes (pyaceqd/two_level_system/tls.py:207-212), dim
    [2, n_phot1 + 1, n_phot2 + 1]: the reference's tuple, equally spaced colours. The reference needs n_phot1 and
    n_phot2 among the options (KeyError otherwise); absent, tls_photons' defaults (2, 2: dim 18) are taken."""
    from ..general_system.general_dressed_states import dressed_states
    dim = [2, options.get("n_phot1", 2) + 1, options.get("n_phot2", 2) + 1]
    return dressed_states(tls_photons, dim, t_start, t_end, *pulses, filename=filename, plot=plot, t_lim=t_lim,
                          e_lim=e_lim, firstonly=firstonly, colors=None, visible_states=visible_states,
                          print_states=print_states, **options)
