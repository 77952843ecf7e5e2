"""Generates tests/golden/pyref_params_cavity.json: the ACE param text (and %.8f pulse files) the REFERENCE's cavity
and sensor models write with prepare_only=True, captured as make_golden.py gen_params captures `tls`, `biexciton`
and `sixls_linear` (same import path for the reference, same tokens for the temp-file paths).

The nine models: tls_one_sensor, tls_two_sensor, tls_photon, tls_photons, tls_photon_sensor, tls_photon_two_sensor
(two_level_system/tls.py) and biexciton_photons, biexciton_photons_extended, biexciton_sensors
(four_level_system/linear.py), each with non-default arguments, two pulses and a list of three multi-time operators
(all three kinds, both applyBefore values). tests/test_params_cavity_golden.py lowers the same calls through our
wrappers and checks every param line. Run in the build container only (it needs the reference tree):

    python tests/golden/make_golden_cavity.py
"""
import contextlib
import io
import json
import os
import tempfile
import warnings

from make_golden import HERE, _ref_correlations


def _mto(lower, raise_, proj):
    return [{"operator": lower, "applyFrom": "_left", "applyBefore": "false", "time": 1.5},
            {"operator": raise_, "applyFrom": "_right", "time": 1.5},
            {"operator": proj, "applyFrom": "", "applyBefore": "true", "time": 2.0}]


def cases():
    """function name -> (module below the package, keyword arguments); the golden records both, and the test calls our
    function of that name in our module of that name"""
    tls_mod, lin_mod = "two_level_system.tls", "four_level_system.linear"
    return {
        "tls_one_sensor": (tls_mod, dict(
            dt=0.1, lindblad=True, gamma_e=0.02, delta_s1=0.4, epsilon=0.003, linewidth1=0.05,
            multitime_op=_mto("|0><1|_2 otimes Id_2", "|1><0|_2 otimes Id_2", "Id_2 otimes |1><1|_2"))),
        "tls_two_sensor": (tls_mod, dict(
            dt=0.1, lindblad=True, gamma_e=0.02, delta_s1=0.4, delta_s2=-0.3, epsilon=0.003, linewidth1=0.05,
            linewidth2=0.07, multitime_op=_mto("|0><1|_2 otimes Id_2 otimes Id_2", "|1><0|_2 otimes Id_2 otimes Id_2",
                                               "Id_2 otimes Id_2 otimes |1><1|_2"))),
        "tls_photon": (tls_mod, dict(
            dt=0.1, lindblad=True, gamma_e=0.02, cav_coupl1=0.08, cav_loss1=0.2, delta_cx1=-1.5, n_phot1=3,
            laser_cav_coupl=0.25, multitime_op=_mto("Id_2 otimes b_4", "Id_2 otimes bdagger_4", "|1><1|_2 otimes Id_4"))),
        "tls_photons": (tls_mod, dict(
            dt=0.1, lindblad=True, gamma_e=0.02, cav_coupl1=0.08, cav_loss1=0.2, delta_cx1=-1.5, cav_coupl2=0.05,
            cav_loss2=0.3, delta_cx2=0.7, n_phot1=2, n_phot2=1, laser_cav_coupl=0.25,
            multitime_op=_mto("Id_2 otimes b_3 otimes Id_2", "Id_2 otimes bdagger_3 otimes Id_2",
                              "|1><1|_2 otimes Id_3 otimes Id_2"))),
        "tls_photon_sensor": (tls_mod, dict(
            dt=0.1, lindblad=True, gamma_e=0.02, cav_coupl1=0.08, cav_loss1=0.2, delta_cx1=-1.5, delta_s1=0.4,
            epsilon=0.003, linewidth1=0.05, n_phot1=2,
            multitime_op=_mto("Id_2 otimes b_3 otimes Id_2", "Id_2 otimes bdagger_3 otimes Id_2",
                              "Id_2 otimes Id_3 otimes |1><1|_2"))),
        "tls_photon_two_sensor": (tls_mod, dict(
            dt=0.1, lindblad=True, gamma_e=0.02, cav_coupl1=0.08, cav_loss1=0.2, delta_cx1=-1.5, delta_s1=0.4,
            delta_s2=-0.3, epsilon=0.003, linewidth1=0.05, linewidth2=0.07, n_phot1=2,
            multitime_op=_mto("Id_2 otimes b_3 otimes Id_2 otimes Id_2", "Id_2 otimes bdagger_3 otimes Id_2 otimes Id_2",
                              "Id_2 otimes Id_3 otimes Id_2 otimes |1><1|_2"))),
        "biexciton_photons": (lin_mod, dict(
            dt=0.1, lindblad=True, delta_xy=0.1, delta_b=3.0, gamma_e=0.02, gamma_b=0.03, cav_coupl=0.08, cav_loss=0.2,
            delta_cx=-1.5, n_phot1=2, n_phot2=1,
            multitime_op=_mto("Id_4 otimes b_3 otimes Id_2", "Id_4 otimes bdagger_3 otimes Id_2",
                              "|3><3|_4 otimes Id_3 otimes Id_2"))),
        "biexciton_photons_extended": (lin_mod, dict(
            dt=0.1, lindblad=True, delta_xy=0.1, delta_b=3.0, gamma_e=0.02, gamma_b=0.03, cav_coupl=0.08, cav_loss=0.2,
            delta_cx=-1.5, multitime_op=_mto("|0><1|_18 + sqrt(2)*|1><4|_18", "|1><0|_18 + sqrt(2)*|4><1|_18",
                                             "|14><14|_18"))),
        "biexciton_sensors": (lin_mod, dict(
            dt=0.1, lindblad=True, delta_xy=0.1, delta_b=3.0, gamma_e=0.02, gamma_b=0.03, delta_s1=0.4, delta_s2=-0.3,
            epsilon=0.003, linewidth1=0.05, linewidth2=0.07,
            multitime_op=_mto("|0><1|_4 otimes Id_2 otimes Id_2", "|1><0|_4 otimes Id_2 otimes Id_2",
                              "Id_4 otimes |1><1|_2 otimes Id_2"))),
    }


def gen_params_cavity():
    import importlib
    warnings.simplefilter("ignore")
    _ref_correlations()
    from pyaceqd.pulses import ChirpedPulse  # noqa: E402
    p1 = ChirpedPulse(tau_0=1.0, e_start=0.2, e0=1.3, t0=2.0, alpha=5.0, phase=0.3)
    p2 = ChirpedPulse(tau_0=0.8, e_start=-1.0, e0=0.7, t0=3.0, polar_x=0.6)
    out = {}
    for name, (mod, kw) in cases().items():
        fn = getattr(importlib.import_module("pyaceqd." + mod), name)
        tmp = tempfile.mkdtemp() + "/"
        with contextlib.redirect_stdout(io.StringIO()):
            fn(0, 4, p1, p2, temp_dir=tmp, prepare_only=True, suffix="g", **kw)
        files = sorted(os.listdir(tmp))
        params = [f for f in files if f.endswith(".param")]
        assert len(params) == 1, files
        text = open(tmp + params[0]).read()
        rec = {"module": mod, "kwargs": dict(kw), "pulse_files": {}}
        for f in files:
            if f.endswith(".dat"):
                tok = "<PULSE_Y>" if "_y_" in f else "<PULSE_X>"
                text = text.replace(tmp + f, tok)
                rec["pulse_files"][tok] = open(tmp + f).read()
        rec["param"] = text.replace(tmp, "<TMP>/")
        out[name] = rec
    with open(os.path.join(HERE, "pyref_params_cavity.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    gen_params_cavity()
