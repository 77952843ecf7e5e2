"""The cavity and sensor models pinned to the ACE param text the REFERENCE writes for them.

tests/golden/pyref_params_cavity.json holds the param files (and %.8f pulse files) of the reference's tls_one_sensor,
tls_two_sensor, tls_photon, tls_photons, tls_photon_sensor, tls_photon_two_sensor, biexciton_photons,
biexciton_photons_extended and biexciton_sensors, captured with prepare_only=True, non-default arguments, two pulses
and three multi-time operators (tests/golden/make_golden_cavity.py). Our wrappers are called with the same arguments;
the lowered engine inputs are captured and every param line is checked against them, exactly as
tests/test_params_golden.py does for the 2-, 4- and 6-level models (its _capture and _parse are used here):
H0, Lindblad terms and rates in order, pulse couplings and samples, initial state, outputs, multi-time operators.
"""
import importlib
import inspect
import json
import os

import numpy as np
import pytest

from pyaceqd_amd import opgrammar
from pyaceqd_amd.pulses import ChirpedPulse
from tests.test_params_golden import _capture, _parse

NAMES = ["tls_one_sensor", "tls_two_sensor", "tls_photon", "tls_photons", "tls_photon_sensor", "tls_photon_two_sensor",
         "biexciton_photons", "biexciton_photons_extended", "biexciton_sensors"]
DIMS = dict(zip(NAMES, [4, 8, 8, 12, 12, 24, 24, 18, 16]))  # with the golden arguments (n_phot as captured)


@pytest.fixture(scope="module")
def params(golden_dir):
    with open(os.path.join(golden_dir, "pyref_params_cavity.json")) as f:
        return json.load(f)


def _ours(name, g):
    return getattr(importlib.import_module("pyaceqd_amd." + g["module"]), name)


def test_golden_holds_the_nine_models(params):
    assert sorted(params) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_cavity_model_lowering_matches_reference_param_file(params, name, monkeypatch):
    g = params[name]
    rec = _parse(g["param"])
    kw = dict(g["kwargs"])
    p1 = ChirpedPulse(tau_0=1.0, e_start=0.2, e0=1.3, t0=2.0, alpha=5.0, phase=0.3)
    p2 = ChirpedPulse(tau_0=0.8, e_start=-1.0, e0=0.7, t0=3.0, polar_x=0.6)
    got = _capture(monkeypatch)
    _ours(name, g)(0, 4, p1, p2, suffix="g", **kw)
    sysd, grid = got["system"], got["grid"]
    N = sysd.dim
    assert N == DIMS[name]
    M = lambda s: opgrammar.to_matrix(s, N)  # noqa: E731
    assert grid.ta == rec["ta"] and grid.dt == rec["dt"] and grid.ta + grid.n_steps * grid.dt == pytest.approx(rec["te"])
    np.testing.assert_allclose(np.asarray(got["rho0"]).reshape(N, N), M(rec["initial"]), atol=0)
    H = sum((M(s) for s in rec["ham"]), np.zeros((N, N), dtype=complex))
    np.testing.assert_allclose(sysd.H0, H, rtol=1e-15, atol=1e-15)
    assert len(sysd.lindblad) == len(rec["lind"])
    for (r, L), (rr, s) in zip(sysd.lindblad, rec["lind"]):
        assert r == rr
        np.testing.assert_allclose(L, M(s), atol=0)
    assert len(sysd.channels) == len(rec["pulse"])
    ts_file = rec["ta"] + rec["dt"] * np.arange(grid.n_steps)
    for (X, f), (tok, s) in zip(sysd.channels, rec["pulse"]):
        np.testing.assert_allclose(X, M(s), rtol=1e-15, atol=1e-15)
        d = np.loadtxt(g["pulse_files"][tok].splitlines())
        np.testing.assert_allclose(d[:, 0], ts_file, atol=5e-9)
        k = np.rint((ts_file - sysd.sample_t0) / sysd.sample_dt).astype(int)
        np.testing.assert_allclose(sysd.sample_t0 + k * sysd.sample_dt, ts_file, atol=1e-12)
        fs = np.asarray(f)[k]
        assert np.max(np.abs(fs.real - d[:, 1])) <= 5.01e-9 and np.max(np.abs(fs.imag - d[:, 2])) <= 5.01e-9
    outs = got["out_ops"]
    assert len(outs) == len(rec["out"])
    for O, s in zip(outs, rec["out"]):
        np.testing.assert_allclose(O, M(s), atol=0)
    mtos = got["traj"].mtos
    assert len(mtos) == len(rec["mto"]) == 3
    kinds = {"": 0, "_left": 1, "_right": 2}
    for m, (side, t, s, before) in zip(mtos, rec["mto"]):
        assert m.step == int(round((t - rec["ta"]) / rec["dt"])) and m.kind == kinds[side] and m.before == before
        np.testing.assert_allclose(m.op, M(s), atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_default_arguments_lower_too(params, name, monkeypatch):
    """the defaults (n_phot, output operators, initial state) give a consistent system of the documented dimension"""
    got = _capture(monkeypatch)
    p1 = ChirpedPulse(tau_0=1.0, e_start=0.0, e0=1.0, t0=2.0)
    _ours(name, params[name])(0, 1, p1, dt=0.1)
    want = {"tls_one_sensor": 4, "tls_two_sensor": 8, "tls_photon": 6, "tls_photons": 18, "tls_photon_sensor": 12,
            "tls_photon_two_sensor": 24, "biexciton_photons": 16, "biexciton_photons_extended": 18,
            "biexciton_sensors": 16}[name]
    sysd = got["system"]
    assert sysd.dim == want and np.allclose(sysd.H0, np.asarray(sysd.H0).conj().T)
    assert np.asarray(got["rho0"]).reshape(want, want)[0, 0] == 1 and len(got["out_ops"]) in (2, 4)


def test_wrappers_keep_the_reference_keywords(params):
    """every keyword of a captured call is a named parameter of our wrapper (none swallowed by **options)"""
    for name in NAMES:
        sig = inspect.signature(_ours(name, params[name]))
        for k in params[name]["kwargs"]:
            assert k in sig.parameters and sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, (name, k)
        for k in ("dt", "phonons", "lindblad", "temp_dir", "pt_file", "suffix", "multitime_op", "prepare_only",
                  "output_ops", "initial", "dressedstates", "rf", "rf_file", "firstonly"):
            assert k in sig.parameters, (name, k)


@pytest.mark.parametrize("kw,word", [(dict(phonons=True), "phonons"), (dict(dressedstates=True), "dressedstates")])
def test_above_dim_6_refuses_what_needs_superoperators(kw, word, monkeypatch):
    """phonons / dressed states at dim 18: NotImplementedError naming the keyword and the limit, before a PT is
    generated or read and before any device call"""
    from pyaceqd_amd.general_system import general_system as gs
    from pyaceqd_amd.two_level_system.tls import tls_photons

    def boom(*a, **k):
        raise AssertionError("reached the PT / the device")
    monkeypatch.setattr(gs, "_resolve_pt", boom)
    monkeypatch.setattr(gs, "dressed_states", boom)
    with pytest.raises(NotImplementedError, match=word + r".*dim <= 6.*dim 18"):
        tls_photons(0, 1, ChirpedPulse(tau_0=1.0, e_start=0.0, e0=1.0, t0=2.0), dt=0.1, **kw)
    with pytest.raises(NotImplementedError, match="dim <= 6"):
        gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_7", output_ops=["|1><1|_7"], calc_dynmap=True)
    with pytest.raises(NotImplementedError, match="get_M_t"):
        gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_7", output_ops=["|1><1|_7"], get_M_t=0.5)
