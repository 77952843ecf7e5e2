"""Dynamical maps above dim 6 (the wide_maps opt-in), host side only: the drop-in layer lets calc_dynmap and get_M_t
through at dim 7..24 only under wide_maps=True or PQD_WIDE_MAPS=1, hands engine.dynmap_wide the run's system, grid
and MTOs, and changes nothing at dim <= 6. No GPU: engine.dynmap_wide is a spy and everything else that would touch a
PT or the device raises."""
import numpy as np
import pytest

from pyaceqd_amd import _lib, engine
from pyaceqd_amd.general_system import general_system as gs
from pyaceqd_amd.pulses import ChirpedPulse
from pyaceqd_amd.two_level_system.tls import tls, tls_photons, tls_two_sensor


def _pulse():
    return ChirpedPulse(tau_0=1.0, e_start=0.0, e0=1.0, t0=2.0)


def _no_pt_no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the PT / the device")
    for name in ("_resolve_pt", "propagate", "propagate_table", "propagate_trapz", "dressed_states",
                 "free_propagators", "_dynmap"):
        monkeypatch.setattr(gs, name, boom)
    monkeypatch.setattr(engine, "dynmap_wide", boom)
    monkeypatch.setattr(_lib, "context", lambda device=None: None)


def _spy(monkeypatch):
    seen = []

    def spy(system, grid, pt=None, mtos=(), ta=None, ctx=None):
        seen.append(dict(system=system, grid=grid, pt=pt, mtos=list(mtos), ta=ta))
        n_maps = 1 if ta is None else len(ta)
        return np.zeros((n_maps, grid.n_steps, system.dim ** 2, system.dim ** 2), dtype=complex)
    monkeypatch.setattr(engine, "dynmap_wide", spy)
    return seen


def _dim7(**kw):
    return gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_7", output_ops=["|1><1|_7"], **kw)


@pytest.mark.parametrize("env_pt", [None, "1"])
@pytest.mark.parametrize("kw", [dict(), dict(wide_maps=False), dict(wide_maps=None)])
def test_without_the_opt_in_both_refusals_stand(kw, env_pt, monkeypatch):
    _no_pt_no_device(monkeypatch)
    monkeypatch.delenv("PQD_WIDE_MAPS", raising=False)
    if env_pt:
        monkeypatch.setenv("PQD_WIDE_PT", env_pt)
    else:
        monkeypatch.delenv("PQD_WIDE_PT", raising=False)
    with pytest.raises(NotImplementedError, match=r"calc_dynmap.*dim <= 6.*dim 7"):
        _dim7(calc_dynmap=True, **kw)
    with pytest.raises(NotImplementedError, match=r"get_M_t.*dim <= 6.*dim 7"):
        _dim7(get_M_t=0.5, **kw)
    with pytest.raises(NotImplementedError, match=r"get_M_t.*dim <= 6.*dim 7"):
        _dim7(get_M_t=[0.5, 0.6], **kw)
    with pytest.raises(NotImplementedError, match=r"calc_dynmap.*dim <= 6.*dim 18.*wide_maps"):
        tls_photons(0, 1, _pulse(), dt=0.1, calc_dynmap=True, **kw)
    with pytest.raises(NotImplementedError, match=r"get_M_t.*dim <= 6.*dim 18.*wide_maps"):
        tls_photons(0, 1, _pulse(), dt=0.1, get_M_t=0.5, **kw)
    with pytest.raises(NotImplementedError, match=r"calc_dynmap.*dim <= 6.*dim 18"):  # wide_pt alone opens no map
        tls_photons(0, 1, _pulse(), dt=0.1, calc_dynmap=True, wide_pt=True, **kw)


def test_environment_switch_opts_in_and_false_beats_it(monkeypatch):
    _no_pt_no_device(monkeypatch)
    seen = _spy(monkeypatch)
    monkeypatch.setenv("PQD_WIDE_MAPS", "1")
    M = tls_two_sensor(0, 1, _pulse(), dt=0.1, get_M_t=0.5)
    assert M.shape == (64, 64) and len(seen) == 1
    with pytest.raises(NotImplementedError, match="get_M_t"):
        tls_two_sensor(0, 1, _pulse(), dt=0.1, get_M_t=0.5, wide_maps=False)
    monkeypatch.setenv("PQD_WIDE_MAPS", "0")
    with pytest.raises(NotImplementedError, match="get_M_t"):
        tls_two_sensor(0, 1, _pulse(), dt=0.1, get_M_t=0.5)
    with pytest.raises(NotImplementedError, match="calc_dynmap"):
        tls_two_sensor(0, 1, _pulse(), dt=0.1, calc_dynmap=True)
    assert len(seen) == 1


def test_calc_dynmap_hands_over_one_map_with_the_calls_mtos(monkeypatch):
    _no_pt_no_device(monkeypatch)
    seen = _spy(monkeypatch)
    monkeypatch.delenv("PQD_WIDE_MAPS", raising=False)
    tables = []

    def table(system, grid, rho0, out_ops, traj, pt=None, ctx=None, **kw):
        tables.append((system, grid, traj, pt, kw))
        return [np.zeros((1 + len(out_ops), grid.n_steps + 1), dtype=complex)]
    monkeypatch.setattr(gs, "propagate_table", table)
    mt = [{"operator": "|1><0|_2 otimes Id_2 otimes Id_2", "applyFrom": "_left", "time": 0.3, "applyBefore": "false"},
          {"operator": "|0><1|_2 otimes Id_2 otimes Id_2", "applyFrom": "_right", "time": 0.0, "applyBefore": "true"}]
    res, dm = tls_two_sensor(0, 1.2, _pulse(), dt=0.1, calc_dynmap=True, wide_maps=True, multitime_op=mt)
    assert dm.shape == (12, 64, 64) and res.shape == (3, 13)
    (s,) = seen
    assert s["system"].dim == 8 and s["grid"].n_steps == 12 and s["grid"].ta == 0 and s["pt"] is None
    assert s["ta"] is None  # one map from the grid's start
    assert [(m.step, m.before, m.kind) for m in s["mtos"]] == [(3, False, 1), (0, True, 2)]
    assert s["mtos"][0].op[4, 0] == 1 and s["mtos"][1].op[0, 4] == 1
    # `result` is the ordinary propagation of the same system, grid and MTOs
    (t,) = tables
    assert t[0] is s["system"] and t[1] is s["grid"] and t[2].mtos == s["mtos"] and t[4] == {}


def test_get_M_t_is_one_step_from_that_time_without_a_pt(monkeypatch):
    _no_pt_no_device(monkeypatch)
    seen = _spy(monkeypatch)
    monkeypatch.delenv("PQD_WIDE_MAPS", raising=False)
    monkeypatch.delenv("PQD_WIDE_PT", raising=False)
    M = tls_two_sensor(0, 1, _pulse(), dt=0.1, get_M_t=0.5, wide_maps=True, phonons=True, n_sub=2)
    assert M.shape == (64, 64)
    Ms = tls_two_sensor(0, 1, _pulse(), dt=0.1, get_M_t=[0.5, 0.25, 0.7], wide_maps=True)
    assert Ms.shape == (3, 64, 64)
    a, b = seen
    assert a["system"].dim == 8 and a["grid"].n_steps == 1 and a["grid"].dt == 0.1 and a["grid"].n_sub == 2
    assert list(a["ta"]) == [0.5] and a["pt"] is None and a["mtos"] == []
    assert list(b["ta"]) == [0.5, 0.25, 0.7] and b["grid"].n_steps == 1
    # the channels are those of the run's grid (t_start .. t_end), not of a one-step grid
    low = tls_two_sensor(0, 1, _pulse(), dt=0.1, lower_only=True, n_sub=2)
    assert a["system"].sample_t0 == low.systems[0].sample_t0 and a["system"].sample_dt == low.systems[0].sample_dt
    np.testing.assert_array_equal(a["system"].channels[0][1], low.systems[0].channels[0][1])


def test_calc_dynmap_with_phonons_needs_wide_pt_too(monkeypatch):
    _no_pt_no_device(monkeypatch)
    _spy(monkeypatch)
    monkeypatch.delenv("PQD_WIDE_PT", raising=False)
    with pytest.raises(NotImplementedError, match=r"phonons.*dim <= 6.*dim 8.*wide_pt"):
        tls_two_sensor(0, 1, _pulse(), dt=0.1, calc_dynmap=True, wide_maps=True, phonons=True)


def test_calc_dynmap_with_phonons_resolves_the_pt_and_hands_it_over(monkeypatch):
    from pyaceqd_amd import pt as ptmod
    _no_pt_no_device(monkeypatch)
    seen = _spy(monkeypatch)
    pt8 = ptmod.random_pt(8, 3, D=4, n_slices=2, seed=1)
    monkeypatch.setattr(gs, "_resolve_pt", lambda pt_file, boson_mat, **k: pt8)
    kws = []

    def table(system, grid, rho0, out_ops, traj, pt=None, ctx=None, **kw):
        kws.append((pt, kw))
        return [np.zeros((1 + len(out_ops), grid.n_steps + 1), dtype=complex)]
    monkeypatch.setattr(gs, "propagate_table", table)
    tls_two_sensor(0, 1, _pulse(), dt=0.1, calc_dynmap=True, wide_maps=True, wide_pt=True, phonons=True)
    assert seen[0]["pt"] is pt8 and kws == [(pt8, {"wide_pt": True})]


@pytest.mark.parametrize("kw", [dict(calc_dynmap=True), dict(get_M_t=0.5)])
def test_dim_27_is_refused_with_the_opt_in(kw, monkeypatch):
    _no_pt_no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match=r"dim <= 6.*dim 27.*dim <= 24"):
        gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_27", output_ops=["|1><1|_27"], wide_maps=True, **kw)


@pytest.mark.parametrize("maps", [None, True, False])
def test_dim_2_never_reaches_the_wide_entry(maps, monkeypatch):
    seen = _spy(monkeypatch)
    calls = []
    monkeypatch.setattr(_lib, "context", lambda device=None: None)
    monkeypatch.setattr(gs, "_dynmap", lambda *a: calls.append("dynmap") or ("res", "dm"))
    monkeypatch.setattr(gs, "free_propagators",
                        lambda system, grid, ctx=None: calls.append(grid.ta) or np.stack([np.eye(4) * 2, np.eye(4) * 3]))
    monkeypatch.setenv("PQD_WIDE_MAPS", "1")
    kw = {} if maps is None else {"wide_maps": maps}
    assert tls(0, 1, _pulse(), dt=0.1, calc_dynmap=True, **kw) == ("res", "dm")
    np.testing.assert_array_equal(tls(0, 1, _pulse(), dt=0.1, get_M_t=0.5, **kw), 6 * np.eye(4))
    Ms = tls(0, 1, _pulse(), dt=0.1, get_M_t=[0.5, 0.7], **kw)
    assert Ms.shape == (2, 4, 4) and calls == ["dynmap", 0.5, 0.5, 0.7] and not seen
