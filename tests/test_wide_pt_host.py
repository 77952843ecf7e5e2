"""Phonons above dim 6 (the wide_pt opt-in), host side only: the generated PT of a coupling blown up by an identity
factor is the bare one with a blown-up dictionary map, and the drop-in layer lets phonons=True through at dim 7..24
only under wide_pt=True or PQD_WIDE_PT=1. No GPU: the lowered problem is returned before a PT or a device is touched."""
import numpy as np
import pytest

from pyaceqd_amd import pt as ptmod
from pyaceqd_amd import ptgen
from pyaceqd_amd.general_system import general_system as gs
from pyaceqd_amd.pulses import ChirpedPulse
from pyaceqd_amd.two_level_system.tls import tls_photons, tls_two_sensor

GEN = dict(t_mem=2.0, threshold=1e-6, max_bond=24)


@pytest.mark.parametrize("diag", [(0, 1), (0, 1, 1, 2)])
def test_generated_pt_of_a_blown_up_coupling_is_the_bare_one(diag):
    """kron(B, I_4) has B's eigenvalue pairs: the same Q, closures and bond vector, array-equal, and the dictionary
    map of B repeated over the identity factor's 4 x 4 indices"""
    B, k = np.diag(np.array(diag, dtype=float)), 4
    n = len(diag)
    bare = ptgen.qd_phonon_pt(B, 0.5, **GEN)
    wide = ptgen.qd_phonon_pt(np.kron(B, np.eye(k)), 0.5, **GEN)
    for name in ("Q", "closure", "closure0", "bond0"):
        np.testing.assert_array_equal(getattr(wide, name), getattr(bare, name), err_msg=name)
    assert wide.n_init == bare.n_init and wide.chi == bare.chi <= 24 and wide.D == bare.D == (4 if n == 2 else 9)
    want = np.empty((n * k) ** 2, dtype=np.int32)
    for i in range(n * k):
        for j in range(n * k):
            want[i * n * k + j] = bare.gmap[(i // k) * n + (j // k)]
    np.testing.assert_array_equal(wide.gmap, want)
    np.testing.assert_array_equal(wide.gmap, ptmod.pair_dictionary(np.kron(B, np.eye(k)))[0])


def _pulse():
    return ChirpedPulse(tau_0=1.0, e_start=0.0, e0=1.0, t0=2.0)


def _no_pt_no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the PT / the device")
    for name in ("_resolve_pt", "propagate", "propagate_table", "propagate_trapz", "dressed_states"):
        monkeypatch.setattr(gs, name, boom)


def test_wide_pt_lowers_tls_photons_with_phonons(monkeypatch):
    _no_pt_no_device(monkeypatch)
    monkeypatch.delenv("PQD_WIDE_PT", raising=False)
    low = tls_photons(0, 1, _pulse(), dt=0.1, phonons=True, wide_pt=True, lower_only=True)
    assert isinstance(low, gs.Lowered) and low.systems[0].dim == 18 and low.grid.n_steps == 10 and low.n_t == [11]
    same = tls_photons(0, 1, _pulse(), dt=0.1, phonons=False, lower_only=True)
    np.testing.assert_array_equal(low.systems[0].H0, same.systems[0].H0)


@pytest.mark.parametrize("kw", [dict(), dict(wide_pt=False), dict(wide_pt=None)])
def test_without_the_opt_in_the_old_error_is_raised(kw, monkeypatch):
    _no_pt_no_device(monkeypatch)
    monkeypatch.delenv("PQD_WIDE_PT", raising=False)
    with pytest.raises(NotImplementedError, match=r"phonons.*dim <= 6.*dim 18"):
        tls_photons(0, 1, _pulse(), dt=0.1, phonons=True, lower_only=True, **kw)
    with pytest.raises(NotImplementedError, match=r"phonons.*dim <= 6.*dim 8.*wide_pt"):
        tls_two_sensor(0, 1, _pulse(), dt=0.1, phonons=True, **kw)


def test_environment_switch_opts_in(monkeypatch):
    _no_pt_no_device(monkeypatch)
    monkeypatch.setenv("PQD_WIDE_PT", "1")
    low = tls_photons(0, 1, _pulse(), dt=0.1, phonons=True, lower_only=True)
    assert low.systems[0].dim == 18
    with pytest.raises(NotImplementedError, match="phonons"):  # an explicit False wins over the environment
        tls_photons(0, 1, _pulse(), dt=0.1, phonons=True, lower_only=True, wide_pt=False)
    monkeypatch.setenv("PQD_WIDE_PT", "0")
    with pytest.raises(NotImplementedError, match="phonons"):
        tls_photons(0, 1, _pulse(), dt=0.1, phonons=True, lower_only=True)


def test_wide_pt_reaches_the_engine_only_where_it_applies(monkeypatch):
    """dim 8 with phonons: the PT is resolved and engine.propagate_table gets wide_pt=True; dim 2 gets no such keyword"""
    seen = []
    pt8 = ptmod.random_pt(8, 3, D=4, n_slices=2, seed=1)
    pt2 = ptmod.random_pt(2, 3, D=4, n_slices=2, seed=1)
    monkeypatch.setattr(gs, "_resolve_pt", lambda pt_file, boson_mat, **k: pt8 if boson_mat.shape[0] == 8 else pt2)

    def spy(system, grid, rho0, out_ops, traj, pt=None, ctx=None, **kw):
        seen.append((system.dim, pt, kw))
        return [np.zeros((1 + len(out_ops), grid.n_steps + 1), dtype=complex)]
    monkeypatch.setattr(gs, "propagate_table", spy)
    from pyaceqd_amd import _lib
    monkeypatch.setattr(_lib, "context", lambda device=None: None)
    tls_two_sensor(0, 1, _pulse(), dt=0.1, phonons=True, wide_pt=True)
    from pyaceqd_amd.two_level_system.tls import tls
    tls(0, 1, _pulse(), dt=0.1, phonons=True, wide_pt=True)
    assert seen[0] == (8, pt8, {"wide_pt": True}) and seen[1] == (2, pt2, {})


@pytest.mark.parametrize("wide", [True, None])
def test_dynmap_and_get_M_t_stay_refused_at_dim_7(wide, monkeypatch):
    _no_pt_no_device(monkeypatch)
    monkeypatch.setenv("PQD_WIDE_PT", "1")
    with pytest.raises(NotImplementedError, match="calc_dynmap.*dim <= 6.*dim 7"):
        gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_7", output_ops=["|1><1|_7"], calc_dynmap=True,
                             wide_pt=wide)
    with pytest.raises(NotImplementedError, match="get_M_t.*dim <= 6.*dim 7"):
        gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_7", output_ops=["|1><1|_7"], get_M_t=0.5, wide_pt=wide)
    with pytest.raises(NotImplementedError, match="dressedstates.*dim <= 6.*dim 7"):
        gs.system_ace_stream(0, 1, dt=0.1, initial="|0><0|_7", output_ops=["|1><1|_7"], dressedstates=True,
                             wide_pt=wide)
