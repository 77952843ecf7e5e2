"""In-memory engine interface: the numeric content of an ACE param file as arrays, run on libpqd.

This is what `system_ace_stream` (general_system/general_system.py) lowers the operator strings to.
It replaces the param-file / `ACE` subprocess / outfile round trip of the reference
(pyaceqd/general_system/general_system.py:227-343) with one C-ABI call, batched over trajectories.

Objects
  System        H0, Lindblad terms, pulse channels (add_Hamiltonian / add_Lindblad / add_Pulse lines)
  Grid          ta, dt, n_steps (te = ta + n_steps dt), n_sub exponential-midpoint sub-steps
  ProcessTensor PT-MPO slices Q[s][g][d][d'], closures, dictionary map g(alpha), slice schedule
  Trajectories  per-trajectory output window [begin, end] and multi-time operators (MTOs)
"""
from dataclasses import dataclass, field
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .constants import hbar as HBAR

KIND = {"": 0, "_left": 1, "_right": 2}


def _c(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


@dataclass
class System:
    dim: int
    H0: np.ndarray
    lindblad: List[Tuple[float, np.ndarray]] = field(default_factory=list)
    channels: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)  # (X, samples f[k])
    sample_t0: float = 0.0
    sample_dt: float = 1.0
    hbar: float = HBAR

    def to_c(self):
        N = self.dim
        keep = {}
        keep["H0"] = _c(self.H0).reshape(N, N)
        if self.lindblad:
            keep["lr"] = np.ascontiguousarray([float(r) for r, _ in self.lindblad], dtype=np.float64)
            keep["lo"] = _c(np.stack([o for _, o in self.lindblad])).reshape(-1, N, N)
        if self.channels:
            keep["co"] = _c(np.stack([x for x, _ in self.channels])).reshape(-1, N, N)
            ns = {len(f) for _, f in self.channels}
            if len(ns) != 1:
                raise ValueError("all pulse channels must share one sample grid")
            keep["cs"] = _c(np.stack([f for _, f in self.channels]))
        s = _lib.pqd_system()
        s.dim = N
        s.hbar = float(self.hbar)
        s.H0 = _lib.cptr(keep["H0"])
        s.n_lind = len(self.lindblad)
        s.lind_rates = _lib.fptr(keep.get("lr"))
        s.lind_ops = _lib.cptr(keep.get("lo"))
        s.n_chan = len(self.channels)
        s.chan_ops = _lib.cptr(keep.get("co"))
        s.chan_samples = _lib.cptr(keep.get("cs"))
        s.n_samples = int(keep["cs"].shape[1]) if self.channels else 0
        s.sample_t0 = float(self.sample_t0)
        s.sample_dt = float(self.sample_dt)
        return s, keep


@dataclass
class Grid:
    ta: float
    dt: float
    n_steps: int
    n_sub: int = 1

    def to_c(self):
        g = _lib.pqd_grid()
        g.ta, g.dt, g.n_steps, g.n_sub = float(self.ta), float(self.dt), int(self.n_steps), int(self.n_sub)
        return g

    @property
    def times(self):
        return self.ta + self.dt * np.arange(self.n_steps + 1)


@dataclass
class ProcessTensor:
    """PT-MPO for a diagonal system-bath coupling.

    Q[s, g] is the chi x chi transfer matrix of slice s for dictionary entry g; gmap[alpha] = g for
    Liouville index alpha = i*N + j. Step n uses slice sched(n): n < n_init -> n, afterwards the
    slices [n_init, n_slices) repeat periodically (n_slices = n_init + 1: stationary / "infinite" PT).
    """
    Q: np.ndarray
    closure: np.ndarray
    closure0: np.ndarray
    bond0: np.ndarray
    gmap: np.ndarray
    n_init: int = None
    dt: Optional[float] = None
    meta: Optional[dict] = None   # generation parameters (ptgen.generation_key); stored by pt.save_pt

    def __post_init__(self):
        self.Q = _c(self.Q)
        assert self.Q.ndim == 4 and self.Q.shape[2] == self.Q.shape[3]
        self.closure = _c(self.closure).reshape(self.Q.shape[0], self.chi)
        self.closure0 = _c(self.closure0).reshape(self.chi)
        self.bond0 = _c(self.bond0).reshape(self.chi)
        self.gmap = np.ascontiguousarray(self.gmap, dtype=np.int32)
        if self.n_init is None:
            self.n_init = self.n_slices - 1
        self._handles = {}

    @property
    def chi(self):
        return self.Q.shape[2]

    @property
    def n_slices(self):
        return self.Q.shape[0]

    @property
    def D(self):
        return self.Q.shape[1]

    def schedule(self, n_steps):
        n = np.arange(n_steps, dtype=np.int64)
        per = max(1, self.n_slices - self.n_init)
        s = np.where(n < self.n_init, n, self.n_init + (n - self.n_init) % per)
        return np.ascontiguousarray(np.minimum(s, self.n_slices - 1), dtype=np.int32)

    def handle(self, ctx, dim, wide=False):
        """device-resident copy (uploaded once per context, shared by all calls). wide=True: the handle of
        pqd_pt_create_wide (dim 2..24), which sends a plan onto the Hilbert-space path with a PT"""
        key = (id(ctx), dim, bool(wide))
        if key not in self._handles:
            d = _lib.pqd_pt_desc()
            d.chi, d.D, d.n_slices = self.chi, self.D, self.n_slices
            d.Q, d.closure, d.closure0 = _lib.cptr(self.Q), _lib.cptr(self.closure), _lib.cptr(self.closure0)
            d.bond0, d.gmap = _lib.cptr(self.bond0), _lib.iptr(self.gmap)
            h = C.c_void_p()
            create = _lib.lib().pqd_pt_create_wide if wide else _lib.lib().pqd_pt_create
            _lib.check(create(ctx.handle, int(dim), C.byref(d), C.byref(h)))
            self._handles[key] = (h, ctx)
        return self._handles[key][0]

    def __del__(self):
        try:
            for h, _ctx in getattr(self, "_handles", {}).values():
                _lib.lib().pqd_pt_destroy(h)
        except Exception:
            pass


@dataclass
class MTO:
    traj: int
    step: int
    before: bool
    kind: int          # 0 "", 1 "_left", 2 "_right"
    op: np.ndarray


@dataclass
class Trajectories:
    out_begin: np.ndarray
    out_end: np.ndarray
    mtos: List[MTO] = field(default_factory=list)
    system: Optional[np.ndarray] = None   # per-trajectory index into a list of systems (scans)

    @property
    def n_traj(self):
        return len(self.out_begin)

    def offsets(self, n_out):
        lens = (np.asarray(self.out_end, dtype=np.int64) - np.asarray(self.out_begin, dtype=np.int64) + 1) * n_out
        off = np.zeros(len(lens), dtype=np.int64)
        if len(lens) > 1:
            off[1:] = np.cumsum(lens)[:-1]
        return off, int(lens.sum()) if len(lens) else 0

    def to_c(self, n_out, N):
        keep = {}
        keep["b"] = np.ascontiguousarray(self.out_begin, dtype=np.int32)
        keep["e"] = np.ascontiguousarray(self.out_end, dtype=np.int32)
        off, total = self.offsets(n_out)
        keep["o"] = off
        t = _lib.pqd_traj()
        t.n_traj = self.n_traj
        t.out_begin, t.out_end, t.out_offset = _lib.iptr(keep["b"]), _lib.iptr(keep["e"]), _lib.lptr(off)
        t.n_mto = len(self.mtos)
        if self.mtos:
            keep["mt"] = np.ascontiguousarray([m.traj for m in self.mtos], dtype=np.int32)
            keep["ms"] = np.ascontiguousarray([m.step for m in self.mtos], dtype=np.int32)
            keep["mb"] = np.ascontiguousarray([1 if m.before else 0 for m in self.mtos], dtype=np.int32)
            keep["mk"] = np.ascontiguousarray([m.kind for m in self.mtos], dtype=np.int32)
            keep["mo"] = _c(np.stack([np.asarray(m.op).reshape(N, N) for m in self.mtos]))
            t.mto_traj, t.mto_step, t.mto_before = _lib.iptr(keep["mt"]), _lib.iptr(keep["ms"]), _lib.iptr(keep["mb"])
            t.mto_kind, t.mto_ops = _lib.iptr(keep["mk"]), _lib.cptr(keep["mo"])
        return t, keep, total


def split_output(out, traj, n_out):
    """flat output buffer -> list of (window_len, n_out) arrays, one per trajectory"""
    off, _ = traj.offsets(n_out)
    res = []
    for t in range(traj.n_traj):
        L = int(traj.out_end[t] - traj.out_begin[t] + 1)
        res.append(out[off[t]: off[t] + L * n_out].reshape(L, n_out))
    return res


def _systems(system):
    return list(system) if isinstance(system, (list, tuple)) else [system]


def _prep(system, grid, rho0, out_ops, traj, pt, ctx, wide_pt=False):
    systems = _systems(system)
    N = systems[0].dim
    if any(s.dim != N for s in systems):
        raise ValueError("all systems of a batch must have the same dimension")
    convs = [s.to_c() for s in systems]
    sc = (_lib.pqd_system * len(systems))(*[c for c, _ in convs])
    k1 = [k for _, k in convs]
    gc = grid.to_c()
    r0 = _c(rho0).reshape(N * N)
    ops = _c(np.stack([np.asarray(o).reshape(N, N) for o in out_ops]))
    tc, k2, total = traj.to_c(len(out_ops), N)
    pth = None
    sched = None
    if pt is not None:
        if pt.gmap.shape[0] != N * N:
            raise ValueError(f"PT gmap has {pt.gmap.shape[0]} entries, system needs {N * N}")
        if pt.dt is not None and abs(float(pt.dt) - float(grid.dt)) > 1e-9 * abs(float(grid.dt)):
            # a PT is a discretisation at its own dt (the eta_k are integrals over dt-wide slices): propagating it
            # on another grid is wrong physics, not a numerical detail
            raise ValueError(f"PT was generated for dt = {pt.dt}, the grid has dt = {grid.dt}")
        pth = pt.handle(ctx, N, wide_pt)
        sched = pt.schedule(max(1, grid.n_steps))
    tsys = np.ascontiguousarray(np.zeros(max(1, traj.n_traj)) if traj.system is None else traj.system, dtype=np.int32)
    if len(systems) == 1 and traj.system is not None and np.any(tsys != 0):
        raise ValueError("trajectory system index out of range")
    keep = (k1, k2, r0, ops, sched, sc, gc, tc, tsys, len(systems))
    return keep, total


def propagate(system, grid: Grid, rho0, out_ops: Sequence, traj: Trajectories,
              pt: Optional[ProcessTensor] = None, ctx=None, *, wide_pt=False):
    """Run all trajectories; returns a list of (window_len, n_out) complex arrays.
    `system` may be a list of Systems (parameter scan); traj.system then selects one per trajectory.
    wide_pt=True (here, in propagate_table, propagate_trapz and Plan) hands the PT over as a wide handle
    (pqd_pt_create_wide): the run takes the Hilbert-space path with a PT, at any dim in [2, 24]. Without it a PT
    needs dim <= 6, as before."""
    ctx = ctx or _lib.context()
    dim = _systems(system)[0].dim
    with ctx.lock:
        keep, total = _prep(system, grid, rho0, out_ops, traj, pt, ctx, wide_pt)
        k1, k2, r0, ops, sched, sc, gc, tc, tsys, n_sys = keep
        out = np.zeros(max(1, total), dtype=np.complex128)
        pth = pt.handle(ctx, dim, wide_pt) if pt is not None else None
        _lib.check(_lib.lib().pqd_propagate_multi(ctx.handle, n_sys, sc, _lib.iptr(tsys), C.byref(gc), pth,
                                                  _lib.iptr(sched), _lib.cptr(r0), len(out_ops), _lib.cptr(ops),
                                                  C.byref(tc), _lib.cptr(out), max(1, total)))
    return split_output(out, traj, len(out_ops))


def live_rows(system, rho0, traj: Optional[Trajectories] = None):
    """The Liouville rows alpha = i N + j that can ever be nonzero (pqd_live_rows; host only, no device): reachable from
    the nonzero entries of rho0 through L0, the generators of every channel with a nonzero sample, and the MTOs of
    `traj`; the union over a list of systems. Returns a sorted list of row indices. The batched sweep contracts only
    these rows with the PT (PQD_LIVE_ROWS)."""
    systems = _systems(system)
    N = systems[0].dim
    if any(s.dim != N for s in systems):
        raise ValueError("all systems of a batch must have the same dimension")
    convs = [s.to_c() for s in systems]
    sc = (_lib.pqd_system * len(systems))(*[c for c, _ in convs])
    r0 = _c(rho0).reshape(N * N)
    tc, keep = (None, None) if traj is None else traj.to_c(1, N)[:2]
    mask = (C.c_uint8 * (N * N))()
    _lib.check(_lib.lib().pqd_live_rows(len(systems), sc, _lib.cptr(r0), None if tc is None else C.byref(tc), mask))
    del convs, keep
    return [a for a in range(N * N) if mask[a]]


def table_offsets(traj: Trajectories, n_out):
    """offsets of the per-trajectory ACE tables ((1 + n_out) rows of the window) in a pqd_propagate_table buffer"""
    L = np.asarray(traj.out_end, dtype=np.int64) - np.asarray(traj.out_begin, dtype=np.int64) + 1
    off = np.zeros(traj.n_traj + 1, dtype=np.int64)
    np.cumsum((1 + n_out) * L, out=off[1:])
    return off, L


def split_table(table, traj, n_out):
    """flat table buffer -> list of (1 + n_out, window_len) views, one per trajectory"""
    off, L = table_offsets(traj, n_out)
    return [table[off[t]: off[t + 1]].reshape(1 + n_out, int(L[t])) for t in range(traj.n_traj)]


def tables_from_outputs(outs, traj: Trajectories, grid: Grid):
    """host form of the device table assembly (pqd_propagate_table): per-trajectory (window_len, n_out) outputs ->
    (1 + n_out, window_len) tables with the step times in row 0 (the oracle-backed tests route through this)"""
    res = []
    for b, o in zip(traj.out_begin, outs):
        r = np.empty((1 + o.shape[1], o.shape[0]), dtype=np.complex128)
        r[0] = grid.ta + grid.dt * np.arange(int(b), int(b) + o.shape[0])
        r[1:] = o.T
        res.append(r)
    return res


def propagate_trapz(system, grid: Grid, rho0, out_ops: Sequence, traj: Trajectories, k_head, k_tail, dx,
                    pt: Optional[ProcessTensor] = None, ctx=None, *, wide_pt=False):
    """propagate() reduced on the device to trapezoid integrals over each trajectory's output window
    (pqd_propagate_trapz): res[t, q] = dx (y_{k_head[q]}(0) / 2 + sum_{s=1}^{L-2} y_{k_tail[q]}(s) + y_{k_tail[q]}(L-1) / 2),
    0 for windows shorter than 2 steps. The tau integrals of G2_reuse (pol_entanglement/G2.py:484-505) without
    downloading the tables. Returns (n_traj, n_pairs) complex."""
    ctx = ctx or _lib.context()
    dim = _systems(system)[0].dim
    kh = np.ascontiguousarray(k_head, dtype=np.int32)
    kt = np.ascontiguousarray(k_tail, dtype=np.int32)
    if kh.shape != kt.shape or kh.ndim != 1:
        raise ValueError("k_head and k_tail must be 1-D of equal length")
    res = np.zeros((max(1, traj.n_traj), max(1, len(kh))), dtype=np.complex128)
    with ctx.lock:
        keep, total = _prep(system, grid, rho0, out_ops, traj, pt, ctx, wide_pt)
        k1, k2, r0, ops, sched, sc, gc, tc, tsys, n_sys = keep
        pth = pt.handle(ctx, dim, wide_pt) if pt is not None else None
        _lib.check(_lib.lib().pqd_propagate_trapz(ctx.handle, n_sys, sc, _lib.iptr(tsys), C.byref(gc), pth,
                                                  _lib.iptr(sched), _lib.cptr(r0), len(out_ops), _lib.cptr(ops),
                                                  C.byref(tc), len(kh), _lib.iptr(kh), _lib.iptr(kt), float(dx),
                                                  _lib.cptr(res)))
    return res[: traj.n_traj, : len(kh)]


def propagate_table(system, grid: Grid, rho0, out_ops: Sequence, traj: Trajectories,
                    pt: Optional[ProcessTensor] = None, ctx=None, *, wide_pt=False):
    """propagate() returning ACE's output table per trajectory: (1 + n_out, window_len) arrays, row 0 = the step
    times grid.ta + dt * step, row 1 + k = output k (general_system.py:343), assembled on the device
    (pqd_propagate_table) so the arrays are views of one host buffer."""
    ctx = ctx or _lib.context()
    dim = _systems(system)[0].dim
    off, _ = table_offsets(traj, len(out_ops))
    n_tab = int(off[-1])
    with ctx.lock:
        keep, total = _prep(system, grid, rho0, out_ops, traj, pt, ctx, wide_pt)
        k1, k2, r0, ops, sched, sc, gc, tc, tsys, n_sys = keep
        table = np.empty(max(1, n_tab), dtype=np.complex128)
        pth = pt.handle(ctx, dim, wide_pt) if pt is not None else None
        _lib.check(_lib.lib().pqd_propagate_table(ctx.handle, n_sys, sc, _lib.iptr(tsys), C.byref(gc), pth,
                                                  _lib.iptr(sched), _lib.cptr(r0), len(out_ops), _lib.cptr(ops),
                                                  C.byref(tc), _lib.cptr(table), max(1, n_tab)))
    return split_table(table, traj, len(out_ops))


def free_propagators(system: System, grid: Grid, ctx=None):
    """M[2n + h] = free propagator of half step h of step n (N^2 x N^2, row-major vec convention)"""
    ctx = ctx or _lib.context()
    N2 = system.dim ** 2
    with ctx.lock:
        sc, keep = system.to_c()
        gc = grid.to_c()
        M = np.zeros((max(1, 2 * grid.n_steps), N2, N2), dtype=np.complex128)
        _lib.check(_lib.lib().pqd_free_propagators(ctx.handle, C.byref(sc), C.byref(gc), _lib.cptr(M)))
    return M[: 2 * grid.n_steps]


def dynmap_wide(system: System, grid: Grid, pt: Optional[ProcessTensor] = None, mtos: Sequence = (), ta=None,
                ctx=None):
    """Dynamical maps on the Hilbert-space paths (pqd_dynmap_wide), dim 2..24: complex (n_maps, n_steps, N^2, N^2),
    dm[m, n] = E(ta[m] + (n + 1) dt, ta[m]) acting on row-major vec(rho). Column beta is the state that started as the
    basis element |i><j| (beta = i N + j), written out after every step by one workgroup; the maps are assembled on the
    device and downloaded once. ta: the maps' start times (None: one map from grid.ta). mtos (MTO objects, `traj`
    ignored) are applied inside every map, in the order of a step. pt: propagated as a wide handle
    (pqd_pt_create_wide), the closed reduced state is read out. kernel time: dynmap_kernel_ms."""
    ctx = ctx or _lib.context()
    N = system.dim
    tav = np.ascontiguousarray([grid.ta] if ta is None else np.atleast_1d(ta), dtype=np.float64)
    if tav.ndim != 1 or len(tav) < 1:
        raise ValueError("ta must be a non-empty 1-D sequence of start times")
    mtos = list(mtos)
    ms = mb = mk = mo = None
    if mtos:
        ms = np.ascontiguousarray([m.step for m in mtos], dtype=np.int32)
        mb = np.ascontiguousarray([1 if m.before else 0 for m in mtos], dtype=np.int32)
        mk = np.ascontiguousarray([m.kind for m in mtos], dtype=np.int32)
        mo = _c(np.stack([np.asarray(m.op).reshape(N, N) for m in mtos]))
    sched = None
    if pt is not None:
        if pt.gmap.shape[0] != N * N:
            raise ValueError(f"PT gmap has {pt.gmap.shape[0]} entries, system needs {N * N}")
        if pt.dt is not None and abs(float(pt.dt) - float(grid.dt)) > 1e-9 * abs(float(grid.dt)):
            raise ValueError(f"PT was generated for dt = {pt.dt}, the grid has dt = {grid.dt}")
        sched = pt.schedule(max(1, grid.n_steps))
    n_steps = max(0, int(grid.n_steps))
    dm = np.empty((len(tav), n_steps, N * N, N * N), dtype=np.complex128)
    with ctx.lock:
        sc, keep = system.to_c()
        gc = grid.to_c()
        pth = pt.handle(ctx, N, True) if pt is not None else None
        _lib.check(_lib.lib().pqd_dynmap_wide(ctx.handle, C.byref(sc), C.byref(gc), pth, _lib.iptr(sched), len(tav),
                                              _lib.fptr(tav), len(mtos), _lib.iptr(ms), _lib.iptr(mb), _lib.iptr(mk),
                                              _lib.cptr(mo), _lib.cptr(dm.reshape(-1)) if dm.size else None, dm.size))
    return dm


def dynmap_kernel_ms(ctx=None):
    """duration (ms, device events) of the propagation kernel of the context's last dynmap_wide call"""
    ctx = ctx or _lib.context()
    ms = C.c_double()
    _lib.check(_lib.lib().pqd_dynmap_timing(ctx.handle, C.byref(ms)))
    return ms.value


DRESSED_LAUNCHES = 0  # pqd_dressed_states[_wide] calls issued by this process (tests count launches with it)


def dressed_states(system_or_systems, grid: Grid, rho=None, want_vectors=True, ctx=None):
    """Dressed states of every system at every output time of `grid` in one launch (pqd_dressed_states for dim <= 6,
    pqd_dressed_states_wide for dim 7..24): the eigenpairs of H(t_n) = H0 + sum_p (f_p(t_n) X_p + h.c.), Lindblad
    terms and n_sub ignored.

    Returns (evals, evecs, occ), each with leading axes (n_sys, n_steps + 1), or (n_steps + 1,) when a single System
    (not a list) was passed: evals (..., N) ascending; evecs (..., N, N) with evecs[..., j, i] = component i of
    eigenvector j (unit norm, first component above 1e-12 real and positive), None when want_vectors is False;
    occ (..., N) = Re sum_ik v_j[i] conj(v_j[k]) rho[..., i, k] for rho of shape (n_sys, n_steps + 1, N, N) (the
    reference's formula, general_dressed_states.py:161-165), None when rho is None."""
    global DRESSED_LAUNCHES
    ctx = ctx or _lib.context()
    single = not isinstance(system_or_systems, (list, tuple))
    systems = _systems(system_or_systems)
    N = systems[0].dim
    if any(s.dim != N for s in systems):
        raise ValueError("all systems of a batch must have the same dimension")
    n_sys, n_t = len(systems), int(grid.n_steps) + 1
    r = None
    if rho is not None:
        r = _c(rho)
        if r.size != n_sys * n_t * N * N:
            raise ValueError(f"rho has {r.size} elements, {n_sys} systems x {n_t} times x {N} x {N} are needed")
        r = r.reshape(n_sys, n_t, N, N)
    evals = np.empty((n_sys, n_t, N), dtype=np.float64)
    evecs = np.empty((n_sys, n_t, N, N), dtype=np.complex128) if want_vectors else None
    occ = np.empty((n_sys, n_t, N), dtype=np.float64) if r is not None else None
    with ctx.lock:
        convs = [s.to_c() for s in systems]
        sc = (_lib.pqd_system * n_sys)(*[c for c, _ in convs])
        gc = grid.to_c()
        DRESSED_LAUNCHES += 1
        # N <= 6: a column per lane in registers (dressed.hip); above: the LDS-resident solver, N <= 24 (dressed_wide.hip)
        call = _lib.lib().pqd_dressed_states if N <= 6 else _lib.lib().pqd_dressed_states_wide
        _lib.check(call(ctx.handle, n_sys, sc, C.byref(gc), _lib.cptr(r), _lib.fptr(evals), _lib.cptr(evecs),
                        _lib.fptr(occ)))
    if single:
        return evals[0], None if evecs is None else evecs[0], None if occ is None else occ[0]
    return evals, evecs, occ


def dressed_kernel_ms(ctx=None):
    """kernel duration (ms, device events) of the context's last dressed_states call"""
    ctx = ctx or _lib.context()
    ms = C.c_double()
    _lib.check(_lib.lib().pqd_dressed_timing(ctx.handle, C.byref(ms)))
    return ms.value


def dressed_table(times, evals, evecs):
    """The table the reference reads from timedep_eigenstates' `.ds` file (general_dressed_states.py:62-70): complex
    (1 + N + N^2, n_t), row 0 = time, rows 1..N the eigenvalues, row 1 + N + i N + j = component j of eigenvector i."""
    evals = np.asarray(evals)
    n_t, N = evals.shape
    tab = np.empty((1 + N + N * N, n_t), dtype=np.complex128)
    tab[0] = times
    tab[1: 1 + N] = evals.T
    tab[1 + N:] = np.asarray(evecs).reshape(n_t, N * N).T
    return tab


class Plan:
    """Device-resident propagation job for repeated execution (bench.py, parameter scans)."""

    def __init__(self, system, grid, rho0, out_ops, traj, pt=None, ctx=None, *, wide_pt=False):
        self.ctx = ctx or _lib.context()
        self.traj = traj
        self.n_out = len(out_ops)
        self.dim = _systems(system)[0].dim
        with self.ctx.lock:
            self._keep, self.total = _prep(system, grid, rho0, out_ops, traj, pt, self.ctx, wide_pt)
            k1, k2, r0, ops, sched, sc, gc, tc, tsys, n_sys = self._keep
            pth = pt.handle(self.ctx, self.dim, wide_pt) if pt is not None else None
            h = C.c_void_p()
            _lib.check(_lib.lib().pqd_plan_create_multi(self.ctx.handle, n_sys, sc, _lib.iptr(tsys), C.byref(gc),
                                                        pth, _lib.iptr(sched), _lib.cptr(r0), self.n_out,
                                                        _lib.cptr(ops), C.byref(tc), max(1, self.total),
                                                        C.byref(h)))
            self.handle = h
        self._pt = pt

    def execute(self, rebuild_free=True):
        _lib.check(_lib.lib().pqd_plan_execute(self.handle, 1 if rebuild_free else 0))

    def synchronize(self):
        """wait for the last execute; re-runs a timed-out split launch on the batched kernel, raises
        _lib.NumericError on NaN/Inf outputs"""
        _lib.check(_lib.lib().pqd_plan_synchronize(self.handle))

    PATHS = {0: "no PT (one wave per trajectory)", 1: "batched lock-step sweep", 2: "split groups",
             3: "register-resident TLS quads", 4: "split groups, several trajectories per group",
             5: "no PT, Hilbert space (one workgroup per trajectory)",
             6: "wide PT, Hilbert space (one workgroup per trajectory, bond slices in a workspace)"}

    def info(self):
        """(path name, trajectories per workgroup, split launches that fell back to the batched kernel)"""
        p, b, f, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().pqd_plan_info(self.handle, C.byref(p), C.byref(b), C.byref(f), C.byref(n)))
        return self.PATHS[p.value], b.value, f.value

    def windows(self):
        """True when the free propagators are built through pulse windows"""
        on = C.c_int32()
        _lib.check(_lib.lib().pqd_plan_windows(self.handle, C.byref(on)))
        return bool(on.value)

    def sweep_lean(self):
        """True when the batched sweep runs the lean instance of the lock-step kernel (the headline configuration
        only: N = 4, chi = 64, 8 trajectories per workgroup, default switches; PQD_SWEEP_LEAN=0 forces the general one)"""
        on = C.c_int32()
        _lib.check(_lib.lib().pqd_plan_sweep_lean(self.handle, C.byref(on)))
        return bool(on.value)

    def sweep_readout(self):
        """True when the lean instance reads this plan's outputs inside its fused column phase: some workgroup has steps
        after its last MTO and before its last two steps (PQD_LEAN_RO=0 keeps the closure pass everywhere)"""
        on = C.c_int32()
        _lib.check(_lib.lib().pqd_plan_sweep_readout(self.handle, C.byref(on)))
        return bool(on.value)

    def sweep_stage(self):
        """the number of workgroups whose fast steps (sweep_readout) take F(n), W(n) and the closure vector from LDS,
        staged there a step ahead: those whose trajectories share one system (PQD_LEAN_STAGE=0: none)"""
        n = C.c_int32()
        _lib.check(_lib.lib().pqd_plan_sweep_stage(self.handle, C.byref(n)))
        return int(n.value)

    def sweep_colk(self):
        """the k-steps of four rows in which the plan's fast steps (sweep_readout) apply the fused column operator: 3 where
        the lean instance deals 9 to 12 live rows of 16 in quarters and multiplies them in their compact index
        (pqd_live_col_map), else 4 (PQD_LIVE_COL=0: always 4). Results are bit-identical either way"""
        k = C.c_int32()
        _lib.check(_lib.lib().pqd_plan_sweep_colk(self.handle, C.byref(k)))
        return int(k.value)

    def describe(self):
        """every decision plan creation took (pqd_plan_describe) as a dict of strings: path, workgroup shape, split /
        quad / trunk layout, windows, the A/B switches, and hashes of the block, row-unit and group tables. A plan whose
        sweep leaves out rows that stay zero (live_rows) has two more entries at the end: "live", the mask of the rows it
        contracts (hex, bit alpha), and "parts", 1 when the lean instance deals them in quarters; and behind them
        "colk" = 3 where the column phase runs three k-steps (sweep_colk)"""
        buf = C.create_string_buffer(2048)
        _lib.check(_lib.lib().pqd_plan_describe(self.handle, buf, len(buf)))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split())

    def live_rows(self):
        """the Liouville rows the plan's sweep contracts with the PT, sorted (pqd_plan_live_rows): every row unless the
        plan runs the batched sweep and some rows stay exactly zero (engine.live_rows; PQD_LIVE_ROWS=0: every row)"""
        n = self.dim * self.dim
        mask = (C.c_uint8 * n)()
        _lib.check(_lib.lib().pqd_plan_live_rows(self.handle, mask, n))
        return [a for a in range(n) if mask[a]]

    def traj_steps(self):
        """trajectory-steps one execute propagates (shared trunks counted once per workgroup)"""
        p, b, f, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.lib().pqd_plan_info(self.handle, C.byref(p), C.byref(b), C.byref(f), C.byref(n)))
        return n.value

    def output_device_ptr(self):
        return _lib.lib().pqd_plan_output_device(self.handle)

    def output_tensor(self, device=None):
        """the outputs as one flat complex128 torch tensor on `device` (default: this plan's GPU), copied device to
        device after synchronize; the input of a collective gather (scan.gather_tensor)"""
        import torch
        dev = torch.device(device) if device is not None else torch.device("cuda", self.ctx.device)
        t = torch.empty(max(1, self.total), dtype=torch.complex128, device=dev)
        _lib.check(_lib.lib().pqd_plan_copy_output(self.handle, C.c_void_p(t.data_ptr()), max(1, self.total)))
        return t[: self.total]

    def download_table(self):
        """the outputs as ACE tables (propagate_table's layout): list of (1 + n_out, window_len) views"""
        n = C.c_int64()
        _lib.check(_lib.lib().pqd_plan_table_len(self.handle, C.byref(n)))
        table = np.empty(max(1, n.value), dtype=np.complex128)
        _lib.check(_lib.lib().pqd_plan_download_table(self.handle, _lib.cptr(table), max(1, n.value)))
        return split_table(table, self.traj, self.n_out)

    def download(self):
        out = np.zeros(max(1, self.total), dtype=np.complex128)
        _lib.check(_lib.lib().pqd_plan_download(self.handle, _lib.cptr(out), max(1, self.total)))
        return split_output(out, self.traj, self.n_out)

    def timing(self, reset=True):
        f, w, n = C.c_double(), C.c_double(), C.c_int32()
        _lib.check(_lib.lib().pqd_plan_timing(self.handle, C.byref(f), C.byref(w), C.byref(n), 1 if reset else 0))
        return f.value, w.value, n.value

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().pqd_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
