"""Shared builders for tests: small systems, trajectories and a pure-numpy restatement of the
propagation semantics (used only for tiny sizes, as an independent cross-check of the C oracle)."""
import numpy as np
import scipy.linalg as sla

from pyaceqd_amd.engine import Grid, MTO, System, Trajectories
from pyaceqd_amd.constants import hbar


def ketbra(N, a, b):
    m = np.zeros((N, N), dtype=complex)
    m[a, b] = 1
    return m


def random_system(N, n_chan=2, n_lind=2, seed=0, n_steps=20, dt=0.1, ta=0.0, n_sub=1):
    rng = np.random.default_rng(seed)
    H = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    H = 0.5 * (H + H.conj().T)
    lind = [(0.05 * (k + 1), rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))) for k in range(n_lind)]
    ds = dt / (4 * n_sub)
    ns = 4 * n_sub * n_steps + 1
    tt = ta + ds * np.arange(ns)
    chans = []
    for c in range(n_chan):
        X = 0.5 * (rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N)))
        f = np.exp(-((tt - tt.mean()) / (0.3 * (tt[-1] - tt[0] + 1e-9))) ** 2) * np.exp(1j * (c + 1) * tt)
        chans.append((X, f))
    sysd = System(dim=N, H0=H, lindblad=lind, channels=chans, sample_t0=ta, sample_dt=ds)
    return sysd, Grid(ta, dt, n_steps, n_sub)


def sparse_jump_ops(N, n_lind, seed):
    """(rate, A) with the nonzero structures of the reference models, cycled over k: diagonal, a single entry,
    strictly upper triangular with about N entries, N // 2 occupied rows (chosen at random) of one or two entries;
    from n_lind = 5 on, operator 4 is entirely zero (all its row offsets equal). Rates as random_system's."""
    rng = np.random.default_rng(seed)
    val = lambda: complex(rng.normal(), rng.normal())  # noqa: E731
    ops = []
    for k in range(n_lind):
        A = np.zeros((N, N), dtype=complex)
        kind = k % 4
        if k == 4:
            pass
        elif kind == 0:
            for i in range(N):
                A[i, i] = val()
        elif kind == 1:
            A[int(rng.integers(N)), int(rng.integers(N))] = val()
        elif kind == 2:
            for i in range(N - 1):
                A[i, i + 1] = val()
            A[0, N - 1] = val()
        else:
            for i in rng.choice(N, size=N // 2, replace=False):
                for j in rng.choice(N, size=int(rng.integers(1, 3)), replace=False):
                    A[i, j] = val()
        ops.append((0.05 * (k + 1), A))
    return ops


def offgrid_channels(sysd, grid, cover=(0.23, 0.78), sdt=0.0137 * np.pi, floor=0.3):
    """Replace the samples of every channel of `sysd` (in place; returned for convenience) by samples on a raster
    incommensurate with grid.dt that spans only the `cover` fraction of the run: sub-step midpoints fall between
    samples (interpolation weights all over (0, 1)), before the first and after the last one (clamping). The envelope
    is floor + (1 - floor) 4 x (1 - x) over the samples, so both end values are `floor`: non-zero makes the clamped
    values visible, floor = 0 gives exact zeros at both ends (pulse windows). Sets sample_t0 and sample_dt."""
    T = grid.n_steps * grid.dt
    t_lo, t_hi = grid.ta + cover[0] * T, grid.ta + cover[1] * T
    ns = max(1, int((t_hi - t_lo) / sdt))
    k = np.arange(ns)
    x = k / max(1, ns - 1)
    env = floor + (1.0 - floor) * 4.0 * x * (1.0 - x)
    tt = t_lo + sdt * k
    sysd.channels = [(X, (env * np.exp(1j * (c + 1) * tt)).astype(complex)) for c, (X, _) in enumerate(sysd.channels)]
    sysd.sample_t0 = float(t_lo)
    sysd.sample_dt = float(sdt)
    return sysd


def random_rho(N, seed=1):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    r = A @ A.conj().T
    return r / np.trace(r)


def dense_ops(N, n_out, seed):
    """n_out full complex non-Hermitian N x N operators, normal + 1j * normal each, drawn one operator after the other:
    dense_ops(N, m, seed) is the head of dense_ops(N, n, seed) for m < n, so cases with fewer outputs share the columns
    of one reference"""
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N)) for _ in range(n_out)]


def dense_state(N, seed):
    """a full complex non-Hermitian N x N matrix in place of a density matrix (the two-time callers hand over
    operator-multiplied states)"""
    return dense_ops(N, 1, seed)[0]


def readout_trajectories(N, n_steps, n_traj, seed=0):
    """Trajectories of the output-readout tests (n_steps >= 9, or 8 with up to three trajectories). Windows [b, e] are
    ragged at both ends; trajectory 0 opens its window at step 2. Every trajectory t has three MTOs inside its window,
    at steps b + 1, b + 2 and b + 4, of the kinds t, t + 1, t + 2 mod 3, applied before / after / after for even t and after / before / after for odd t:
    MTOs at steps with outputs, and a single trajectory already sees the kinds 0, 1, 2 and both flags. Trajectory 0 also
    has one at step 0 (before its window, applied before, kind 1) and a second one in its (b + 4, after) slot. The last MTO
    is at step 7 at most, which leaves the rest of the run free of events. The operators are dense, scaled to the
    Frobenius norm sqrt(N) of a unitary: the state keeps its size across an MTO, so every output column takes its
    largest value from four unrelated states and no column of a 256-column table is small against the others."""
    rng = np.random.default_rng(seed)

    def op():
        A = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
        return A * (np.sqrt(N) / np.linalg.norm(A))
    beg = [(2, 0, 1, 3, 0)[t % 5] for t in range(n_traj)]
    end = [n_steps - (0, 3, 1, 2, 4)[t % 5] for t in range(n_traj)]
    mt = []
    for t in range(n_traj):
        b = beg[t]
        mt += [MTO(t, b + 1, t % 2 == 0, t % 3, op()), MTO(t, b + 2, t % 2 == 1, (t + 1) % 3, op()),
               MTO(t, b + 4, False, (t + 2) % 3, op())]
    mt += [MTO(0, 0, True, 1, op()), MTO(0, beg[0] + 4, False, 1, op())]
    return Trajectories(np.array(beg), np.array(end), mt)


def readout_pt(N, chi, seed):
    """pt.random_pt(N, chi, D=min(N * N, 9), n_slices=5, eps=0.1) of the first seed from `seed` on whose closure vectors
    overlap the bond vector alike: |bond0 . c| within a factor 1.5 over closure0 and the five slices' closures. The
    slices are close to the identity, so a step's outputs are those of the reduced state times that overlap, and a random
    PT's overlaps differ up to tenfold from step to step: every column of a trajectory would take its largest value
    at the one step with the largest overlap, and a column that happens to be small there would be small against the rest
    of the table. With even overlaps every step of the window counts."""
    from pyaceqd_amd import pt as ptmod
    for s in range(seed, seed + 1000):
        pt = ptmod.random_pt(N, chi, D=min(N * N, 9), n_slices=5, seed=s, eps=0.1)
        w = np.abs(np.concatenate([[pt.closure0 @ pt.bond0], pt.closure @ pt.bond0]))
        if w.max() < 1.5 * w.min():
            return pt
    raise AssertionError("no seed with even closure overlaps")


def column_errors(got, ref):
    """per trajectory and output column k: max_n |got - ref| / max_n |ref[:, k]|, as one (n_traj, n_out) array, and
    the smallest ratio of a column's max_n |ref| to its trajectory's largest (how far the normalisation is from empty)"""
    assert len(got) == len(ref)
    err, ratio = [], []
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        cmax = np.max(np.abs(b), axis=0)
        err.append(np.max(np.abs(a - b), axis=0) / cmax)
        ratio.append(cmax.min() / cmax.max())
    return np.array(err), float(min(ratio))


def numpy_liouvillian(sysd, t):
    N = sysd.dim
    I = np.eye(N)
    H = np.array(sysd.H0, dtype=complex)
    u = (t - sysd.sample_t0) / sysd.sample_dt
    for X, f in sysd.channels:
        ns = len(f)
        if u <= 0:
            fv = f[0]
        elif u >= ns - 1:
            fv = f[-1]
        else:
            k = int(np.floor(u))
            fv = f[k] + (u - k) * (f[k + 1] - f[k])
        H = H + fv * X + np.conj(fv) * X.conj().T
    L = -1j / sysd.hbar * (np.kron(H, I) - np.kron(I, H.T))
    for g, Lk in sysd.lindblad:
        LdL = Lk.conj().T @ Lk
        L = L + g * (np.kron(Lk, Lk.conj()) - 0.5 * np.kron(LdL, I) - 0.5 * np.kron(I, LdL.T))
    return L


def numpy_free_props(sysd, grid):
    out = []
    w = 0.5 * grid.dt / grid.n_sub
    for n in range(grid.n_steps):
        for h in range(2):
            M = np.eye(sysd.dim ** 2, dtype=complex)
            for j in range(grid.n_sub):
                t = grid.ta + n * grid.dt + h * 0.5 * grid.dt + (j + 0.5) * w
                M = sla.expm(numpy_liouvillian(sysd, t) * w) @ M
            out.append(M)
    return np.array(out)


def numpy_propagate(sysd, grid, rho0, out_ops, traj, pt=None):
    """direct restatement with superoperators and einsum (small sizes only)"""
    N = sysd.dim
    N2 = N * N
    M = numpy_free_props(sysd, grid)
    chi = pt.chi if pt is not None else 1
    res = []
    for t in range(traj.n_traj):
        st = np.outer(np.asarray(rho0).reshape(N2), pt.bond0 if pt is not None else [1.0]).astype(complex)
        b, e = int(traj.out_begin[t]), int(traj.out_end[t])
        rows = []
        mt = [m for m in traj.mtos if m.traj == t]

        def apply(m, st):
            A = np.asarray(m.op)
            S = {0: np.kron(A, A.conj()), 1: np.kron(A, np.eye(N)), 2: np.kron(np.eye(N), A.T)}[m.kind]
            return S @ st
        sched = pt.schedule(max(1, grid.n_steps)) if pt is not None else None
        for n in range(e + 1):
            for m in mt:
                if m.step == n and m.before:
                    st = apply(m, st)
            if n >= b:
                c = (pt.closure0 if n == 0 else pt.closure[sched[n - 1]]) if pt is not None else np.ones(1)
                r = st @ c
                rows.append([np.trace(np.asarray(O) @ r.reshape(N, N)) for O in out_ops])
            for m in mt:
                if m.step == n and not m.before:
                    st = apply(m, st)
            if n == e:
                break
            st = M[2 * n] @ st
            if pt is not None:
                Qs = pt.Q[sched[n]]
                st = np.stack([st[a] @ Qs[pt.gmap[a]] for a in range(N2)])
            st = M[2 * n + 1] @ st
        res.append(np.array(rows))
    return res


# ------------------------------------------------------------------ timebin_tl.f90 restated in long double
# Written from the Fortran (timebin/timebin_tl.f90:13-77, :145-342), not from the C oracle: an independent check of
# oracle/mapchain_oracle.c. Map stacks in the Fortran layout (N2, N2, n), vectors column-major vec(rho). Time and
# index arithmetic stays in float64 (it decides the step counts); states and maps are np.clongdouble. Every function
# also returns the highest index (0-based) of a precalc map it used, -1 when it used none.
LD = np.clongdouble


def tb_round6(x):
    """round_to_6 (:13-20): nint(x * 10^6) / 10^6, nint rounding halves away from zero"""
    v = float(x) * 1000000.0
    n = int(np.floor(abs(v) + 0.5))
    return float(n if v >= 0 else -n) / 1000000.0


def tb_steps(t_start, t_stop, dt, n_dm):
    """(n_start, steps on the explicit maps, steps left to fast_propagate) of propagate_tb (:59-75)"""
    n_start = int(tb_round6(t_start) / dt)
    n_stop = int(tb_round6(t_stop) / dt)
    n_steps = n_stop - n_start
    steps_dm = max(0, min(n_dm - n_start, n_steps))
    return n_start, steps_dm, max(0, n_steps - steps_dm)


def numpy_fast_propagate(rho, precalc, n_steps):
    """fast_propagate (:23-47): one precalc map per set bit of n_steps, least significant first"""
    rho = np.asarray(rho, dtype=LD)
    n, i, top = int(n_steps), 0, -1
    while n > 0:
        if n & 1:
            rho = np.asarray(precalc[:, :, i], dtype=LD) @ rho
            top = i
        n >>= 1
        i += 1
    return rho, top


def numpy_propagate_tb(t_start, t_stop, dt, rho, dm_tl, precalc):
    """propagate_tb (:50-77): explicit maps dm_tl(:, :, n_start + 1 ...) while there are any, then fast_propagate"""
    n_start, steps_dm, rem = tb_steps(t_start, t_stop, dt, dm_tl.shape[2])
    rho = np.asarray(rho, dtype=LD)
    for s in range(steps_dm):
        rho = np.asarray(dm_tl[:, :, n_start + s], dtype=LD) @ rho
    top = -1
    if rem > 0:
        rho, top = numpy_fast_propagate(rho, precalc, rem)
    return rho, top


def _tb_left(rho, op, dim):
    return (np.asarray(op, dtype=LD) @ rho.reshape(dim, dim, order="F")).reshape(dim * dim, order="F")


def _tb_right(rho, op, dim):
    return (rho.reshape(dim, dim, order="F") @ np.asarray(op, dtype=LD)).reshape(dim * dim, order="F")


def _tb_trace(rho, dim):
    return np.trace(rho.reshape(dim, dim, order="F"))


def numpy_four_time_8op(dm_1, dm_2, rho_init, t1, precalc, dt, dim, ops8, early_only, late_t1_only, tb):
    """four_time_8op (:216-303); ops8 = (et1l, et1r, et2l, et2r, lt1l, lt1r, lt2l, lt2r)"""
    dm_1, dm_2, precalc = (np.asarray(a, dtype=LD) for a in (dm_1, dm_2, precalc))
    et1l, et1r, et2l, et2r, lt1l, lt1r, lt2l, lt2r = (np.asarray(o, dtype=LD) for o in ops8)
    n_t = len(t1)
    res = np.zeros((n_t, n_t), dtype=LD)
    tops = [-1]

    def prop(a, b, r, dm):
        r, top = numpy_propagate_tb(a, b, dt, r, dm, precalc)
        tops.append(top)
        return r
    for i in range(n_t):
        t1n = t1[i]
        rho_vec = prop(0.0, t1n, np.asarray(rho_init, dtype=LD), dm_1)
        for j in range(n_t - i):
            t2 = t1[i + j]
            r = _tb_left(_tb_right(rho_vec, et1r, dim), et1l, dim)
            r = prop(t1n, t2, r, dm_1)
            r = _tb_left(_tb_right(r, et2r, dim), et2l, dim)
            if early_only:
                res[i, i + j] = _tb_trace(r, dim)
                continue
            r = prop(t2, tb, r, dm_1)
            r = prop(0.0, t1n, r, dm_2)
            r = _tb_left(_tb_right(r, lt1r, dim), lt1l, dim)
            if late_t1_only:
                res[i, i + j] = _tb_trace(r, dim)
                continue
            r = prop(t1n, t2, r, dm_2)
            r = _tb_left(_tb_right(r, lt2r, dim), lt2l, dim)
            res[i, i + j] = _tb_trace(r, dim)
    return res, max(tops)


def numpy_four_time(dm_1, dm_2, rho_init, t1, precalc, dt, dim, ops4, tb):
    """four_time (:145-214): op_1, op_2 from the right in the early bin, op_3, op_4 from the left in the late one"""
    dm_1, dm_2, precalc = (np.asarray(a, dtype=LD) for a in (dm_1, dm_2, precalc))
    o1, o2, o3, o4 = (np.asarray(o, dtype=LD) for o in ops4)
    n_t = len(t1)
    res = np.zeros((n_t, n_t), dtype=LD)
    tops = [-1]

    def prop(a, b, r, dm):
        r, top = numpy_propagate_tb(a, b, dt, r, dm, precalc)
        tops.append(top)
        return r
    for i in range(n_t):
        t1n = t1[i]
        rho_vec = prop(0.0, t1n, np.asarray(rho_init, dtype=LD), dm_1)
        for j in range(n_t - i):
            t2 = t1[i + j]
            r = _tb_right(rho_vec, o1, dim)
            r = prop(t1n, t2, r, dm_1)
            r = _tb_right(r, o2, dim)
            r = prop(t2, tb, r, dm_1)
            r = prop(0.0, t1n, r, dm_2)
            r = _tb_left(r, o3, dim)
            r = prop(t1n, t2, r, dm_2)
            r = _tb_left(r, o4, dim)
            res[i, i + j] = _tb_trace(r, dim)
    return res, max(tops)


def numpy_dynamics_t1(dm_1, dm_2, rho_init, t1, precalc, dt, dim):
    """dynamics_t1 (:305-342): column 0 = rho_init, columns 1 .. n_t - 1 along t1 with dm_1, then n_t - 1 more
    along the same segments with dm_2, continuing from the last dm_1 column"""
    dm_1, dm_2, precalc = (np.asarray(a, dtype=LD) for a in (dm_1, dm_2, precalc))
    n_t = len(t1)
    res = np.zeros((dim * dim, 2 * n_t - 1), dtype=LD)
    res[:, 0] = np.asarray(rho_init, dtype=LD)
    top = -1
    for half, dm in enumerate((dm_1, dm_2)):
        for i in range(n_t - 1):
            k = i + half * (n_t - 1)
            res[:, k + 1], tp = numpy_propagate_tb(t1[i], t1[i + 1], dt, res[:, k], dm, precalc)
            top = max(top, tp)
    return res, top


def timebin_inputs(dim):
    """seeded inputs of the time-bin tests: 7 explicit maps per bin, 5 binary powers of one map, dt = 0.1, tb = 2.3,
    and per dim a sorted t1 grid sized so that the pair triangle leaves one pair in the last wave (dims 2-4), a ragged
    last wave (dim 5) or exercises 28 padding lanes (dim 6); see tests/test_timebin_oracle.py for the properties"""
    rng = np.random.default_rng(4200 + dim)
    N2 = dim * dim
    mk = lambda: np.eye(N2) + 0.05 * (rng.normal(size=(N2, N2)) + 1j * rng.normal(size=(N2, N2))) / dim  # noqa: E731
    F = lambda maps: np.asfortranarray(np.asarray(maps).transpose(1, 2, 0))  # noqa: E731
    n_map, n_precalc, dt, tb = 7, 5, 0.1, 2.3
    dm_1 = F([mk() for _ in range(n_map)])
    dm_2 = F([mk() for _ in range(n_map)])
    tl = mk()
    precalc = F([np.linalg.matrix_power(tl, 2 ** k) for k in range(n_precalc)])
    rho = random_rho(dim, seed=4300 + dim).reshape(N2, order="F")
    ops8 = [rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)) for _ in range(8)]
    t1 = {
        2: np.sort(np.concatenate([np.round(np.arange(27) * 0.1, 6), [0.25, 0.3, 0.65, 1.25, 1.25, 2.05]])),
        3: np.array([0.0, 0.1, 0.2, 0.25, 0.3, 0.3, 0.5, 0.6, 0.65, 0.7, 0.8, 1.2, 1.9, 2.3, 2.45]),
        4: np.array([0.0, 0.1, 0.25, 0.3, 0.3, 0.65, 0.9, 1.7, 2.6]),
        5: np.array([0.0, 0.25, 0.25, 0.6, 1.1, 2.5]),
        6: np.array([0.25, 0.25, 0.6, 1.1, 2.5]),
    }[dim]
    return dict(dm_1=dm_1, dm_2=dm_2, rho=rho, t1=t1, precalc=precalc, dt=dt, dim=dim, ops8=ops8, tb=tb,
                n_map=n_map, n_precalc=n_precalc)


def simple_traj(n_steps, mtos=(), n_traj=1, begins=None, ends=None):
    begins = np.zeros(n_traj, dtype=int) if begins is None else np.asarray(begins)
    ends = np.full(n_traj, n_steps) if ends is None else np.asarray(ends)
    return Trajectories(begins, ends, list(mtos))


def rabi_system(area_pi=1.0, tau=2.0, t0=10.0, gamma=0.0, dt=0.05, te=20.0):
    """resonant TLS driven by a unit-area Gaussian scaled to `area_pi` (units of pi): H = -pi hbar/2 (f s+ + h.c.)"""
    N = 2
    n_steps = int(round(te / dt))
    ds = dt / 4
    tt = ds * np.arange(4 * n_steps + 1)
    f = area_pi * np.exp(-0.5 * ((tt - t0) / tau) ** 2) / (np.sqrt(2 * np.pi) * tau)
    X = -0.5 * np.pi * hbar * ketbra(N, 1, 0)
    lind = [(gamma, ketbra(N, 0, 1))] if gamma else []
    return System(dim=2, H0=np.zeros((2, 2)), lindblad=lind, channels=[(X, f.astype(complex))], sample_t0=0.0,
                  sample_dt=ds), Grid(0.0, dt, n_steps, 1)


# ------------------------------------------------------------------ time-local maps: unit of error, inputs, restatement
# Shared by tests/golden/make_golden_tlmap_truth.py, tests/test_tlmap_truth_host.py and tests/test_gpu_tlmap_small.py.
EPS = float(np.finfo(np.float64).eps)
TL_MAX_SWEEPS = 40   # csrc/tlmap.hip


def tl_rel(got, ref):
    """max|got - ref| / max|ref|"""
    got, ref = np.asarray(got), np.asarray(ref)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def tl_kept(A, rcond):
    """numpy's float64 singular values of A (descending) and how many of them numpy's pinv keeps: s > rcond * max(s)"""
    s = np.linalg.svd(np.asarray(A, dtype=np.complex128), compute_uv=False)
    return s, int(np.count_nonzero(s > rcond * s[0]))


def tl_unit(A, E, T, rcond):
    """u = eps (|T|_2 |A|_2 + |E|_2) / s_min_kept / max|T|: the first-order change of T = E pinv(A, rcond), relative to
    its largest entry, under backward errors of size eps |A|_2 in A and eps |E|_2 in E. With dA and dE such errors and
    P = pinv(A), d(E P) = dE P - E P dA P on the kept subspace, and |P|_2 = 1 / s_min_kept, so
    |dT|_2 <= eps (|E|_2 + |T|_2 |A|_2) / s_min_kept. s_min_kept is the smallest singular value above rcond * s_max."""
    s, k = tl_kept(A, rcond)
    tmax = float(np.max(np.abs(T)))
    if k == 0 or tmax == 0.0:
        raise ValueError("no singular value kept, or a zero result: the unit is not defined")
    return EPS * (np.linalg.norm(T, 2) * s[0] + np.linalg.norm(E, 2)) / s[k - 1] / tmax


def tl_near_cut(A, rcond):
    """True when a singular value of A lies within 1 % of the cut rcond * s_max. A Jacobi singular value carries an
    absolute error of about eps * s_max, at the cut 1e-12 * s_max a relative one of about 2e-4: whether such a value is
    kept is not defined, and neither is the result. 1e-2 is 50 times that. numpy's float64 singular values."""
    s, _ = tl_kept(A, rcond)
    cut = rcond * s[0]
    return bool(cut > 0.0 and np.any(np.abs(s - cut) < 1e-2 * cut))


def tl_haar(rng, n):
    return np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))[0]


def tl_graded(rng, n, n_maps, cond=1e3, tail=None):
    """n_maps maps Q1 diag(s) Q2 with fresh Haar-like Q1, Q2 and s log-spaced from 1 to 1 / cond; `tail` replaces the
    last len(tail) singular values"""
    dm = np.empty((n_maps, n, n), dtype=np.complex128)
    for i in range(n_maps):
        s = np.logspace(0, -np.log10(cond), n)
        if tail is not None:
            s[n - len(tail):] = tail
        dm[i] = (tl_haar(rng, n) * s) @ tl_haar(rng, n)
    return dm


def tl_semigroup_chain(N, seed, n_maps=120, tau=0.5):
    """(T, dm): T = expm(tau L) and the cumulative maps dm[i] = T^(i+1) of a Lindblad semigroup on N levels (row-major
    vec, n = N^2). L has a random Hermitian Hamiltonian (normal entries, scaled by 0.5) and the N - 1 decay channels
    |k><k+1| of rate 1: one stationary state, every other mode decays, so the singular values of dm[i] fall
    exponentially, cross rcond * s_max one after another, and the kept rank goes from N^2 to 1."""
    rng = np.random.default_rng(seed)
    H = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    H = 0.25 * (H + H.conj().T)
    I = np.eye(N)
    L = -1j * (np.kron(H, I) - np.kron(I, H.T))
    for k in range(N - 1):
        Lk = ketbra(N, k, k + 1)
        LdL = Lk.conj().T @ Lk
        L = L + np.kron(Lk, Lk.conj()) - 0.5 * np.kron(LdL, I) - 0.5 * np.kron(I, LdL.T)
    T = sla.expm(tau * L)
    dm = np.empty((n_maps, N * N, N * N), dtype=np.complex128)
    dm[0] = T
    for i in range(1, n_maps):
        dm[i] = T @ dm[i - 1]
    return T, dm


def tl_rr_pairs(n):
    """the column pairs (p < q) of each round of tlmap.hip's round-robin tournament: m = n + (n & 1) players, player
    m - 1 fixed; round k, slot j pairs (k + j) mod (m - 1) with (k - j) mod (m - 1), slot 0 pairs k with m - 1. For odd
    n the player n is a dummy whose pairs are left out. One (ps, qs) index pair per round."""
    m = n + (n & 1)
    rounds = []
    for k in range(m - 1):
        ps, qs = [], []
        for j in range(m // 2):
            p, q = (k, m - 1) if j == 0 else ((k + j) % (m - 1), (k - j + (m - 1)) % (m - 1))
            p, q = min(p, q), max(p, q)
            if q < n:
                ps.append(p)
                qs.append(q)
        rounds.append((np.array(ps, dtype=int), np.array(qs, dtype=int)))
    return rounds


def tl_tol_factor(n):
    """csrc/tlmap.hip rotates a pair while |a_p^H a_q| > tl_tol_factor(n) eps |a_p| |a_q|"""
    return min(n, 4)


def _tl_fma(a, b, c):
    """fma(a, b, c) of float64 arrays: the product and the sum in long double (64-bit mantissa on x86), rounded once
    more to float64. Not the exact fused result, but like it the rounding error of a b survives when a b and c cancel,
    which a float64 product does not show."""
    return (np.asarray(a, dtype=np.longdouble) * b + c).astype(np.float64)


def _tl_rotate_fused(X, Y, c, s):
    """a_p' = c x - s y and a_q' = s x + c y as the kernel's instructions evaluate them: the compiler contracts each
    component to fma(x, c, -(y s)) and fma(x, s, y c). With x = y and c = s (equal columns) the plain float64 form
    gives an exact zero, the fused one the rounding error of a product, and the kernel goes on to orthogonalise such
    residue: a restatement without this expects too few sweeps of rank-deficient maps (6 for 10 at n = 9)."""
    xr, xi = np.asarray(X.real, dtype=np.longdouble), np.asarray(X.imag, dtype=np.longdouble)
    yr, yi = Y.real, Y.imag
    P = (xr * c - yr * s).astype(np.float64) + 1j * (xi * c - yi * s).astype(np.float64)
    Q = (xr * s + yr * c).astype(np.float64) + 1j * (xi * s + yi * c).astype(np.float64)
    return P, Q


def tl_jacobi_restated(dm, rcond, max_sweeps=TL_MAX_SWEEPS, dtype=np.complex128):
    """csrc/tlmap.hip in numpy, all maps of the chain at once: out[0] = dm[0], out[i] = dm[i] pinv(dm[i-1], rcond) by
    the kernel's one-sided Jacobi on the columns of dm[i-1] (same tournament, same rotation test
    |a_p^H a_q| > min(n, 4) eps |a_p| |a_q|, same rotation, same weights 1 / s_j^2 for s_j > rcond s_max), and the kernel's
    sweep count per map (sweeps[0] = 0): the sweeps run, the last of them without a rotation, or max_sweeps. Sums run
    in numpy's order, not the kernel's, and only the rotation of A is evaluated fused (_tl_rotate_fused: it decides
    the sweep count of rank-deficient maps): results agree with the kernel to rounding, not bit for bit. `dtype` np.clongdouble runs the same steps with that type's eps (for choosing test inputs, not used by a
    test). Returns (out, sweeps)."""
    dm = np.asarray(dm, dtype=dtype)
    n_maps, n = dm.shape[0], dm.shape[1]
    out = np.empty_like(dm)
    out[0] = dm[0]
    sweeps = np.zeros(n_maps, dtype=int)
    if n_maps < 2:
        return out, sweeps
    A = dm[:-1].copy()                                  # (B, n, n), columns A[:, :, j]
    V = np.broadcast_to(np.eye(n, dtype=dtype), A.shape).copy()
    tol = np.finfo(dm.real.dtype).eps * tl_tol_factor(n)
    rounds = tl_rr_pairs(n)
    live = np.arange(n_maps - 1)                        # the maps that rotated in their last sweep
    fused = np.dtype(dtype) == np.complex128
    with np.errstate(all="ignore"):
        for sweep in range(max_sweeps):
            Al, Vl = A[live], V[live]
            rotated = np.zeros(len(live), dtype=bool)
            for ps, qs in rounds:
                if len(ps) == 0:
                    continue
                X, Y = Al[:, :, ps], Al[:, :, qs]
                al = np.sum(X.real ** 2 + X.imag ** 2, axis=1)
                be = np.sum(Y.real ** 2 + Y.imag ** 2, axis=1)
                g = np.sum(X.conj() * Y, axis=1)
                ga = np.hypot(g.real, g.imag)
                act = (ga > tol * np.sqrt(al) * np.sqrt(be)) & (ga > 0.0)
                if not act.any():
                    continue
                rotated |= act.any(axis=1)
                gs = np.where(act, ga, 1.0)
                zeta = (be - al) / (2.0 * gs)
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = np.where(act, 1.0 / np.sqrt(1.0 + t * t), 1.0)
                s = np.where(act, c * t, 0.0)
                ph = np.where(act, g.conj() / gs, 1.0)  # e^{-i phi}, phi = arg(a_p^H a_q)
                c, s, ph = c[:, None, :], s[:, None, :], ph[:, None, :]
                Y = ph * Y
                if fused:   # on A, which decides the rotations; V only enters the result
                    Al[:, :, ps], Al[:, :, qs] = _tl_rotate_fused(X, Y, c, s)
                else:
                    Al[:, :, ps], Al[:, :, qs] = c * X - s * Y, s * X + c * Y
                X, Y = Vl[:, :, ps], ph * Vl[:, :, qs]
                Vl[:, :, ps], Vl[:, :, qs] = c * X - s * Y, s * X + c * Y
            A[live], V[live] = Al, Vl
            sweeps[1 + live] = sweep + 1
            live = live[rotated]                        # a sweep without a rotation ends a map's loop
            if len(live) == 0:
                break
        w2 = np.sum(A.real ** 2 + A.imag ** 2, axis=1)  # (B, n): s_j^2
        smax = np.sqrt(np.max(w2, axis=1, initial=0.0))
        w = np.where(np.sqrt(w2) > rcond * smax[:, None], 1.0 / w2, 0.0)
        Bm = (dm[1:] @ V) * w[:, None, :]
        out[1:] = Bm @ A.conj().transpose(0, 2, 1)
    return out, sweeps
