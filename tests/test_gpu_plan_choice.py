"""The decisions plan creation takes (pqd_plan_describe), pinned per shape and environment. GPU only; nothing executes.

Path, workgroup shape, split chunks, multi-trajectory grouping, quad strips, trunks, windows and the A/B switches set
the speed of a plan, not its results, so the parity tests cannot see them change. Each case constructs an engine.Plan
and compares Plan.describe() with the line recorded under its id in tests/golden/plan_choice.json (for a plan whose
creation fails: the error code and message). The decisions depend on the device's CU count, which the file records; on
a device with another count the cases skip. PQD_RECORD_PLAN_CHOICE=1 writes the file instead of comparing: it was
recorded once, before plan creation was split into stages, and is not regenerated.

Trajectory kinds: "g2e" is the two-time sweep (MTO pair of kinds 2 and 1 after step t1 = t mod 100, window
[t1, t1 + 300]); "g2l" has t1 spread over [100, 200] and windows of 200 steps, so that shared trunks would save more
than a quarter of all steps; "mixed" is test_gpu_msplit.mixed_trajectories; "many" puts 40 MTO steps on every
trajectory; "plain" has none.
"""
import json
import os

import numpy as np
import pytest

from pyaceqd_amd import engine, pt as ptmod
from pyaceqd_amd.engine import MTO, Grid, Trajectories
from tests import helpers as H
from tests.test_gpu_msplit import mixed_trajectories

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_choice.json")
RECORD = os.environ.get("PQD_RECORD_PLAN_CHOICE") == "1"
KEEP_ENV = ("PQD_LIB", "PQD_DEVICE", "PQD_TORCH_FIRST", "PQD_RECORD_PLAN_CHOICE")


def case(N, chi, n_traj, kind="g2e", n_out=1, n_sys=1, n_steps=None, **env):
    return dict(N=N, chi=chi, n_traj=n_traj, kind=kind, n_out=n_out, n_sys=n_sys, n_steps=n_steps), env


def variants(prefix, shape, envs):
    return {f"{prefix}-{'-'.join(f'{k[4:]}{v}' for k, v in e.items()) or 'default'}": case(*shape[0], **shape[1], **e)
            for e in envs}


C4 = ((4, 64, 20), {})  # N = 4, chi = 64, two-time sweep
CASES = {
    # no PT
    **variants("nopt-N3-10", ((3, 0, 10), {}), [{}, {"PQD_WIN": "0"}, {"PQD_WIN": "2"}, {"PQD_IDLE": "0"}]),
    # quads
    "quad-chi16-8": case(2, 16, 8),
    "quad-chi16-1100": case(2, 16, 1100),
    "quad-chi32-8": case(2, 32, 8),
    "quad-chi32-1100": case(2, 32, 1100),
    **variants("quad-chi64-8", ((2, 64, 8), {}),
               [{}, {"PQD_QUAD": "2"}, {"PQD_QUAD": "0"}, {"PQD_QPW": "1"}, {"PQD_QCG": "2"}, {"PQD_QPRIO": "0"},
                {"PQD_QUAD": "2", "PQD_QPW": "1"}, {"PQD_QUAD": "2", "PQD_QCG": "2"},
                {"PQD_QUAD": "2", "PQD_QPRIO": "0"}]),
    "quad-chi32-1100-QCG1": case(2, 32, 1100, PQD_QCG="1"),
    "quad-chi32-1100-QPW2": case(2, 32, 1100, PQD_QPW="2"),
    "quad-chi16-1100-QCG2": case(2, 16, 1100, PQD_QCG="2"),
    "quad-chi32-4-SPLIT2": case(2, 32, 4, PQD_SPLIT="2"),
    # single-trajectory split groups
    "split-N3-chi32-1": case(3, 32, 1),
    "split-N5-chi32-1": case(5, 32, 1),
    "split-N6-chi32-1": case(6, 32, 1),
    "split-N4-chi64-1": case(4, 64, 1),
    **variants("split-N4-chi64-15", ((4, 64, 15), {"kind": "mixed"}),
               [{}, {"PQD_SPLIT": "0"}, {"PQD_SPLIT_OW": "0"}, {"PQD_SPLIT_GRAN": "1"}, {"PQD_SPLIT_L2": "0"}]),
    "split-N4-chi64-16-SPLIT_OW0": case(4, 64, 16, kind="mixed", PQD_SPLIT_OW="0"),
    # several launches of them, where the multi-trajectory groups are unsupported
    "split-N5-chi64-20": case(5, 64, 20),
    "split-N5-chi64-37": case(5, 64, 37),
    "split-N4-chi16-20": case(4, 16, 20),
    "split-N4-chi16-31": case(4, 16, 31),
    "split-N4-chi64-20-nout9": case(4, 64, 20, n_out=9),
    # multi-trajectory split groups
    **{f"msplit-N4-chi64-{n}": case(4, 64, n) for n in (16, 20, 32, 100, 512, 600)},
    **variants("msplit-N4-chi64-20", C4,
               [{"PQD_MSPLIT": "0"}, {"PQD_MS_TB": "5"}, {"PQD_SPLIT_XCD": "0"}, {"PQD_MS_L2": "0"},
                {"PQD_MS_PTM": "0"}, {"PQD_TRUNK": "1"}, {"PQD_FUSE": "0"}]),
    "msplit-N4-chi64-100-MS_PTM0": case(4, 64, 100, PQD_MS_PTM="0"),
    "msplit-N4-chi64-8-MSPLIT2": case(4, 64, 8, PQD_MSPLIT="2"),
    "msplit-N4-chi64-20-g2l": case(4, 64, 20, kind="g2l"),
    "msplit-N4-chi64-20-many-MS_TB16": case(4, 64, 20, kind="many", n_steps=100, PQD_MS_TB="16"),
    "msplit-N3-chi32-40": case(3, 32, 40),
    "msplit-N6-chi32-64": case(6, 32, 64),
    "msplit-N6-chi32-128": case(6, 32, 128),
    "msplit-N4-chi128-20": case(4, 128, 20),
    "msplit-N2-chi256-8": case(2, 256, 8),
    "msplit-N4-chi256-8": case(4, 256, 8),
    "msplit-N4-chi256-600": case(4, 256, 600),
    # batched lock-step sweep
    **variants("batched-N4-chi64-2048", ((4, 64, 2048), {}),
               [{}, {"PQD_SWEEP_LEAN": "0"}, {"PQD_BT": "4"}, {"PQD_PT_MODE": "1"}, {"PQD_CMUL3": "0"},
                {"PQD_TRPRE": "0"}, {"PQD_ROWPAIR": "0"}, {"PQD_UNITBAL": "0"}, {"PQD_ABLATE": "1"}]),
    "batched-N6-chi64-300": case(6, 64, 300),
    "batched-N3-chi128-600": case(3, 128, 600),
    # (400 trajectories: up to 304, 19 resident groups of 16, the multi-trajectory split groups take this shape)
    "batched-N5-chi32-400-COLBIG0": case(5, 32, 400, PQD_COLBIG="0"),
    # trunk pre-pass
    **variants("trunk-N4-chi64-2048-g2l", ((4, 64, 2048), {"kind": "g2l"}),
               [{"PQD_TRUNK": "-1"}, {"PQD_TRUNK": "0"}, {"PQD_TRUNK": "1"}, {"PQD_BRANCH": "0"}]),
    "trunk-N6-chi32-300-g2l-3sys": case(6, 32, 300, kind="g2l", n_sys=3),
    "trunk-N2-chi16-300-g2l": case(2, 16, 300, kind="g2l"),
    # empty
    "empty-ntraj0": case(4, 64, 0),
    "empty-nsteps0": case(4, 64, 3, kind="plain", n_steps=0),
}

_systems, _pts, _n_cu = {}, {}, []


def trajectories(N, n_traj, kind, n_steps):
    """(n_steps, Trajectories) of a kind; the MTO operators are fixed matrices (identical pairs share a superoperator)"""
    A, Cm = H.ketbra(N, 0, 1), H.ketbra(N, 1, 0)
    if kind == "mixed":
        n_steps = 40 if n_steps is None else n_steps
        return n_steps, mixed_trajectories(n_steps, N, n_traj, seed=N + n_traj)
    if kind == "plain":
        return n_steps, Trajectories(np.zeros(n_traj, dtype=int), np.full(n_traj, n_steps), [])
    if kind == "many":
        mt = [MTO(t, 2 * k + t % 2, False, 0, A + Cm) for t in range(n_traj) for k in range(40)]
        return n_steps, Trajectories(np.zeros(n_traj, dtype=int), np.full(n_traj, n_steps), mt)
    if kind == "g2e":
        n_steps, n_tau = 399, 300
        t1 = np.arange(n_traj) % 100
    else:
        n_steps, n_tau = 400, 200
        t1 = 100 + (np.arange(n_traj) * 100) // max(1, n_traj - 1)
    mt = []
    for t in range(n_traj):
        mt += [MTO(t, int(t1[t]), False, 2, A), MTO(t, int(t1[t]), False, 1, Cm)]
    return n_steps, Trajectories(t1.astype(int), (t1 + n_tau).astype(int), mt)


def build_plan(N, chi, n_traj, kind, n_out, n_sys, n_steps):
    n_steps, tr = trajectories(N, n_traj, kind, n_steps)
    if n_sys > 1:
        tr.system = np.arange(n_traj) % n_sys
    if (N, n_sys) not in _systems:
        _systems[N, n_sys] = [H.random_system(N, n_steps=400, seed=20 + k)[0] for k in range(n_sys)]
    if chi and (N, chi) not in _pts:
        _pts[N, chi] = ptmod.random_pt(N, chi, D=2, n_slices=2, seed=N + chi, eps=0.1)
    systems = _systems[N, n_sys]
    ops = [H.ketbra(N, k % N, (k // N) % N) for k in range(n_out)]
    return engine.Plan(systems if n_sys > 1 else systems[0], Grid(0.0, 0.1, n_steps), H.random_rho(N), ops, tr,
                       pt=_pts[N, chi] if chi else None)


def describe_line(shape):
    try:
        return " ".join(f"{k}={v}" for k, v in build_plan(**shape).describe().items())
    except (ValueError, engine._lib.PQDError) as e:
        return f"error {getattr(e, 'code', None)}: {e}"


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_plan_choice(monkeypatch, cid):
    shape, env = CASES[cid]
    for k in list(os.environ):
        if k.startswith("PQD_") and k not in KEEP_ENV:
            monkeypatch.delenv(k)
    if not _n_cu:
        _n_cu.append(int(build_plan(3, 0, 1, "plain", 1, 1, 4).describe()["n_cu"]))
    n_cu = _n_cu[0]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    line = describe_line(shape)
    print(f"{cid}: {line}")
    if RECORD:
        rec = golden() if os.path.exists(GOLDEN) else {"n_cu": n_cu, "cases": {}}
        assert rec["n_cu"] == n_cu
        rec["cases"][cid] = line
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    rec = golden()
    if rec["n_cu"] != n_cu:
        pytest.skip(f"the decisions were recorded on a device with {rec['n_cu']} CUs, this one has {n_cu}")
    assert line == rec["cases"][cid]


@pytest.mark.gpu
def test_describe_argument_checks():
    """a buffer one byte short of the line and its NUL, and a NULL buffer, are PQD_ERR_ARG; the exact length fits"""
    import ctypes as C
    plan = build_plan(3, 0, 1, "plain", 1, 1, 4)
    L = engine._lib.lib()
    line = " ".join(f"{k}={v}" for k, v in plan.describe().items())
    buf = C.create_string_buffer(len(line) + 1)
    assert L.pqd_plan_describe(plan.handle, buf, len(line) + 1) == 0 and buf.value.decode() == line
    assert L.pqd_plan_describe(plan.handle, buf, len(line)) == 1
    assert L.pqd_plan_describe(plan.handle, None, 64) == 1


@pytest.mark.gpu
def test_unit_balance_switch_reaches_the_row_units(monkeypatch):
    """PQD_UNITBAL=0 deals whole row units to the least-loaded wave. At N = 6 (36 PT rows over two slices: units of up
    to four rows that do not divide evenly among the waves) that is another unit list than the balanced one, and
    nothing else about the plan changes. In the table's N = 4 case (16 rows in units of two on 8 waves) both lists agree."""
    shape = dict(N=6, chi=64, n_traj=300, kind="g2e", n_out=1, n_sys=1, n_steps=None)
    for k in list(os.environ):
        if k.startswith("PQD_") and k not in KEEP_ENV:
            monkeypatch.delenv(k)
    balanced = build_plan(**shape).describe()
    monkeypatch.setenv("PQD_UNITBAL", "0")
    whole = build_plan(**shape).describe()
    print(f"units balanced {balanced['units']} umax {balanced['umax']}, whole {whole['units']} umax {whole['umax']}")
    assert whole["units"] != balanced["units"]
    skip = ("units", "umax", "tk_umax")
    assert {k: v for k, v in whole.items() if k not in skip} == {k: v for k, v in balanced.items() if k not in skip}


def test_recording_reaches_every_branch():
    """conditions on the recorded shapes (no GPU): every path, both workgroup sizes, and both values of each of the
    decisions the parity tests cannot see"""
    rec = golden()["cases"]
    assert set(rec) == set(CASES)
    plans = [dict(kv.split("=", 1) for kv in line.split()) for line in rec.values() if not line.startswith("error")]
    seen = lambda key: {p[key] for p in plans}  # noqa: E731
    assert seen("path") == {"0", "1", "2", "3", "4"}
    assert seen("BT") >= {"4", "8"}
    assert seen("qcg") >= {"2", "4"}
    for key in ("tk_split", "win", "lean"):
        assert seen(key) == {"0", "1"}, key
    for key in ("split_chunk", "ms_xcd", "n_trunk"):
        assert "0" in seen(key) and len(seen(key)) > 1, key
