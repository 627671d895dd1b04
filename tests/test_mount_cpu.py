"""Host side of the per-instance base mount and gravity: the header constants
and symbols, the row packer against the documented layout, robot.Mount's three
constructors and their validation, the host kinematics and gravity torque under
a mount against the nominal ones and the numpy oracle, and the argument checks
of DeviceFleetLoop and run_sweep.  No device."""
from __future__ import annotations

import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import oracle.panda as OP
from ffddp import _abi
from ffddp import fleet as FL
from ffddp import plant as PL
from ffddp import robot as R
from ffddp.config import mount_rows
from ffddp.controller import classical_benchmark_config
from ffddp.fleet_loop import DeviceFleetLoop
from ffddp.trajectory import benchmark_traj

ROOT = Path(__file__).resolve().parents[1]

NEW_SYMBOLS = ("ffddp_solve_batch_mnt_dev", "ffddp_calc_diff_mnt", "ffddp_mount_rows", "ffddp_gravity_torque_mnt_dev",
               "ffddp_fleet_pre_mnt_dev", "ffddp_fleet_obs_frame_dev")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]),
            "y": np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]),
            "z": np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])}[axis]


def _seeded_q(n=5):
    rng = np.random.default_rng(23)
    return R.Q_NEUTRAL[None] + rng.uniform(-0.5, 0.5, (n, 7))


def test_header_constants_and_symbols():
    text = (ROOT / "include" / "ffddp.h").read_text()
    m = re.search(r"#define FFDDP_MOUNT_W (\d+)", text)
    assert m and int(m.group(1)) == _abi.MOUNT_W == 16
    m = re.search(r"#define FFDDP_FRAME_W (\d+)", text)
    assert m and int(m.group(1)) == _abi.FRAME_W == 12
    lib = _abi.load()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.SYMBOLS and re.search(r"\bint %s\(" % sym, text), sym
        assert getattr(lib, sym).argtypes is not None, sym


def test_rows_of_the_nominal_mount_are_the_robot_constants():
    rows = mount_rows([R.Mount(), None])
    assert rows.shape == (2, _abi.MOUNT_W) and rows.dtype == np.float64
    assert np.array_equal(rows[0], rows[1])
    r = rows[0]
    assert np.array_equal(_bits(r[0:9]), _bits(R.JOINT_R[0].reshape(9)))  # row-major
    assert np.array_equal(_bits(r[9:12]), _bits(R.JOINT_P[0]))
    assert np.array_equal(_bits(r[12:15]), _bits(R.GRAVITY))
    assert r[15] == 0.0
    # row-major: an asymmetric rotation is packed as given
    m = R.Mount.remounted(_rot("x", 20.0), [0.05, -0.03, 0.02])
    got = mount_rows([m])[0]
    assert np.array_equal(got[0:9], m.base_R.reshape(9)) and got[5] == m.base_R[1, 2] != m.base_R[2, 1]
    assert np.array_equal(got[9:12], m.base_p) and np.array_equal(got[12:15], R.GRAVITY) and got[15] == 0.0
    assert mount_rows([]).shape == (0, _abi.MOUNT_W)


def test_builder_errors():
    lib = _abi.load()
    out = np.zeros((2, _abi.MOUNT_W))
    good = _abi.make_robot()

    def c_builder(rb):
        robots = (_abi.Robot * 2)(good, rb)
        return lib.ffddp_mount_rows(robots, 2, _abi.dptr(out))

    assert c_builder(_abi.make_robot(mount=R.Mount.table_tilt(10.0))) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for field, idx in (("joint_R", 4), ("joint_p", 2), ("gravity", 1)):
            rb = _abi.make_robot()
            arr = getattr(rb, field)
            (arr[0] if field != "gravity" else arr)[idx] = bad
            assert c_builder(rb) == -1, (field, bad)
    assert lib.ffddp_mount_rows(None, 2, _abi.dptr(out)) == -1
    assert lib.ffddp_mount_rows((_abi.Robot * 2)(good, good), 2, None) == -1
    assert lib.ffddp_mount_rows((_abi.Robot * 2)(good, good), -1, _abi.dptr(out)) == -1
    assert lib.ffddp_mount_rows(None, 0, None) == 0  # B == 0: nothing read or written, as the header states


def test_mount_validation():
    with pytest.raises(ValueError, match="rotation"):
        R.Mount(base_R=np.eye(3) * 1.001)
    with pytest.raises(ValueError, match="rotation"):
        R.Mount(base_R=np.diag([1.0, 1.0, -1.0]))  # a reflection
    skew = _rot("z", 12.0)
    skew[0, 1] += 1.0e-6
    for ctor in (R.Mount.in_frame, R.Mount.remounted):
        with pytest.raises(ValueError, match="rotation"):
            ctor(skew, np.zeros(3))
        with pytest.raises(ValueError, match="finite"):
            ctor(np.eye(3), [0.0, np.nan, 0.0])
        with pytest.raises(ValueError, match="finite"):
            ctor(np.full((3, 3), np.inf), np.zeros(3))
        with pytest.raises(ValueError):
            ctor(np.eye(4), np.zeros(3))
    with pytest.raises(ValueError, match="finite"):
        R.Mount(gravity=[0.0, 0.0, np.inf])
    with pytest.raises(ValueError, match="finite"):
        R.Mount(base_p=[0.0, np.nan, 0.0])
    # within 1e-9 of a rotation is accepted
    ok = _rot("z", 12.0)
    ok[0, 1] += 1.0e-11
    R.Mount.in_frame(ok, np.zeros(3))
    # the three constructors
    m = R.Mount()
    assert np.array_equal(m.base_R, R.JOINT_R[0]) and np.array_equal(m.base_p, R.JOINT_P[0])
    assert np.array_equal(m.gravity, R.GRAVITY) and m.frame is None
    assert np.array_equal(m.obs_frame(), np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    Rf, pf = _rot("x", -8.0), np.array([0.03, 0.0, 0.0])
    f = R.Mount.in_frame(Rf, pf)
    assert np.allclose(f.base_R, Rf.T @ R.JOINT_R[0], rtol=0, atol=1e-16)
    assert np.allclose(f.base_p, Rf.T @ (R.JOINT_P[0] - pf), rtol=0, atol=1e-16)
    assert np.allclose(f.gravity, Rf.T @ R.GRAVITY, rtol=0, atol=1e-15)
    assert np.array_equal(f.frame[0], Rf) and np.array_equal(f.frame[1], pf)
    D = R.R_MJ_FROM_PIN
    assert np.allclose(f.obs_frame(), np.concatenate([(D @ Rf @ D).reshape(9), D @ pf]), rtol=0, atol=1e-16)
    w = R.Mount.remounted(Rf, pf)
    assert w.frame is None and np.array_equal(w.gravity, R.GRAVITY)
    assert np.allclose(w.base_R, Rf @ R.JOINT_R[0], rtol=0, atol=1e-16)
    assert np.allclose(w.base_p, Rf @ R.JOINT_P[0] + pf, rtol=0, atol=1e-16)
    assert R.Mount.table_tilt(0.0).frame is not None
    assert np.allclose(mount_rows([R.Mount.table_tilt(0.0)]), mount_rows([None]), rtol=0, atol=1e-16)


@pytest.mark.parametrize("tilt", [5.0, 10.0, 15.0])
def test_table_tilt_mount_is_the_same_arm_seen_from_the_table(tilt):
    m = R.Mount.table_tilt(tilt)
    Rf, pf = m.frame
    rb = _abi.make_robot(mount=m)
    q = _seeded_q()
    # the gravity torque does not depend on the frame it is computed in
    assert np.max(np.abs(_abi.gravity_torque(q, rb) - _abi.gravity_torque(q))) < 1e-12
    assert np.max(np.abs(_abi.gravity_torque(q))) > 1.0
    # the EE pose is the nominal one re-expressed
    for b in range(q.shape[0]):
        Rn, pn = _abi.frame_placement(q[b])
        Rm, pm = _abi.frame_placement(q[b], rb)
        assert np.max(np.abs(pm - Rf.T @ (pn - pf))) < 1e-12
        assert np.max(np.abs(Rm - Rf.T @ Rn)) < 1e-12
        assert np.max(np.abs(pm - pn)) > 1e-3  # and it moved
    # the tilted table is the flat table in the mount's frame
    fr = m.obs_frame()
    Rmj, pmj = fr[:9].reshape(3, 3), fr[9:]
    n, pt = PL.table_plane(tilt)
    n0, pt0 = PL.table_plane(0.0)
    assert np.max(np.abs(Rmj.T @ n - np.array([0.0, 0.0, 1.0]))) < 1e-12
    assert abs((Rmj.T @ (pt - pmj))[2] - pt0[2]) < 1e-12
    assert np.max(np.abs(Rmj.T @ (pt - pmj) - pt0)) < 1e-12
    assert np.array_equal(n0, [0.0, 0.0, 1.0])


def _oracle_patched(monkeypatch_ctx, m):
    JR, JP = OP.JOINT_PLACEMENT_R.copy(), OP.JOINT_PLACEMENT_P.copy()
    JR[0], JP[0] = m.base_R, m.base_p
    monkeypatch_ctx.setattr(OP, "JOINT_PLACEMENT_R", JR)
    monkeypatch_ctx.setattr(OP, "JOINT_PLACEMENT_P", JP)
    monkeypatch_ctx.setattr(OP, "GRAVITY", m.gravity.copy())


def test_gravity_torque_equals_the_oracle_under_the_patched_mount(monkeypatch):
    q = _seeded_q()
    nominal = OP.gravity_torque(q)
    for m, moves in ((R.Mount.remounted(_rot("x", 20.0), np.zeros(3)), True),
                     (R.Mount.remounted(np.eye(3), [0.05, -0.03, 0.02]), False),
                     (R.Mount.in_frame(_rot("x", -8.0), [0.03, 0.0, 0.0]), False),
                     (R.Mount.table_tilt(15.0), False)):
        got = _abi.gravity_torque(q, _abi.make_robot(mount=m))
        with monkeypatch.context() as mpc:
            _oracle_patched(mpc, m)
            want = OP.gravity_torque(q)
        assert np.max(np.abs(got - want)) < 1e-12
        # a re-mount with the world's gravity kept changes the load; a change of frame or a translation does not
        d = np.max(np.abs(got - nominal))
        assert (d > 1.0) if moves else (d < 1e-12), d
    assert np.array_equal(OP.gravity_torque(q), nominal)  # the patch is gone


def test_loop_argument_is_checked_before_the_device():
    traj, _ = benchmark_traj(np.array([-0.4, 0.05, 0.55]))
    cfg = classical_benchmark_config(0.005, 0.3)
    q0 = np.tile(R.Q_NEUTRAL, (2, 1))
    with pytest.raises(ValueError, match="mounts"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, mounts=[R.Mount.table_tilt(5.0)])
    with pytest.raises(ValueError, match="mounts"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, mounts=[R.Mount.table_tilt(5.0), 1.0])
    with pytest.raises(ValueError, match="frame"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4,
                        mounts=[None, R.Mount.remounted(_rot("x", 20.0), np.zeros(3))])
    with pytest.raises(ValueError, match="frame"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, mounts=[R.Mount(), None])


def test_run_sweep_tilt_known_arguments():
    kw = dict(seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(NotImplementedError, match="device_loop"):
        FL.run_sweep(tilt_known=True, **kw)
    for bad in (2, "yes", 0.5):
        with pytest.raises(ValueError, match="tilt_known"):
            FL.run_sweep(tilt_known=bad, device_loop=True, **kw)


def test_sweep_tool_tilt_known_option(capsys):
    spec = importlib.util.spec_from_file_location("sweep_c4_tool_mnt", ROOT / "tools" / "sweep_c4.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args(["--device-loop", "1", "--tilt-known", "1"]).tilt_known == 1
    assert ap.parse_args([]).tilt_known == 0
    with pytest.raises(SystemExit):
        ap.parse_args(["--tilt-known", "2"])
    capsys.readouterr()
