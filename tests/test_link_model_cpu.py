"""Host side of the per-instance link models: the header constant and symbols,
the row packer against the documented layout, LinkModel's payload algebra, the
gravity torque of a payload against the frame Jacobian and the numpy oracle,
and run_sweep's argument and draw.  No device."""
from __future__ import annotations

import ctypes as C
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import oracle.panda as OP
from ffddp import _abi
from ffddp import fleet as FL
from ffddp import robot as R
from ffddp.config import link_model_rows
from ffddp.controller import classical_benchmark_config
from ffddp.fleet_loop import DeviceFleetLoop
from ffddp.trajectory import benchmark_traj

ROOT = Path(__file__).resolve().parents[1]

NEW_SYMBOLS = ("ffddp_solve_batch_mdl_dev", "ffddp_calc_diff_mdl", "ffddp_link_model_rows",
               "ffddp_gravity_torque_mdl_dev", "ffddp_fleet_pre_mdl_dev")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_header_constant_and_symbols():
    text = (ROOT / "include" / "ffddp.h").read_text()
    m = re.search(r"#define FFDDP_LINK_W (\d+)", text)
    assert m and int(m.group(1)) == _abi.LINK_W == 128
    lib = _abi.load()
    for sym in NEW_SYMBOLS:
        assert sym in _abi.SYMBOLS and re.search(r"\bint %s\(" % sym, text), sym
        assert getattr(lib, sym).argtypes is not None, sym


def test_rows_of_the_nominal_model_are_the_robot_constants():
    rows = link_model_rows([R.LinkModel(), None])
    assert rows.shape == (2, _abi.LINK_W) and rows.dtype == np.float64
    assert np.array_equal(rows[0], rows[1])
    r = rows[0]
    used = np.zeros(_abi.LINK_W, bool)
    for j in range(7):
        assert _bits(r[16 * j]) == _bits(R.MASS[j])
        assert np.array_equal(_bits(r[16 * j + 1:16 * j + 4]), _bits(R.COM[j]))
        assert np.array_equal(_bits(r[16 * j + 4:16 * j + 13]), _bits(R.INERTIA[j].reshape(9)))  # row-major
        used[16 * j:16 * j + 13] = True
    assert not r[~used].any() and (~used).sum() == 128 - 7 * 13
    # all nine inertia entries travel: an asymmetric matrix is packed as given
    I = R.INERTIA.copy()
    I[2, 0, 1] += 1.0e-3
    got = link_model_rows([R.LinkModel(inertia=I)])[0]
    assert got[16 * 2 + 4 + 1] == I[2, 0, 1] and got[16 * 2 + 4 + 3] == I[2, 1, 0] != I[2, 0, 1]
    assert link_model_rows([]).shape == (0, _abi.LINK_W)


def test_builder_errors():
    lib = _abi.load()
    out = np.zeros((2, _abi.LINK_W))

    def c_builder(models):
        robots = (_abi.Robot * 2)(*[_abi.make_robot(m) for m in models])
        return lib.ffddp_link_model_rows(robots, 2, _abi.dptr(out))

    assert c_builder([R.LinkModel(), R.LinkModel()]) == 0
    for bad in (0.0, -1.0, np.nan, np.inf):
        mass = R.MASS.copy()
        mass[4] = bad
        m = R.LinkModel(mass=mass)
        with pytest.raises(ValueError, match="finite"):
            link_model_rows([R.LinkModel(), m])
        assert c_builder([R.LinkModel(), m]) == -1
    for bad in (np.nan, -np.inf):
        com, I = R.COM.copy(), R.INERTIA.copy()
        com[6, 1] = bad
        I[0, 2, 1] = bad
        for m in (R.LinkModel(com=com), R.LinkModel(inertia=I)):
            with pytest.raises(ValueError, match="finite"):
                link_model_rows([m, R.LinkModel()])
            assert c_builder([m, R.LinkModel()]) == -1
    assert lib.ffddp_link_model_rows(None, 2, _abi.dptr(out)) == -1
    with pytest.raises(ValueError, match="LinkModel"):
        R.LinkModel(mass=np.ones(6))


def test_with_payload_and_scaled():
    base = R.LinkModel()
    mp, cp = 2.0, np.array([0.03, -0.02, 0.15])
    Ip = np.array([[4.0e-3, 3.0e-4, -2.0e-4], [3.0e-4, 5.0e-3, 1.0e-4], [-2.0e-4, 1.0e-4, 3.0e-3]])
    m = base.with_payload(mp, cp, Ip)
    # only link 7 changed; the argument was not touched
    assert np.array_equal(base.mass, R.MASS) and np.array_equal(m.mass[:6], R.MASS[:6])
    assert np.array_equal(m.com[:6], R.COM[:6]) and np.array_equal(m.inertia[:6], R.INERTIA[:6])
    # total mass and first moment
    assert m.mass[6] == R.MASS[6] + mp
    assert np.allclose(m.mass[6] * m.com[6], R.MASS[6] * R.COM[6] + mp * cp, rtol=0, atol=1e-15)
    # symmetric, positive definite, and the second moment about the link origin is the sum of the parts'
    I = m.inertia[6]
    assert np.allclose(I, I.T, rtol=0, atol=1e-18) and np.all(np.linalg.eigvalsh(I) > 0.0)
    about0 = lambda mass, c, Ic: Ic + mass * R._spread(c)  # noqa: E731
    assert np.allclose(about0(m.mass[6], m.com[6], I), about0(R.MASS[6], R.COM[6], R.INERTIA[6]) + about0(mp, cp, Ip),
                       rtol=0, atol=1e-15)
    # a zero-size point payload at the link's own com changes only the mass
    p = base.with_payload(0.7, R.COM[6])
    assert p.mass[6] == R.MASS[6] + 0.7
    assert np.allclose(p.com[6], R.COM[6], rtol=0, atol=1e-17) and np.allclose(p.inertia[6], R.INERTIA[6], rtol=0, atol=1e-17)
    # the default payload position is the EE offset
    assert np.array_equal(base.with_payload(0.5).com, base.with_payload(0.5, R.EE_P).com)
    # scaled: per-link factors, inertia with the mass, com kept
    f = np.array([0.8, 0.9, 1.1, 1.2, 0.85, 1.15, 1.05])
    s = base.scaled(f)
    assert np.array_equal(s.mass, R.MASS * f) and np.array_equal(s.com, R.COM)
    assert np.array_equal(s.inertia, R.INERTIA * f[:, None, None])
    assert np.array_equal(base.scaled(1.1).mass, R.MASS * 1.1)
    with pytest.raises(ValueError):
        base.scaled(0.0)
    with pytest.raises(ValueError):
        base.with_payload(-1.0)


def _seeded_q(n=5):
    rng = np.random.default_rng(21)
    return R.Q_NEUTRAL[None] + rng.uniform(-0.5, 0.5, (n, 7))


def test_gravity_torque_of_a_point_payload_is_the_jacobian_transpose_of_its_weight():
    mp = 0.5
    model = R.LinkModel().with_payload(mp, R.EE_P)
    q = _seeded_q()
    g_nom = _abi.gravity_torque(q)
    g_pay = _abi.gravity_torque(q, _abi.make_robot(model))
    assert np.array_equal(g_nom, _abi.gravity_torque(q, _abi.robot_struct()))
    for b in range(q.shape[0]):
        J, _, _ = OP.frame_jacobian_lwa(q[b])
        want = J[:3].T @ np.array([0.0, 0.0, 9.81 * mp])
        assert np.max(np.abs((g_pay[b] - g_nom[b]) - want)) < 1e-12, b
        assert np.max(np.abs(want)) > 0.05  # the load the GPU tests rely on


def test_gravity_torque_equals_the_oracle_under_the_patched_model(monkeypatch):
    Ip = np.array([[4.0e-3, 3.0e-4, -2.0e-4], [3.0e-4, 5.0e-3, 1.0e-4], [-2.0e-4, 1.0e-4, 3.0e-3]])
    q = _seeded_q()
    for model in (R.LinkModel().with_payload(0.5, R.EE_P), R.LinkModel().with_payload(2.0, [0.03, -0.02, 0.15], Ip),
                  R.LinkModel().scaled([0.8, 0.9, 1.1, 1.2, 0.85, 1.15, 1.05])):
        got = _abi.gravity_torque(q, _abi.make_robot(model))
        with monkeypatch.context() as mpc:
            mpc.setattr(OP, "LINK_MASS", model.mass)
            mpc.setattr(OP, "LINK_COM", model.com)
            mpc.setattr(OP, "LINK_INERTIA", model.inertia)
            want = OP.gravity_torque(q)
        assert np.max(np.abs(got - want)) < 1e-12
        assert np.max(np.abs(got - OP.gravity_torque(q))) > 0.05  # the patch is gone and the model differs


def test_loop_argument_is_checked_before_the_device():
    traj, _ = benchmark_traj(np.array([-0.4, 0.05, 0.55]))
    cfg = classical_benchmark_config(0.005, 0.3)
    q0 = np.tile(R.Q_NEUTRAL, (2, 1))
    with pytest.raises(ValueError, match="link_models"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, link_models=[R.LinkModel()])
    with pytest.raises(ValueError, match="link_models"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, link_models=[R.LinkModel(), 1.0])


def test_run_sweep_payload_arguments_and_draw():
    kw = dict(seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(NotImplementedError, match="device_loop"):
        FL.run_sweep(payload_spread=(0.0, 3.0), **kw)
    for bad in ((1.0, 0.5), (0.5,), (0.5, np.inf), (np.nan, 1.0), (-1.0, 1.0), 0.5, (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match="payload_spread"):
            FL.run_sweep(payload_spread=bad, device_loop=True, **kw)
    names, tilt, scale, seed = FL._sweep_instances(("flat", "tilted_10"), 3)
    pm = FL.sweep_payload_masses(seed, (0.0, 3.0))
    assert pm.shape == (len(seed),)
    for b, s in enumerate(seed):
        u = np.random.default_rng([int(s), 7]).uniform(0.0, 1.0)
        assert pm[b] == 0.0 + (3.0 - 0.0) * u
    assert np.all((pm >= 0.0) & (pm <= 3.0)) and len(set(pm[:3])) == 3
    assert np.array_equal(FL.sweep_payload_masses(seed, [0.0, 3.0]), pm)
    assert np.all(FL.sweep_payload_masses(seed, (1.5, 1.5)) == 1.5)
    # a generator of its own: every other per-instance draw is unmoved
    spread = {"w_tau": (2.0e-4, 3.2e-3), "w_fn": (7.0, 112.0)}
    w, sc = FL.sweep_cost_weights(seed, spread), FL.sweep_limit_scales(seed, (0.25, 1.0))
    phys = FL.sweep_plant_physics(seed, (0.5, 0.5))
    FL.sweep_payload_masses(seed, (0.0, 3.0))
    again = FL.sweep_cost_weights(seed, spread)
    assert all(np.array_equal(again[k], w[k]) for k in w)
    assert np.array_equal(FL.sweep_limit_scales(seed, (0.25, 1.0)), sc)
    assert FL.sweep_plant_physics(seed, (0.5, 0.5)) == phys
    for s in seed:
        for stream in (1, 2, 3, 4, 5, 6):
            a = np.random.default_rng([int(s), stream]).uniform(0.0, 1.0, 2)
            assert not np.array_equal(a, np.random.default_rng([int(s), 7]).uniform(0.0, 1.0, 2))


def test_sweep_tool_payload_spread_option(capsys):
    spec = importlib.util.spec_from_file_location("sweep_c4_tool_mdl", ROOT / "tools" / "sweep_c4.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    a = ap.parse_args(["--device-loop", "1", "--payload-spread", "0", "3"])
    assert a.payload_spread == [0.0, 3.0] and FL.check_payload_spread(a.payload_spread) == (0.0, 3.0)
    assert ap.parse_args([]).payload_spread is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--payload-spread", "0.25"])
    capsys.readouterr()
