"""Host side of the per-instance torque limits: the row builder against a numpy
restatement of fill_consts' lines, the header constants, DeviceFleetLoop's and
run_sweep's argument checks and draws, and the sweep tool's option.  No device."""
from __future__ import annotations

import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp import robot as R
from ffddp.config import classical_preset, ff_preset, torque_limit_rows
from ffddp.controller import classical_benchmark_config
from ffddp.fleet_loop import DeviceFleetLoop, instance_torque_limits
from ffddp.trajectory import benchmark_traj

ROOT = Path(__file__).resolve().parents[1]


def test_header_constants_equal_abi():
    text = (ROOT / "include" / "ffddp.h").read_text()
    m = re.search(r"#define FFDDP_TAU_LIM_W (\d+)", text)
    assert m and int(m.group(1)) == _abi.TAU_LIM_W == 32
    for sym in ("ffddp_solve_batch_lim_dev", "ffddp_calc_diff_lim", "ffddp_torque_limit_rows",
                "ffddp_fleet_post_lim_dev"):
        assert sym in _abi.SYMBOLS and re.search(r"\bint %s\(" % sym, text), sym


def _restated(limits, margin):
    """csrc/ffddp_consts.hpp's torque-limit lines in numpy, operation for operation (float64)."""
    lim = np.asarray(limits, np.float64)
    mn = lim[0]
    for i in range(1, 7):
        mn = lim[i] if lim[i] < mn else mn
    mg = np.float64(margin) if margin > 0.0 else np.float64(0.0)
    mg = mg if mg < mn - np.float64(1.0e-6) else mn - np.float64(1.0e-6)
    ts_lb, ts_ub, u_lb, u_ub = -lim + mg, lim - mg, -lim, lim.copy()
    wm = np.float64(margin) if margin > 0.0 else np.float64(0.0)
    l_ = lim - wm
    ws = np.where(l_ > 1.0e-9, l_, 1.0e-9)
    return dict(ts_lb=ts_lb, ts_ub=ts_ub, u_lb=u_lb, u_ub=u_ub, ws_lim=ws, mg=mg)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


MARGINS = (0.2, 0.0, -1.0, 11.5, 12.0, 300.0)  # 12 N m is the smallest Panda limit: the last three take the clamp


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("preset", [classical_preset, ff_preset])
def test_row_of_the_configuration_restates_fill_consts(preset, margin):
    cfg = preset(12)
    cfg.tau_soft_limit_margin = margin
    lim = np.asarray(cfg.tau_limits, float)
    rows = torque_limit_rows(cfg, lim[None])
    assert rows.shape == (1, _abi.TAU_LIM_W) and rows.dtype == np.float64
    want = _restated(lim, margin)
    if margin >= lim.min():
        assert want["mg"] == lim.min() - 1.0e-6
    r = rows[0]
    for j in range(7):
        assert _bits(r[4 * j + 0]) == _bits(want["u_ub"][j]), j
        assert _bits(r[4 * j + 1]) == _bits(want["ts_ub"][j]), j
        assert _bits(r[4 * j + 2]) == _bits(want["ws_lim"][j]), j
        assert r[4 * j + 3] == 0.0
    assert not r[28:].any()
    # the kernels form the lower bounds by negation: the restated ones are those bits
    assert np.array_equal(_bits(-want["ts_ub"]), _bits(want["ts_lb"]))
    assert np.array_equal(_bits(-want["u_ub"]), _bits(want["u_lb"]))
    assert np.array_equal(_bits(-r[1:28:4]), _bits(want["ts_lb"])) and np.array_equal(_bits(-r[0:28:4]), _bits(want["u_lb"]))


def test_rows_of_distinct_limits():
    cfg = ff_preset(8)
    base = np.asarray(cfg.tau_limits, float)
    rng = np.random.default_rng(3)
    lim = base[None] * rng.choice([1.0, 0.5, 0.25, 0.125, 0.0625, 0.013], size=(9, 7))
    rows = torque_limit_rows(cfg, lim)
    for b in range(lim.shape[0]):  # the margin's clamp follows each instance's own smallest limit
        want = _restated(lim[b], cfg.tau_soft_limit_margin)
        assert np.array_equal(_bits(rows[b, 0:28:4]), _bits(want["u_ub"]))
        assert np.array_equal(_bits(rows[b, 1:28:4]), _bits(want["ts_ub"]))
        assert np.array_equal(_bits(rows[b, 2:28:4]), _bits(want["ws_lim"]))
    assert np.any(lim.min(1) < cfg.tau_soft_limit_margin)  # some row takes the clamp
    assert np.all(rows[:, 1:28:4] > 0.0)
    # row b depends on limits[b] alone
    assert np.array_equal(torque_limit_rows(cfg, lim[4:5])[0], rows[4])
    assert torque_limit_rows(cfg, np.zeros((0, 7))).shape == (0, _abi.TAU_LIM_W)


def test_builder_errors():
    cfg = classical_preset(8)
    base = np.asarray(cfg.tau_limits, float)
    for bad in (0.0, -3.0, np.nan, np.inf):
        lim = np.tile(base, (2, 1))
        lim[1, 4] = bad
        with pytest.raises(ValueError, match="finite"):
            torque_limit_rows(cfg, lim)
        # the C builder itself refuses them too
        out = np.zeros((2, _abi.TAU_LIM_W))
        import ctypes as C

        st = cfg.to_struct()
        assert _abi.load().ffddp_torque_limit_rows(C.byref(st), 2, _abi.dptr(lim), _abi.dptr(out)) == -1
        assert _abi.load().ffddp_torque_limit_rows(None, 2, _abi.dptr(lim), _abi.dptr(out)) == -1
    for shape in ((7,), (2, 6), (2, 7, 1)):
        with pytest.raises(ValueError, match="shape"):
            torque_limit_rows(cfg, np.ones(shape))


def test_loop_argument():
    base = np.asarray(R.TAU_LIMITS, float)
    lim = instance_torque_limits(base, [1.0, 0.5, 0.25], 3)
    assert lim.shape == (3, 7) and np.array_equal(lim[0], base) and np.array_equal(lim[2], 0.25 * base)
    arr = np.tile(base, (3, 1)) * np.array([[1.0], [0.5], [0.125]])
    got = instance_torque_limits(base, arr, 3)
    assert np.array_equal(got, arr) and got is not arr
    for bad in ([1.0, 0.5], np.ones((3, 6)), np.ones((2, 7)), 0.5, np.ones((3, 7, 1))):
        with pytest.raises(ValueError, match="torque_limits takes"):
            instance_torque_limits(base, bad, 3)
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0]):
        with pytest.raises(ValueError, match="finite"):
            instance_torque_limits(base, bad, 3)
    nan = arr.copy()
    nan[1, 3] = np.nan
    neg = arr.copy()
    neg[2, 0] = -1.0
    for bad in (nan, neg, np.zeros((3, 7))):
        with pytest.raises(ValueError, match="finite"):
            instance_torque_limits(base, bad, 3)
    # the loop itself, before it touches the device
    traj, _ = benchmark_traj(np.array([-0.4, 0.05, 0.55]))
    cfg = classical_benchmark_config(0.005, 0.3)
    q0 = np.tile(R.Q_NEUTRAL, (2, 1))
    with pytest.raises(ValueError, match="torque_limits"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, torque_limits=[1.0, 0.5, 0.25])
    with pytest.raises(ValueError, match="finite"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, torque_limits=[1.0, 0.0])
    with pytest.raises(ValueError, match="finite"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, torque_limits=np.full((2, 7), np.nan))


def test_sweep_draws_are_reproducible_and_move_no_other_draw():
    names, tilt, scale, seed = FL._sweep_instances(("flat", "tilted_10"), 3)
    sc = FL.sweep_limit_scales(seed, (0.25, 1.0))
    assert sc.shape == (len(seed),)
    for b, s in enumerate(seed):
        u = np.random.default_rng([int(s), 6]).uniform(-1.0, 1.0)
        assert sc[b] == 0.25 * (1.0 / 0.25) ** (0.5 * (1.0 + u))
    assert np.all((sc >= 0.25) & (sc <= 1.0)) and len(set(sc[:3])) == 3
    assert np.array_equal(FL.sweep_limit_scales(seed, [0.25, 1.0]), sc)
    assert np.all(FL.sweep_limit_scales(seed, (0.5, 0.5)) == 0.5)
    # a generator of its own: every other per-instance draw is its own generator's, before and after
    spread = {"w_tau": (2.0e-4, 3.2e-3), "w_fn": (7.0, 112.0)}
    w = FL.sweep_cost_weights(seed, spread)
    phys = FL.sweep_plant_physics(seed, (0.5, 0.5))
    FL.sweep_limit_scales(seed, (0.25, 1.0))
    again = FL.sweep_cost_weights(seed, spread)
    assert all(np.array_equal(again[k], w[k]) for k in w)
    assert FL.sweep_plant_physics(seed, (0.5, 0.5)) == phys
    for s in seed:
        for stream in (1, 2, 3, 4, 5):
            a = np.random.default_rng([int(s), stream]).uniform(-1.0, 1.0, 2)
            assert not np.array_equal(a, np.random.default_rng([int(s), 6]).uniform(-1.0, 1.0, 2))


def test_run_sweep_limit_arguments():
    kw = dict(seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(NotImplementedError, match="device_loop"):
        FL.run_sweep(limit_spread=(0.25, 1.0), **kw)
    for bad in ((0.0, 1.0), (1.0, 0.5), (0.5,), (0.5, np.inf), (np.nan, 1.0), (-1.0, 1.0), 0.5, (0.25, 0.5, 1.0)):
        with pytest.raises(ValueError, match="limit_spread"):
            FL.run_sweep(limit_spread=bad, device_loop=True, **kw)


def _sweep_tool():
    spec = importlib.util.spec_from_file_location("sweep_c4_tool_lim", ROOT / "tools" / "sweep_c4.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sweep_tool_limit_spread_option(capsys):
    ap = _sweep_tool().build_parser()
    a = ap.parse_args(["--device-loop", "1", "--limit-spread", "0.25", "1"])
    assert a.limit_spread == [0.25, 1.0] and FL.check_limit_spread(a.limit_spread) == (0.25, 1.0)
    assert ap.parse_args([]).limit_spread is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--limit-spread", "0.25"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--limit-spread", "lo", "1"])
    capsys.readouterr()
