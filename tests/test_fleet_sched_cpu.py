"""The scheduled fleet tick's host side (no device here): ffddp_fleet_sched's
ctypes layout against the header, the solve-period and command-filter
validation of DeviceFleetLoop and run_sweep (raised before any device use),
the batched command filter against the scalar controller's _safe_tau bit for
bit, and the age indexing of the unmoved kept solution against the
controllers' own list shifting."""
import ctypes
import subprocess
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from ffddp import _abi
from ffddp import controller as CT
from ffddp import fleet as FL
from ffddp import robot as R
from ffddp.fleet_loop import DeviceFleetLoop, resolve_solve_period
from ffddp.trajectory import benchmark_traj

ROOT = Path(__file__).resolve().parents[1]


def test_fleet_sched_layout_matches_header():
    names = [n for n, _ in _abi.FleetSched._fields_]
    offs = "".join(f'  printf("%zu ", offsetof(ffddp_fleet_sched, {n}));\n' for n in names)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ffddp.h"\nint main(void) {\n'
           '  printf("%zu ", sizeof(ffddp_fleet_sched));\n' + offs + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(src)
        exe = Path(d) / "t"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(exe)], check=True)
        vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_abi.FleetSched)
    assert vals[1:] == [getattr(_abi.FleetSched, n).offset for n in names]
    # the header's field order is the binding's
    hdr = (ROOT / "include" / "ffddp.h").read_text()
    body = hdr.split("typedef struct ffddp_fleet_sched {")[1].split("} ffddp_fleet_sched;")[0]
    fields = []
    for ln in body.strip().splitlines():
        decl = ln.split(";")[0]
        fields.append(decl.replace("*", " ").replace("[7]", "").split()[-1])
    assert fields == names


def test_fleet_sched_from_config():
    cfg = CT.classical_benchmark_config(0.005, 0.342)
    cfg.apply_command_filter, cfg.tau_smoothing_alpha = True, 1.7
    s = _abi.fleet_sched(cfg, 3, 0.005)
    assert (s.period, s.apply_filter, s.dt, s.tau_trust_inf) == (3, 1, 0.005, float(cfg.tau_trust_inf))
    assert s.tau_smoothing_alpha == 1.0  # clipped to [0, 1], as _safe_tau does
    assert list(s.tau_rate_limit) == list(np.asarray(cfg.tau_rate_limit, float))
    assert not s.since and not s.age and not s.need


def test_sched_entry_points_null_handle():
    lib = _abi.load()
    p, s, q = _abi.FleetParams(), _abi.FleetState(), _abi.FleetSched()
    pre = lib.ffddp_fleet_pre_sched_dev(None, 1, ctypes.byref(p), ctypes.byref(s), *([None] * 5), 7, 1, None, 7, None,
                                        None, 0, *([None] * 6), q, None)
    post = lib.ffddp_fleet_post_sched_dev(None, 1, ctypes.byref(p), ctypes.byref(s), *([None] * 8), None, None, None,
                                          7, None, None, None, None, None, 0.2, None, 0, None, q, None)
    sel = lib.ffddp_solve_batch_sel_dev(None, 1, *([None] * 6), 10, 0, *([None] * 8), None, None)
    assert pre == -1 and post == -1 and sel == -1  # FFDDP_E_INVALID


def test_solve_period_validation():
    """All of it is host arithmetic on the arguments: no device object exists yet."""
    cfg = CT.classical_benchmark_config(0.005, 0.342, horizon=8)
    assert resolve_solve_period(cfg, None) == 1 and resolve_solve_period(cfg, 1) == 1
    assert resolve_solve_period(cfg, 4) == 4
    for bad in (0, -2, 2.5, True):
        with pytest.raises(ValueError, match="solve_period"):
            resolve_solve_period(cfg, bad)
    cfg.mpc_update_steps = 2
    assert resolve_solve_period(cfg, 2) == 2
    with pytest.raises(NotImplementedError):
        resolve_solve_period(cfg, None)
    with pytest.raises(ValueError, match="contradicts"):
        resolve_solve_period(cfg, 3)
    # the loop itself, before it touches the device
    traj, _ = benchmark_traj(np.array([-0.4, 0.05, 0.55]))
    q0 = np.tile(R.Q_NEUTRAL, (2, 1))
    with pytest.raises(ValueError, match="contradicts"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, solve_period=3)
    with pytest.raises(ValueError, match="solve_period"):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4, solve_period=0)
    with pytest.raises(NotImplementedError):
        DeviceFleetLoop("classical", 2, traj, cfg, q0, steps=4)


def test_run_sweep_validation():
    kw = dict(scenarios=("flat",), seeds=1, total_time=0.1, verbose=False)
    for dl in (False, True):
        with pytest.raises(ValueError, match="solve_period"):
            FL.run_sweep(solve_period=0, device_loop=dl, **kw)
        with pytest.raises(ValueError, match="solve_period"):
            FL.run_sweep(solve_period=1.5, device_loop=dl, **kw)
        with pytest.raises(ValueError, match="command_filter"):
            FL.run_sweep(command_filter="yes", device_loop=dl, **kw)


def test_fleets_refuse_a_period_below_one():
    cfg = CT.classical_benchmark_config(0.005, 0.342, horizon=8)
    cfg.mpc_update_steps = 0
    with pytest.raises(ValueError, match="mpc_update_steps"):
        FL.FleetClassicalMPC(2, None, cfg, np.zeros((2, 7)), np.zeros((2, 7)), np.eye(3), np.zeros(3))


@pytest.mark.parametrize("apply_filter", [True, False])
def test_safe_tau_batch_equals_scalar_safe_tau(apply_filter):
    """B calls of the scalar controller's _safe_tau against one batched call."""
    rng = np.random.default_rng(7)
    B, dt = 64, 0.005
    cfg = CT.classical_benchmark_config(dt, 0.342)
    cfg.apply_command_filter = apply_filter
    lim = np.asarray(cfg.tau_limits, float)
    prev = rng.uniform(-1.0, 1.0, (B, 7)) * lim
    target = prev + rng.normal(0.0, 0.3, (B, 7))                    # inside every bound
    target[8:16] += rng.normal(0.0, 5.0, (8, 7))                    # beyond the rate bound (450 * dt = 2.25)
    target[16:24] += np.sign(rng.normal(size=(8, 7))) * 60.0        # beyond the trust bound (40)
    target[24:32] = rng.normal(0.0, 3.0, (8, 7)) * lim              # beyond the torque limits
    target[32, 3] = np.nan                                          # a NaN row: the previous command
    target[33, 0] = np.inf
    target[34] = np.nan
    prev[40] = lim                                                  # at the limit already
    target[40] = 2.0 * lim
    assert np.any(np.abs(target[8:16] - prev[8:16]) > np.asarray(cfg.tau_rate_limit) * dt)
    assert np.any(np.abs(target[16:24] - prev[16:24]) > cfg.tau_trust_inf) and np.any(np.abs(target[24:32]) > lim)
    got = FL.safe_tau_batch(target, prev, cfg, dt)
    for b in range(B):
        ns = SimpleNamespace(cfg=cfg, sim=SimpleNamespace(dt=dt), _tau_prev=prev[b].copy())
        want = CT._MPCBase._safe_tau(ns, target[b])
        assert np.array_equal(got[b], want, equal_nan=True), b
        assert np.array_equal(ns._tau_prev, want, equal_nan=True)
    assert np.all(np.isfinite(got))
    if apply_filter:
        assert not np.array_equal(got, FL.safe_tau_batch(target, prev, CT.classical_benchmark_config(dt, 0.342), dt))


def _shifted_lists(xs, us, Ks, a):
    """The controllers' lists after `a` receding-horizon shifts (_rollout_shift itself)."""
    c = SimpleNamespace(xs=[x.copy() for x in xs], us=[u.copy() for u in us], Ks=[k.copy() for k in Ks], ks=None)
    for _ in range(a):
        CT._MPCBase._rollout_shift(c)
    return c


@pytest.mark.parametrize("nx", [14, 21])
def test_age_indexing_equals_list_shifting(nx):
    """The kept arrays are never moved: after `a` shifts knot i of the lists is
    knot min(i + a, N - 1) of us / K and min(i + a, N) of xs, and the warm start
    (_shift_guess of the shifted lists) is xs_init[k >= 1] = xs[min(k + a, N)],
    us_init[k] = us[min(k + 1 + a, N - 1)]."""
    N = 8
    rng = np.random.default_rng(nx)
    xs, us, Ks = rng.normal(size=(N + 1, nx)), rng.normal(size=(N, 7)), rng.normal(size=(N, 7, nx))
    x0 = rng.normal(size=nx)
    for a in (0, 1, N - 1, N + 3):
        c = _shifted_lists(xs, us, Ks, a)
        assert len(c.xs) == N + 1 and len(c.us) == N and len(c.Ks) == N
        for i in range(N):
            assert np.array_equal(c.us[i], us[min(i + a, N - 1)]) and np.array_equal(c.Ks[i], Ks[min(i + a, N - 1)])
        for i in range(N + 1):
            assert np.array_equal(c.xs[i], xs[min(i + a, N)])
        # what the policy reads: knot 0, and (force feedback) the next state knot
        assert np.array_equal(c.us[0], us[min(a, N - 1)]) and np.array_equal(c.xs[1], xs[min(a + 1, N)])
        c._cold_control = lambda x: np.zeros(7)
        xs_init, us_init = CT._MPCBase._shift_guess(c, x0, N)
        want_xs = np.stack([x0] + [xs[min(k + a, N)] for k in range(1, N + 1)])
        want_us = np.stack([us[min(k + 1 + a, N - 1)] for k in range(N)])
        assert np.array_equal(np.asarray(xs_init), want_xs), a
        assert np.array_equal(np.asarray(us_init), want_us), a
