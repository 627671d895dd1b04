"""Per-instance fleet tasks, host side: the task records and their numpy
sampler against the host trajectories (bit for bit), and the argument checks
of FleetTask, DeviceFleetLoop(tasks=...) and run_sweep.  No device."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp.fleet_loop import DeviceFleetLoop
from ffddp.trajectory import FleetTask, benchmark_task, benchmark_traj, sample_records, task_records

ROOT = Path(__file__).resolve().parents[1]
EE = np.array([-0.31, 0.02, 0.59])


def make_tasks():
    """Six tasks: with and without t_pre, with and without ee_start / z_pre, delays."""
    c = np.array([-0.5, 0.0, 0.342])
    return [
        benchmark_task(EE),
        benchmark_task(EE, radius=0.06, omega=2.0, delay=0.015),
        FleetTask(center=c, radius=0.12, omega=1.1, z_contact=0.342, t_approach=0.4, t_contact_phase=0.4, t_hold=0.15),
        FleetTask(center=c, radius=0.08, omega=1.7, z_contact=0.35, t_approach=0.5, t_pre=0.2, z_pre=0.45,
                  t_contact_phase=0.7, t_hold=0.1, delay=0.04),
        FleetTask(center=c + [0.02, -0.03, 0.0], radius=0.14, omega=1.0, z_contact=0.342, t_approach=0.3,
                  ee_start=EE + [0.05, 0.0, -0.1], t_contact_phase=0.3, t_hold=0.2),
        FleetTask(center=c, radius=0.1, omega=1.5, z_contact=0.342, t_approach=0.6, t_pre=0.1, ee_start=EE,
                  t_contact_phase=0.7, t_hold=0.0),
    ]


def task_times(task):
    """-0.05 .. 1.3 s, with the task's own phase boundaries exactly."""
    t_pre, t_app = max(float(task.t_pre), 0.0), max(float(task.t_approach), 1.0e-6)
    edges = [t_pre, t_pre + t_app, float(task.t_contact_phase) + float(task.t_hold), 0.0]
    near = [np.nextafter(e, s) for e in edges[:3] for s in (-np.inf, np.inf)]
    return np.concatenate([np.linspace(-0.05, 1.3, 55), edges, near])


def test_header_and_abi_agree_on_the_record_width():
    hdr = (ROOT / "include" / "ffddp.h").read_text()
    assert int(re.search(r"#define FFDDP_FLEET_TASK_W (\d+)", hdr).group(1)) == _abi.FLEET_TASK_W
    offs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FFDDP_FLEET_TASK_([A-Z_]+) (\d+)", hdr)}
    assert offs["DELAY"] == _abi.FLEET_TASK_W - 1 and offs["T_HOLD_END"] == 20 and offs["P_HOLD"] == 17
    assert task_records(make_tasks()).shape == (6, _abi.FLEET_TASK_W)


def test_traj_is_the_host_wrapper_and_benchmark_task_is_benchmark_traj():
    ts = np.linspace(-0.05, 1.3, 28)
    a, (b, meta) = benchmark_task(EE).traj(), benchmark_traj(EE)
    for x, y in zip(a.sample(ts), b.sample(ts)):
        assert np.array_equal(x, y)
    assert benchmark_task(EE).t_contact_phase == meta["t_contact_phase"]


def test_sample_records_equals_host_trajectories_bit_for_bit():
    tasks = make_tasks()
    rec = task_records(tasks)
    seen = set()
    for b, task in enumerate(tasks):
        t = task_times(task)
        P0, V0, S0 = task.traj().sample(t)
        # row b alone, and the same time for every row at once
        P, V, S = sample_records(np.repeat(rec[b:b + 1], t.size, 0), t)
        assert np.array_equal(P, P0) and np.array_equal(V, V0) and np.array_equal(S, S0), b
        for i, ti in enumerate(t):
            Pa, Va, Sa = sample_records(rec, ti)
            assert np.array_equal(Pa[b], P0[i]) and np.array_equal(Va[b], V0[i]) and Sa[b] == S0[i], (b, i)
            p, v, s = task.traj()(ti)  # the scalar path too
            assert np.array_equal(p, P0[i]) and np.array_equal(v, V0[i]) and s == S0[i], (b, i)
        hold = S0 & (t < task.t_contact_phase + task.t_hold)
        seen |= {("pre", bool(np.any(t < max(task.t_pre, 0.0)) and task.t_pre > 0)), ("hold", bool(hold.any())),
                 ("circle", bool((S0 & ~hold).any())), ("approach", bool((~S0).any()))}
    assert {("pre", True), ("pre", False), ("hold", True), ("hold", False), ("circle", True), ("approach", True)} <= seen
    assert rec[1, -1] == 0.015 and rec[0, -1] == 0.0  # the delay is carried, not applied


def test_negative_task_time_waits_at_the_start_pose():
    tasks = make_tasks()
    rec = task_records(tasks)
    P, V, S = sample_records(rec, -0.03)
    P0, _, _ = sample_records(rec, 0.0)
    assert np.array_equal(P, P0) and not V.any() and not S.any()
    assert np.array_equal(P, rec[:, 8:11])


def test_argument_checks():
    with pytest.raises(ValueError, match="delay"):
        benchmark_task(EE, delay=-0.005)
    with pytest.raises(ValueError, match="delay"):
        FleetTask(center=[0, 0, 0], radius=0.1, omega=1.0, z_contact=0.3, delay=float("nan"))
    traj, _ = benchmark_traj(EE)
    q0 = np.zeros((2, 7))
    with pytest.raises(ValueError, match="either traj_fn"):
        DeviceFleetLoop("classical", 2, traj, None, q0, tasks=benchmark_task(EE))
    with pytest.raises(ValueError, match="either traj_fn"):
        DeviceFleetLoop("classical", 2, None, None, q0)
    with pytest.raises(ValueError, match="one FleetTask per instance"):
        DeviceFleetLoop("classical", 2, None, None, q0, tasks=[benchmark_task(EE)] * 3)
    for kw in (dict(stagger=2), dict(device_refs=True), dict(task_spread=(0.3, 0.3))):
        with pytest.raises(NotImplementedError, match="device_loop"):
            FL.run_sweep(scenarios=("flat",), seeds=1, total_time=0.01, verbose=False, **kw)
    with pytest.raises(ValueError, match="stagger"):
        FL.run_sweep(scenarios=("flat",), seeds=1, device_loop=True, stagger=-1)
    with pytest.raises(ValueError, match="task_spread"):
        FL.run_sweep(scenarios=("flat",), seeds=1, device_loop=True, task_spread=(0.3, 1.5))
