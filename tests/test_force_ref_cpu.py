"""Host side of the per-instance force reference: ForceProfile, the numpy
sampler, the run log's metrics with an array reference, run_sweep's argument
checks.  No device."""
from __future__ import annotations

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp.runlog import accumulate_metrics, metrics_accumulators, summary_metrics
from ffddp.trajectory import ForceProfile, force_records, sample_force


def test_force_profile_validation():
    p = ForceProfile(5.0, 30.0, t_on=1.0, t_ramp=0.5)
    assert (p.f0, p.f1, p.t_on, p.t_ramp) == (5.0, 30.0, 1.0, 0.5)
    assert ForceProfile(8.0, 8.0) == ForceProfile(8.0, 8.0, 0.0, 0.0)
    ForceProfile(0.0, 0.0, -1.0, 0.0)  # zero force and a negative switch time are legal
    for bad in (dict(f0=-1.0, f1=5.0), dict(f0=5.0, f1=-0.1), dict(f0=5.0, f1=6.0, t_ramp=-0.1),
                dict(f0=np.nan, f1=5.0), dict(f0=5.0, f1=np.inf), dict(f0=5.0, f1=6.0, t_on=np.nan),
                dict(f0=5.0, f1=6.0, t_ramp=np.inf)):
        with pytest.raises(ValueError):
            ForceProfile(**bad)
    rec = force_records([p, ForceProfile(8.0, 8.0)])
    assert rec.shape == (2, _abi.FLEET_FORCE_W) and rec.dtype == np.float64
    assert np.array_equal(rec, [[5.0, 30.0, 1.0, 0.5], [8.0, 8.0, 0.0, 0.0]])
    assert force_records([]).shape == (0, _abi.FLEET_FORCE_W)


def test_sample_force_breakpoints():
    rec = force_records([ForceProfile(5.0, 30.0, t_on=1.0, t_ramp=0.5)])
    f = lambda t: float(sample_force(rec, t)[0])  # noqa: E731
    assert f(0.2) == 5.0 and f(-3.0) == 5.0  # below t_on
    assert f(1.0) == 5.0  # at t_on: s = 0
    assert f(1.25) == 5.0 + (30.0 - 5.0) * ((1.25 - 1.0) / 0.5)  # inside the ramp, the formula's own rounding
    assert f(1.5) == 30.0  # at t_on + t_ramp: s = 1
    assert f(2.0) == 30.0 and f(1.0e6) == 30.0  # above
    # t_ramp = 0: a step at t_on, the new value from t_on itself
    step = force_records([ForceProfile(8.0, 35.0, t_on=0.4, t_ramp=0.0)])
    g = lambda t: float(sample_force(step, t)[0])  # noqa: E731
    assert g(np.nextafter(0.4, 0.0)) == 8.0 and g(0.4) == 35.0 and g(0.5) == 35.0 and g(-1.0) == 8.0
    # a falling profile, and a constant one at any time
    assert float(sample_force(force_records([ForceProfile(30.0, 10.0, 0.0, 2.0)]), 1.0)[0]) == 20.0
    assert np.array_equal(sample_force(force_records([ForceProfile(22.0, 22.0)]), np.array([-1.0])), [22.0])
    # shapes: one time per row, and rows against a (B, K) grid of times
    both = np.concatenate([rec, step])
    assert np.array_equal(sample_force(both, np.array([1.25, 0.4])), [f(1.25), g(0.4)])
    grid = sample_force(both, np.array([[0.2, 1.25, 2.0], [0.2, 0.4, 2.0]]))
    assert np.array_equal(grid, [[5.0, f(1.25), 30.0], [8.0, 35.0, 35.0]])
    assert np.array_equal(sample_force(both, 2.0), [30.0, 35.0])


def _records(rng, B):
    obs = rng.normal(size=(B, 48))
    obs[:, 46] = rng.uniform(0.0, 40.0, B)
    obs[:, 47] = rng.random(B) < 0.8
    return obs


def test_accumulate_metrics_array_reference_equals_scalar_calls():
    rng = np.random.default_rng(5)
    B, calls = 7, 9
    fn_des = rng.uniform(4.0, 40.0, B)
    t_phase = np.full(B, 0.02)
    acc = metrics_accumulators(B)
    cols = [metrics_accumulators(1) for _ in range(B)]
    scalar = metrics_accumulators(B)
    for k in range(calls):
        obs, p_ref, ts = _records(rng, B), rng.normal(size=(B, 3)), 0.005 * k
        info = rng.normal(size=(B, _abi.FLEET_INFO_W))
        accumulate_metrics(acc, obs, p_ref, ts, t_phase, fn_des, info)
        accumulate_metrics(scalar, obs, p_ref, ts, t_phase, 22.0, info)
        for b in range(B):
            accumulate_metrics(cols[b], obs[b:b + 1], p_ref[b:b + 1], ts, t_phase[b:b + 1], float(fn_des[b]), info[b:b + 1])
    for b in range(B):
        assert np.array_equal(acc[:, b], cols[b][:, 0]), b
    i = _abi.FLEET_METRICS_FIELDS.index("sum_abs_fn_err")
    others = [j for j in range(_abi.FLEET_METRICS_W) if j != i]
    assert np.array_equal(acc[others], scalar[others]) and not np.array_equal(acc[i], scalar[i])
    # a scalar handed over as a 0-d array or a numpy float is the scalar path
    again = metrics_accumulators(B)
    rng = np.random.default_rng(5)
    rng.uniform(4.0, 40.0, B)
    for k in range(calls):
        obs, p_ref, ts = _records(rng, B), rng.normal(size=(B, 3)), 0.005 * k
        info = rng.normal(size=(B, _abi.FLEET_INFO_W))
        accumulate_metrics(again, obs, p_ref, ts, t_phase, np.float64(22.0) if k % 2 else np.array(22.0), info)
    assert np.array_equal(again, scalar)


def test_summary_metrics_series_reference():
    rng = np.random.default_rng(6)
    n = 50
    t = 0.005 * np.arange(1, n + 1)
    et, e3, fn = rng.random(n), rng.random(n), rng.uniform(0.0, 30.0, n)
    contact = (fn > 0.5).astype(float)
    scalar = summary_metrics(t, et, e3, fn, contact, 22.0, 0.1)
    const = summary_metrics(t, et, e3, fn, contact, np.full(n, 22.0), 0.1)
    assert scalar == const
    ramp = np.linspace(5.0, 40.0, n)
    s = summary_metrics(t, et, e3, fn, contact, ramp, 0.1)
    assert s["avg_abs_force_err"] == float(np.mean(np.abs(fn - ramp))) != scalar["avg_abs_force_err"]
    assert {k: v for k, v in s.items() if k != "avg_abs_force_err"} == \
        {k: v for k, v in scalar.items() if k != "avg_abs_force_err"}


def test_run_sweep_force_arguments():
    with pytest.raises(NotImplementedError, match="device_loop"):
        FL.run_sweep(force_spread=(8.0, 36.0), seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(NotImplementedError, match="device_loop"):
        FL.run_sweep(force_spread=(8.0, 36.0), force_ramp=0.5, seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(ValueError, match="force_ramp needs force_spread"):
        FL.run_sweep(force_ramp=0.5, device_loop=True, seeds=1, scenarios=("flat",), verbose=False)
    for bad in ((36.0, 8.0), (-1.0, 8.0), (8.0,), (8.0, np.inf)):
        with pytest.raises(ValueError, match="force_spread"):
            FL.run_sweep(force_spread=bad, device_loop=True, seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(ValueError, match="force_ramp"):
        FL.run_sweep(force_spread=(8.0, 36.0), force_ramp=-0.5, device_loop=True, seeds=1, scenarios=("flat",),
                     verbose=False)
