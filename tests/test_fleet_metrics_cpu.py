"""The sweep's task metrics from running sums, host side: runlog.accumulate_metrics
(the numpy restatement of one ffddp_fleet_metrics_dev call) fed tick by tick,
then runlog.metrics_from_accumulators, against runlog.summary_metrics on the
same series; the header's field indices against _abi; and the argument
refusals that need no device.

Counts, max_fn, the contact-loss percentages (sums of zeros and ones: exact in
any order) and the NaN pattern are exact.  A value made of a sum S of n
non-negative terms is compared relatively within (2 n + 8) * 2^-53: the
accumulators add in tick order (error at most (n - 1) u S), numpy's mean adds
pairwise (at most about (log2 n + 16) u S with its blocks of 8 and 128), and
the division and square root after the sum add at most 2 u on each side --
together below (2 n + 8) u for every n (for n < 8 both add sequentially).
No device."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp.fleet_loop import DeviceFleetLoop
from ffddp.runlog import accumulate_metrics, metrics_accumulators, metrics_from_accumulators, summary_metrics
from ffddp.trajectory import benchmark_traj

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -53
F = {k: i for i, k in enumerate(_abi.FLEET_METRICS_FIELDS)}
SUM_KEYS = ("avg_abs_position_err", "avg_abs_force_err", "rms_tangential_error", "rms_tangential_error_contact_phase",
            "rms_3d_error", "fn_mean_contact_phase")
EXACT_KEYS = ("max_fn", "contact_loss_pct", "contact_loss_contact_phase_pct")
PHASE_KEYS = ("rms_tangential_error_contact_phase", "contact_loss_contact_phase_pct", "fn_mean_contact_phase")


def test_header_and_abi_agree_on_the_fields():
    hdr = (ROOT / "include" / "ffddp.h").read_text()
    assert int(re.search(r"#define FFDDP_FLEET_METRICS_W (\d+)", hdr).group(1)) == _abi.FLEET_METRICS_W
    idx = {m.group(1).lower(): int(m.group(2))
           for m in re.finditer(r"#define FFDDP_FLEET_METRICS_([A-Z0-9_]+) (\d+)", hdr) if m.group(1) != "W"}
    assert idx == F and len(F) == _abi.FLEET_METRICS_W
    assert "ffddp_fleet_metrics_dev" in _abi.SYMBOLS


def _series(seed, steps, B, dt=0.005):
    """Random records and references: obs (steps, B, 48), p_ref (steps, B, 3), ts (steps, B), info, need."""
    rng = np.random.default_rng(seed)
    p_ref = rng.normal(0.0, 0.3, (steps, B, 3))
    obs = rng.normal(size=(steps, B, 48))
    obs[:, :, 28:31] = p_ref + rng.normal(0.0, 0.01, (steps, B, 3))
    obs[:, :, 46] = rng.uniform(0.0, 3.0, (steps, B))
    obs[:, :, 47] = (rng.random((steps, B)) < 0.7).astype(float)
    delay = rng.uniform(0.0, 0.03, B)
    t = np.zeros(steps)
    for k in range(1, steps):
        t[k] = t[k - 1] + dt
    ts = (t[:, None] - delay[None, :]) + dt
    info = rng.normal(size=(steps, B, _abi.FLEET_INFO_W))
    info[:, :, 0] = rng.random((steps, B)) < 0.8
    info[:, :, 4] = rng.random((steps, B)) < 0.2
    info[:, :, 7] = rng.integers(0, 3, (steps, B))
    need = (rng.random((steps, B)) < 0.4).astype(np.uint8)
    fail = (rng.random((steps, B)) < 0.05).astype(np.int32)
    return obs, p_ref, ts, info, need, fail


def _host_summary(obs, p_ref, ts, fn_des, t_phase):
    """fleet._run_sweep_device's series and summary_metrics per instance."""
    err = obs[:, :, 28:31] - p_ref
    fnm = obs[:, :, 46] * (obs[:, :, 47] > 0.5)
    et, e3 = np.linalg.norm(err[:, :, :2], axis=2), np.linalg.norm(err, axis=2)
    contact = (fnm > 0.5).astype(float)
    return [summary_metrics(ts[:, b], et[:, b], e3[:, b], fnm[:, b], contact[:, b], fn_des, t_phase[b])
            for b in range(obs.shape[1])], e3


@pytest.mark.parametrize("steps", [5, 50, 300])
def test_accumulated_summary_equals_summary_metrics(steps):
    B, ld, fn_des = 7, 10, 1.5
    obs, p_ref, ts, info, need, fail = _series(steps, steps, B)
    t_phase = np.array([0.1, 0.0, np.inf, 0.12, 0.05, ts[:, 5].max(), -1.0])  # 2: no contact phase; 5: its last tick only
    if steps > 5:
        obs[steps - 2, 4, 46], obs[steps - 2, 4, 47] = np.nan, 1.0  # a NaN force, inside instance 4's contact phase
        assert ts[steps - 2, 4] >= t_phase[4]
    acc = metrics_accumulators(B, ld)
    acc[:, B:] = -777.25
    for k in range(steps):
        assert accumulate_metrics(acc, obs[k], p_ref[k], ts[k], t_phase, fn_des, info[k], need[k], fail[k]) is acc
    assert np.all(acc[:, B:] == -777.25)  # the columns beyond B are not touched
    got = metrics_from_accumulators(acc[:, :B])
    want, e3 = _host_summary(obs, p_ref, ts, fn_des, t_phase)
    phase = ts >= t_phase[None, :]
    assert np.array_equal(acc[F["n"], :B], np.full(B, float(steps)))
    assert np.array_equal(acc[F["n_phase"], :B], phase.sum(0).astype(float))
    assert phase[:, 2].sum() == 0 and phase[:, 5].sum() == 1 and phase[:, 6].all()
    assert steps == 5 or 0 < phase[:, 0].sum() < steps
    assert np.array_equal(got["unstable_ticks"], (info[:, :, 4] != 0).sum(0))
    assert np.array_equal(got["neg_accepted_ticks"], (info[:, :, 7] > 0).sum(0))
    assert np.array_equal(got["solve_not_ok_ticks"], (info[:, :, 0] == 0).sum(0))
    assert np.array_equal(got["solved_ticks"], (need != 0).sum(0))
    assert np.array_equal(acc[F["plant_fail"], :B], fail.sum(0))
    assert np.array_equal(got["max_err_3d"], e3.max(0))
    for b in range(B):
        for k in EXACT_KEYS:
            assert np.array_equal(got[k][b], want[b][k], equal_nan=True), (b, k)
        for k in SUM_KEYS:
            n = phase[:, b].sum() if k in PHASE_KEYS else steps
            assert np.isnan(got[k][b]) == np.isnan(want[b][k]), (b, k)
            if not np.isnan(want[b][k]):
                assert abs(got[k][b] - want[b][k]) <= (2 * n + 8) * U * abs(want[b][k]), (b, k, got[k][b], want[b][k])
    assert all(np.isnan(got[k][2]) for k in PHASE_KEYS) and np.isfinite(got["rms_3d_error"][2])
    if steps > 5:  # the NaN force reaches the force figures (np.max propagates it too), not the tracking ones
        for k in ("max_fn", "avg_abs_force_err", "fn_mean_contact_phase"):
            assert np.isnan(got[k][4]) and np.isnan(want[4][k]), k
        assert np.isfinite(got["rms_tangential_error"][4]) and np.isfinite(got["contact_loss_pct"][4])
    assert all(np.isfinite(got[k][6]) for k in SUM_KEYS + EXACT_KEYS)


def test_no_tick_at_all_and_untouched_counters():
    B = 3
    acc = metrics_accumulators(B)
    assert acc.shape == (_abi.FLEET_METRICS_W, B) and np.all(acc[F["max_fn"]] == -np.inf)
    got = metrics_from_accumulators(acc)
    want = summary_metrics([], [], [], [], [], 1.5, 0.8)
    for k in SUM_KEYS + EXACT_KEYS:
        assert np.isnan(want[k]) and np.all(np.isnan(got[k])), k
    assert np.all(np.isnan(got["max_err_3d"])) and not got["solved_ticks"].any()
    # info = None leaves the four solver counters; need = None counts every instance as solving
    obs, p_ref, ts, info, need, _ = _series(1, 2, B)
    accumulate_metrics(acc, obs[0], p_ref[0, 0], 0.3, np.zeros(B), 1.5)  # a shared reference row and time
    for k in ("unstable_ticks", "neg_accepted_ticks", "not_ok_ticks", "solved_ticks", "plant_fail"):
        assert not acc[F[k]].any(), k
    assert np.all(acc[F["n"]] == 1.0) and np.all(acc[F["n_phase"]] == 1.0)
    accumulate_metrics(acc, obs[1], p_ref[1, 0], 0.305, np.zeros(B), 1.5, info=info[1])
    assert np.all(acc[F["solved_ticks"]] == 1.0) and np.all(acc[F["n"]] == 2.0)


def test_argument_refusals():
    traj, _ = benchmark_traj(np.array([-0.31, 0.02, 0.59]))
    q0 = np.zeros((2, 7))
    with pytest.raises(ValueError, match="metrics=True"):
        DeviceFleetLoop("classical", 2, traj, None, q0, logs=False)
    with pytest.raises(ValueError, match="t_contact_phase"):
        DeviceFleetLoop("classical", 2, traj, None, q0, metrics=True)
    for kw in (dict(device_summary=True), dict(device_summary=True, keep_logs=False)):
        with pytest.raises(NotImplementedError, match="device_loop"):
            FL.run_sweep(scenarios=("flat",), seeds=1, total_time=0.01, verbose=False, **kw)
    with pytest.raises(ValueError, match="device_summary"):
        FL.run_sweep(scenarios=("flat",), seeds=1, device_loop=True, keep_logs=False)
