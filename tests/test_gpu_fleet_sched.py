"""GPU: the host fleets with a solve period and the command filter against
B = 3 scalar controllers (ffddp.controller, the reference's logic) fed the same
observations: mpc_update_steps = 3 with apply_command_filter, and period 2
without it; classical with both glue paths, and force feedback.  Every tick and
instance must agree exactly -- the solver is batch-independent bit for bit and
the selected-instance solve gives a selected instance the unmasked solve's
bits (tests/test_gpu_solve_sel.py).

The schedule must be exercised: solved_now takes both values in every case,
and with period 3 a solve falls off the period grid -- the mode switch at
tick 20 (t = 0.8), 20 % 3 = 2.  With period 2 tick 20 is on the grid (every
instance solves there anyway), so that case asserts that the switch tick
solves and drops the plan instead."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp.trajectory import benchmark_traj  # noqa: E402

B, TICKS, T_START, HORIZON = 3, 40, 0.7, 8  # the contact hint flips at t = 0.8, inside the window


@pytest.mark.parametrize("period,use_filter", [(3, True), (2, False)])
@pytest.mark.parametrize("variant,device_tick", [("classical", False), ("classical", True), ("ff", None)])
def test_scheduled_fleet_matches_scalar_controllers(variant, device_tick, period, use_filter):
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (B, 7))
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    traj, meta = benchmark_traj(nominal.reset("neutral").ee_pos)
    nominal.close()
    plant = PL.BatchedPlant(B, timestep=0.001, n_substeps=5)
    plant.q, plant.v = q0.copy(), np.zeros((B, 7))
    plant.step(np.zeros((B, 7)), integrate=False)
    ff = variant == "ff"
    make = CT.ff_benchmark_config if ff else CT.classical_benchmark_config
    cfg = make(plant.dt, meta["z_contact"], horizon=HORIZON)
    cfg.mpc_update_steps, cfg.apply_command_filter = period, use_filter
    # one site calibration for both paths (calibration_obs): the same problem bit for bit
    obs_cal = PL.observation_from_record(plant.obs[0])
    Scalar = CT.ForceFeedbackCrocoddylMPC if ff else CT.ClassicalCrocoddylMPC
    scal = []
    for b in range(B):
        sim = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
        sim.set_state(q0[b])
        assert sim.dt == cfg.dt  # the filter's rate limit uses the control period
        scal.append((sim, Scalar(sim=sim, traj_fn=traj, config=cfg, calibration_obs=obs_cal)))
    Rs, p_off = FL.site_calibration(obs_cal)
    kw = dict(q_nom=q0, R_site_from_pin_ee=Rs, p_site_minus_frame_pin=p_off)
    if ff:
        fleet = FL.FleetForceFeedbackMPC(B, traj, cfg, tau0=np.zeros((B, 7)), **kw)
    else:
        fleet = FL.FleetClassicalMPC(B, traj, cfg, tau0=plant.obs[:, 14:21], device_tick=device_tick, **kw)
    t = T_START
    tau_prev = np.zeros((B, 7))  # ff: the measured torque state, the previous command
    solved, surf = np.zeros((TICKS, B), bool), np.zeros((TICKS, B), bool)
    for tick in range(TICKS):
        rec = plant.obs.copy()
        fn = rec[:, 46] * (rec[:, 47] > 0.5)
        if ff:
            tau_f = fleet.compute_control(rec[:, 0:7], rec[:, 7:14], tau_prev, rec[:, 14:21], fn, rec[:, 30], t)
        else:
            tau_f = fleet.compute_control(rec[:, 0:7], rec[:, 7:14], rec[:, 14:21], fn, rec[:, 30], t)
        fi = fleet.last_info
        solved[tick], surf[tick] = fi["solved_now"], fi["surface_mode"]
        for b in range(B):
            obs = PL.observation_from_record(rec[b], tau_cmd=tau_prev[b]) if ff else PL.observation_from_record(rec[b])
            tau_s = scal[b][1].compute_control(obs, t)
            info = scal[b][1].last_info
            tag = (variant, device_tick, period, tick, b)
            assert np.array_equal(tau_f[b], tau_s), (tag, tau_f[b] - tau_s)
            assert bool(fi["ok"][b]) == bool(info["ok"]) and int(fi["iters"][b]) == int(info["iters"]), tag
            assert np.array_equal(fi["cost"][b], info["cost"], equal_nan=True), tag
            assert bool(fi["surface_mode"][b]) == bool(info["surface_mode"]), tag
            assert bool(fi["unstable"][b]) == bool(info["unstable"]), tag
            assert bool(fi["solved_now"][b]) == bool(info["solved_now"]), tag
            assert int(fi["policy_idx"][b]) == int(info["policy_idx"]), tag
            assert int(fi["neg_accepted"][b]) == int(info["neg_accepted"]), tag
            # force feedback: the fleet does not run the logged prediction's regression (fleet.py)
            key = "fn_pred_raw" if ff else "fn_pred"
            assert np.array_equal(fi[key][b], info[key], equal_nan=True), tag
        plant.step(tau_f)
        tau_prev = tau_f.copy()
        t += plant.dt
    # the schedule was exercised: both values, and a solve off the period grid (the mode switch)
    assert solved.any() and not solved.all()
    assert solved[0].all()
    switch = int(np.flatnonzero(np.diff(surf.astype(int), axis=0).any(1))[0]) + 1  # the first tick in the new mode
    assert solved[switch].all()
    off_grid = solved & ((np.arange(TICKS) % period) != 0)[:, None]
    if period == 3 or switch % period != 0:
        assert off_grid[switch].all()
    for sim, c in scal:
        c.close()
        sim.close()
    fleet.close()
    plant.close()
