"""GPU: the force-feedback fleet controller (B instances, one batched device
solve per tick, the tick's glue in the library's fleet kernels) against B
copies of the B = 1 ForceFeedbackCrocoddylMPC fed the same observations; the
classical fleet's device tick against its default tick; and a short
force-feedback sweep whose recorded instances a scalar controller replays."""
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


def _start(B, seed=4):
    rng = np.random.default_rng(seed)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (B, 7))
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    traj, meta = benchmark_traj(obs_n.ee_pos)
    nominal.close()
    plant = PL.BatchedPlant(B, timestep=0.001, n_substeps=5)
    plant.q, plant.v = q0.copy(), np.zeros((B, 7))
    plant.step(np.zeros((B, 7)), integrate=False)
    return q0, traj, meta, plant


@pytest.mark.parametrize("phase_source", ["trajectory", "force_latch"])
def test_ff_fleet_matches_scalar_controllers(phase_source):
    B, ticks = 3, 40
    q0, traj, meta, plant = _start(B)
    t_start = 0.7  # just before contact onset: exercises the mode switch and the contact model
    cfg = CT.ff_benchmark_config(plant.dt, meta["z_contact"], phase_source=phase_source)
    # one site calibration for the fleet, passed to the scalar controllers
    # (calibration_obs), so both paths build the same problem bit for bit
    obs_cal = PL.observation_from_record(plant.obs[0])
    scal = []
    for b in range(B):
        sim = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
        sim.set_state(q0[b])
        scal.append((sim, CT.ForceFeedbackCrocoddylMPC(sim=sim, traj_fn=traj, config=cfg, calibration_obs=obs_cal)))
    Rs, p_off = FL.site_calibration(obs_cal)
    fleet = FL.FleetForceFeedbackMPC(B, traj, cfg, q_nom=q0, tau0=np.zeros((B, 7)), R_site_from_pin_ee=Rs,
                                     p_site_minus_frame_pin=p_off)
    assert np.array_equal(fleet.R_des, scal[1][1].R_des)
    t = t_start
    tau_prev = np.zeros((B, 7))  # the measured torque state: the previous command, zeros at first
    for tick in range(ticks):
        rec = plant.obs.copy()
        fn = rec[:, 46] * (rec[:, 47] > 0.5)
        tau_f = fleet.compute_control(rec[:, 0:7], rec[:, 7:14], tau_prev, rec[:, 14:21], fn, rec[:, 30], t)
        fi = fleet.last_info
        assert np.array_equal(fi["fn_pred"], fi["fn_pred_raw"], equal_nan=True) and "tau_des_inf" in fi
        for b in range(B):
            tau_s = scal[b][1].compute_control(PL.observation_from_record(rec[b], tau_cmd=tau_prev[b]), t)
            info = scal[b][1].last_info
            tag = (phase_source, tick, b)
            assert bool(fi["ok"][b]) == bool(info["ok"]), tag
            assert int(fi["iters"][b]) == int(info["iters"]), tag
            assert bool(fi["surface_mode"][b]) == bool(info["surface_mode"]), tag
            assert bool(fi["unstable"][b]) == bool(info["unstable"]), tag
            assert np.array_equal(fi["cost"][b], info["cost"], equal_nan=True), tag
            assert np.array_equal(fi["fn_pred_raw"][b], info["fn_pred_raw"], equal_nan=True), tag
            assert np.array_equal(tau_f[b], tau_s), (tag, tau_f[b] - tau_s)
        plant.step(tau_f)
        tau_prev = tau_f.copy()
        t += plant.dt
    for sim, c in scal:
        c.close()
        sim.close()
    fleet.close()
    plant.close()


def test_classical_device_tick_bit_identical():
    B, ticks = 3, 40
    q0, traj, meta, plant = _start(B)
    cfg = CT.classical_benchmark_config(plant.dt, meta["z_contact"], phase_source="force_latch")
    Rs, p_off = FL.site_calibration(PL.observation_from_record(plant.obs[0]))
    mk = lambda **kw: FL.FleetClassicalMPC(B, traj, cfg, q_nom=q0, tau0=plant.obs[:, 14:21], R_site_from_pin_ee=Rs,  # noqa: E731
                                           p_site_minus_frame_pin=p_off, **kw)
    ref, dev = mk(), mk(device_tick=True)
    assert ref.device_tick is False and dev.device_tick is True
    t = 0.7
    for tick in range(ticks):
        rec = plant.obs.copy()
        fn = rec[:, 46] * (rec[:, 47] > 0.5)
        args = (rec[:, 0:7], rec[:, 7:14], rec[:, 14:21], fn, rec[:, 30], t)
        tau_r, tau_d = ref.compute_control(*args), dev.compute_control(*args)
        assert np.array_equal(tau_r, tau_d), (tick, tau_r - tau_d)
        assert set(ref.last_info) == set(dev.last_info)
        for k, v in ref.last_info.items():
            assert np.array_equal(v, dev.last_info[k], equal_nan=True), (tick, k)
        assert np.array_equal(ref.valid, dev.valid), tick
        plant.step(tau_r)
        t += plant.dt
    ref.close()
    dev.close()
    plant.close()


def test_ff_sweep_short():
    out = FL.run_sweep(variant="ff", seeds=2, total_time=1.2, verbose=False, record=(0, 9))
    assert out["instances"] == 10 and out["ticks"] == 240
    assert np.all(np.isfinite(out["per_instance"]["rms_3d_error"]))
    assert [str(out["names"][i]) for i in (0, 9)] == ["flat", "actuation_uncertainty"]
    r = out["record"]
    assert np.all(np.isfinite(r["tau"])) and r["tau_hat"].shape == r["tau"].shape
    # the injected instance's torque measurement is noisy from the first tick, the plain one's filter starts at zero
    assert np.all(r["tau_hat"][0, 0] == 0.0) and np.all(r["tau_hat"][0, 1] != 0.0)
    for j, b in enumerate(r["index"]):
        sim = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
        sim.set_state(r["q0"][j])
        ctrl = CT.ForceFeedbackCrocoddylMPC(sim=sim, traj_fn=r["traj"], config=r["config"],
                                            calibration_obs=r["calibration_obs"])
        for k in range(out["ticks"]):
            # tau_cmd = the recorded tau_hat: observation_from_record puts it in tau_meas_act_filt,
            # the state source of the benchmark configuration
            obs = PL.observation_from_record(r["obs"][k, j], tau_cmd=r["tau_hat"][k, j])
            tau_s = ctrl.compute_control(obs, float(r["t"][k]))
            assert np.array_equal(r["tau"][k, j], tau_s), (f"instance {b} tick {k}", r["tau"][k, j] - tau_s)
        ctrl.close()
        sim.close()
