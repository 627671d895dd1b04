"""GPU: DeviceFleetLoop against the host fleets, tick by tick.

Before each tick the loop's controller state is copied into a host fleet
(FleetClassicalMPC(device_tick=True) / FleetForceFeedbackMPC), which is then
fed the observation the device tick saw, with the device tick's gravity torque
reference in place of the host one.  With those two substitutions the solve's
inputs are bit-identical, so everything but the torques must be equal exactly;
the torques differ by the order of summation inside the policy's dot products,
bounded per entry by 64 * 2^-53 * S / d (tests/test_gpu_fleet_loop_kernels.py).
A second test: a run is reproducible, and tick() equals run()."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_fleet_loop_kernels as KT  # noqa: E402  (the numpy restatement and the bound)
from ffddp import _abi  # noqa: E402
from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp.fleet_loop import DeviceFleetLoop  # noqa: E402
from ffddp.trajectory import benchmark_traj  # noqa: E402

B, HORIZON, TICKS, T0 = 6, 8, 40, 0.7  # the contact hint flips at t = 0.8: tick 20 of the window


def _setup(variant, phase_source):
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (B, 7))
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    traj, meta = benchmark_traj(obs_n.ee_pos)
    cal = FL.site_calibration(obs_n)
    dt = nominal.dt
    nominal.close()
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    cfg = make(dt, meta["z_contact"], horizon=HORIZON, phase_source=phase_source)
    tilt = np.array([0.0, 5.0, 10.0, 15.0, -5.0, 2.5])
    scale = np.array([1.0, 0.9, 1.1, 0.95, 1.05, 1.0])[:, None] * np.linspace(0.95, 1.05, 7)
    loop = DeviceFleetLoop(variant, B, traj, cfg, q0, tilt_deg=tilt, torque_scale=scale, steps=TICKS, calibration=cal,
                           t0=T0)
    return loop, traj, cfg, q0, cal


def _close(a, b, tol):
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


@pytest.mark.parametrize("variant,phase_source", [("classical", "trajectory"), ("ff", "trajectory"),
                                                  ("classical", "force_latch")])
def test_device_loop_matches_host_fleet_tick_by_tick(variant, phase_source):
    loop, traj, cfg, q0, (Rs, p_off) = _setup(variant, phase_source)
    kw = dict(q_nom=q0, tau0=np.zeros((B, 7)), R_site_from_pin_ee=Rs, p_site_minus_frame_pin=p_off)
    host = (FL.FleetForceFeedbackMPC(B, traj, cfg, **kw) if variant == "ff"
            else FL.FleetClassicalMPC(B, traj, cfg, device_tick=True, **kw))
    P = loop.params
    n_drop = n_cold = 0
    for k in range(TICKS):
        s = loop.state()
        host.valid, host.latched = s["valid"].astype(bool), s["latched"].astype(bool)
        host.loss_count, host.prev_mode = s["loss_count"].astype(np.int64), s["prev_mode"].copy()
        host.tau_prev = s["tau_prev"].copy()
        for name in ("keep_xs", "keep_us", "keep_K"):
            getattr(host, name).copy_(loop.S[name])  # device to device
        loop.tick()
        t = float(loop.times[k])
        obs = loop.P["obs"].cpu().numpy()  # what tick k saw: the plant steps at the start of tick k + 1
        T = {n: loop.T[n].cpu().numpy() for n in ("x0", "inst_ref", "xs_init", "surface", "xs", "us", "K", "cost",
                                                  "fn_pred", "tau_cmd")}
        host._tau_ref = lambda q, g=T["inst_ref"][:, 14:21]: g.copy()
        fn = obs[:, 46] * (obs[:, 47] > 0.5)
        if variant == "ff":
            tau_h = host.compute_control(obs[:, 0:7], obs[:, 7:14], T["x0"][:, 14:21], obs[:, 14:21], fn, obs[:, 30], t)
        else:
            tau_h = host.compute_control(obs[:, 0:7], obs[:, 7:14], obs[:, 14:21], fn, obs[:, 30], t)
        hi = host.last_info
        row_k = loop.log_info[k].cpu().numpy()
        info = {n: row_k[:, i] for i, n in enumerate(_abi.FLEET_INFO_FIELDS)}
        tag = (variant, phase_source, k)
        # the solve's inputs were the same bits, so:
        assert np.array_equal(host._tk["t"]["x0"].cpu().numpy(), T["x0"]), tag
        assert np.array_equal(host.T["xs_init"].cpu().numpy(), T["xs_init"]), tag
        assert np.array_equal(info["cost"], hi["cost"], equal_nan=True), tag
        assert np.array_equal(info["iters"], hi["iters"]) and np.array_equal(info["ok"] != 0, hi["ok"]), tag
        fin_h = torch.isfinite(host.T["us"][:, 0]).all(1).cpu().numpy()
        assert np.array_equal(info["fin"] != 0, fin_h), tag
        assert np.array_equal(info["surface"] != 0, hi["surface_mode"]), tag
        assert np.array_equal(info["unstable"] != 0, hi["unstable"]), tag
        assert np.array_equal(info["policy_idx"], hi["policy_idx"]), tag
        assert np.array_equal(info["neg_accepted"], hi["neg_accepted"]), tag
        assert np.array_equal(info["fn_pred"], hi["fn_pred"], equal_nan=True), tag
        for name in ("keep_xs", "keep_us", "keep_K"):
            assert torch.equal(getattr(host, name), loop.S[name]), (tag, name)
        s1 = loop.state()
        assert np.array_equal(s1["valid"].astype(bool), host.valid), tag
        assert np.array_equal(s1["latched"].astype(bool), host.latched), tag
        assert np.array_equal(s1["loss_count"], host.loss_count) and np.array_equal(s1["prev_mode"], host.prev_mode), tag
        # the torques, within the bound; S from the numpy restatement on the tick's own arrays
        st = {n: s[n].copy() for n in KT.STATE_KEYS}
        changed = (st["prev_mode"] >= 0) & ((info["surface"] != 0) != (st["prev_mode"] == 1))
        dropped = changed & (st["valid"] != 0)
        st["valid"] = (st["valid"].astype(bool) & ~changed).astype(np.uint8)  # what pre left for post
        d = {n: T[n] for n in ("xs", "us", "K", "cost", "fn_pred")}
        r = KT._post_ref(st, P, d, T["x0"], T["surface"], obs[:, 14:21], variant, HORIZON)
        pol = r["valid_policy"] & ~r["unstable"] & ~r["bad"]
        tol = np.where(pol[:, None], KT.U64 * r["S"], 0.0)
        assert np.all(np.isfinite(tol)), tag
        err = np.abs(T["tau_cmd"] - tau_h)
        assert np.all(err <= tol), (tag, float(np.max(err - tol)))
        assert np.array_equal(s1["tau_prev"], T["tau_cmd"]), tag
        raw_tol = np.where(r["valid_policy"], KT.U64 * np.nan_to_num(r["S"]).max(1), 0.0)
        assert _close(info["tau_raw_inf"], hi["tau_raw_inf"], raw_tol), tag
        assert _close(info["tau_cmd_inf"], hi["tau_cmd_inf"], tol.max(1)), tag
        if variant == "ff":
            des_tol = np.where(r["valid_policy"], KT.U64 * np.nan_to_num(r["S_des"]).max(1), 0.0)
            assert _close(info["tau_des_inf"], hi["tau_des_inf"], des_tol), tag
        # a dropped or missing warm start is a cold start: xs_init = [x0] * (N + 1)
        cold = (s["valid"] == 0) | dropped
        n_drop += int(dropped.sum())
        n_cold += int(cold.sum())
        assert np.array_equal(T["xs_init"][cold][:, 1], T["x0"][cold]), tag
    assert n_cold >= B  # every instance starts cold
    if phase_source == "trajectory":
        assert n_drop >= 1  # the hint flips inside the window
        assert len(set(loop.hints.tolist())) == 2
    host.close()
    loop.close()


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_device_loop_reproducible_and_tick_equals_run(variant):
    loop, *_ = _setup(variant, "trajectory")
    s0 = loop.state()
    logs = []
    for how in ("run", "run", "tick"):
        loop.load_state(s0)
        loop.log_info.fill_(float("nan"))
        loop.log_obs.fill_(float("nan"))
        if how == "run":
            loop.run(TICKS)
        else:
            for _ in range(TICKS):
                loop.tick()
        r = loop.results()
        assert r["info"].shape == (TICKS, B, _abi.FLEET_INFO_W) and r["obs"].shape == (TICKS + 1, B, _abi.FLEET_LOG_W)
        assert not np.any(r["plant_fail"]) and np.all(np.isfinite(r["obs"]))
        logs.append(r)
    for other in logs[1:]:
        assert np.array_equal(logs[0]["info"], other["info"], equal_nan=True)
        assert np.array_equal(logs[0]["obs"], other["obs"])
    assert np.any(logs[0]["surface"] == 1) and np.any(logs[0]["surface"] == 0)
    with pytest.raises(RuntimeError, match="sized for"):
        loop.tick()
    loop.close()


def test_device_loop_rejects_unsupported_config():
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    traj, meta = benchmark_traj(obs_n.ee_pos)
    nominal.close()
    cfg = CT.classical_benchmark_config(0.005, meta["z_contact"], horizon=HORIZON)
    cfg.mpc_update_steps = 2
    with pytest.raises(NotImplementedError):
        DeviceFleetLoop("classical", 2, traj, cfg, np.tile(R.Q_NEUTRAL, (2, 1)), steps=4)
