"""GPU: DeviceFleetLoop with a solve period and the command filter against the
host fleets, tick by tick, by tests/test_gpu_fleet_loop.py's scheme: before
each tick the loop's controller state -- with the scheduled tick's counters
since and age -- is copied into a host fleet, which is then fed the
observation the device tick saw and the device's gravity torque reference.
The solve's inputs are then the same bits, so everything but the torques is
exact; the torques get the dot-product bound of
tests/test_gpu_fleet_loop_kernels.py, which the filter's 1-Lipschitz clips and
smoothing carry through.  Also: a run is reproducible and tick() equals run(),
the state round trip in the middle of a period, and short scheduled sweeps."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_fleet_loop_kernels as KT  # noqa: E402  (the bound)
from ffddp import _abi  # noqa: E402
from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp.fleet_loop import DeviceFleetLoop  # noqa: E402
from ffddp.trajectory import benchmark_traj  # noqa: E402

B, HORIZON, TICKS, T0, PERIOD = 6, 8, 40, 0.7, 3  # the contact hint flips at t = 0.8, inside the window


def _setup(variant, use_filter=True, period=PERIOD):
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (B, 7))
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    traj, meta = benchmark_traj(obs_n.ee_pos)
    cal = FL.site_calibration(obs_n)
    dt = nominal.dt
    nominal.close()
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    cfg = make(dt, meta["z_contact"], horizon=HORIZON)
    cfg.apply_command_filter = use_filter
    tilt = np.array([0.0, 5.0, 10.0, 15.0, -5.0, 2.5])
    scale = np.array([1.0, 0.9, 1.1, 0.95, 1.05, 1.0])[:, None] * np.linspace(0.95, 1.05, 7)
    loop = DeviceFleetLoop(variant, B, traj, cfg, q0, tilt_deg=tilt, torque_scale=scale, steps=TICKS, calibration=cal,
                           t0=T0, solve_period=period)
    return loop, traj, cfg, q0, cal


def _close(a, b, tol):
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)))


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_scheduled_device_loop_matches_host_fleet_tick_by_tick(variant):
    import copy

    loop, traj, cfg, q0, (Rs, p_off) = _setup(variant)
    assert loop.period == PERIOD and loop.sched is not None
    hcfg = copy.copy(cfg)
    hcfg.mpc_update_steps = PERIOD  # the host fleets take the period from the configuration
    kw = dict(q_nom=q0, tau0=np.zeros((B, 7)), R_site_from_pin_ee=Rs, p_site_minus_frame_pin=p_off)
    host = FL.FleetForceFeedbackMPC(B, traj, hcfg, **kw) if variant == "ff" else FL.FleetClassicalMPC(B, traj, hcfg, **kw)
    lim = np.asarray(cfg.tau_limits, float)
    n_filtered = 0
    for k in range(TICKS):
        s = loop.state()
        host.valid, host.latched = s["valid"].astype(bool), s["latched"].astype(bool)
        host.loss_count, host.prev_mode = s["loss_count"].astype(np.int64), s["prev_mode"].copy()
        host.tau_prev = s["tau_prev"].copy()
        host.since, host.age = s["since"].copy(), s["age"].copy()
        for name in ("keep_xs", "keep_us", "keep_K"):
            getattr(host, name).copy_(loop.S[name])  # device to device: the kept arrays are never moved
        loop.tick()
        t = float(loop.times[k])
        obs = loop.P["obs"].cpu().numpy()
        T = {n: loop.T[n].cpu().numpy() for n in ("x0", "inst_ref", "xs_init", "us_init", "tau_cmd")}
        need = loop.log_need[k].cpu().numpy() != 0
        host._tau_ref = lambda q, g=T["inst_ref"][:, 14:21]: g.copy()
        fn = obs[:, 46] * (obs[:, 47] > 0.5)
        if variant == "ff":
            tau_h = host.compute_control(obs[:, 0:7], obs[:, 7:14], T["x0"][:, 14:21], obs[:, 14:21], fn, obs[:, 30], t)
        else:
            tau_h = host.compute_control(obs[:, 0:7], obs[:, 7:14], obs[:, 14:21], fn, obs[:, 30], t)
        hi = host.last_info
        row_k = loop.log_info[k].cpu().numpy()
        info = {n: row_k[:, i] for i, n in enumerate(_abi.FLEET_INFO_FIELDS)}
        tag = (variant, k)
        assert np.array_equal(need, hi["solved_now"]), tag
        # the solving instances' inputs were the same bits, so:
        assert np.array_equal(host.T["x0"].cpu().numpy(), T["x0"]), tag
        assert np.array_equal(host.T["xs_init"].cpu().numpy()[need], T["xs_init"][need]), tag
        assert np.array_equal(host.T["us_init"].cpu().numpy()[need], T["us_init"][need]), tag
        assert np.array_equal(info["cost"], hi["cost"], equal_nan=True), tag
        assert np.array_equal(info["iters"], hi["iters"]) and np.array_equal(info["ok"] != 0, hi["ok"]), tag
        assert np.array_equal(info["surface"] != 0, hi["surface_mode"]), tag
        assert np.array_equal(info["unstable"] != 0, hi["unstable"]), tag
        assert np.array_equal(info["policy_idx"], hi["policy_idx"]), tag
        assert np.array_equal(info["neg_accepted"], hi["neg_accepted"]), tag
        assert np.array_equal(info["fn_pred"], hi["fn_pred"], equal_nan=True), tag
        assert not np.any((info["fin"] != 0) & ~need), tag
        for name in ("keep_xs", "keep_us", "keep_K"):
            assert torch.equal(getattr(host, name), loop.S[name]), (tag, name)
        s1 = loop.state()
        assert np.array_equal(s1["valid"].astype(bool), host.valid), tag
        assert np.array_equal(s1["latched"].astype(bool), host.latched), tag
        assert np.array_equal(s1["loss_count"], host.loss_count) and np.array_equal(s1["prev_mode"], host.prev_mode), tag
        assert np.array_equal(s1["since"], host.since) and np.array_equal(s1["age"], host.age), tag
        assert s1["since"].dtype == np.int32 and s1["age"].dtype == np.int32
        # the torques within the dot-product bound: S = the sum of |terms| of the policy entry, from the
        # knot the policy read (through the age after this tick's keep); exact where no policy ran
        a = np.minimum(np.where(need, s1["age"], s1["age"] - 1), HORIZON)
        ar = np.arange(B)
        kx = {n: loop.S[n].cpu().numpy() for n in ("keep_xs", "keep_us", "keep_K")}
        st = dict(valid=(info["policy_idx"] == 0).astype(np.uint8), tau_prev=s["tau_prev"].copy(),
                  keep_xs=np.stack([kx["keep_xs"][ar, a], kx["keep_xs"][ar, np.minimum(a + 1, HORIZON)]], 1),
                  keep_us=kx["keep_us"][ar, np.minimum(a, HORIZON - 1)][:, None],
                  keep_K=kx["keep_K"][ar, np.minimum(a, HORIZON - 1)][:, None])
        nothing = dict(xs=np.zeros_like(st["keep_xs"]), us=np.full_like(st["keep_us"], np.nan),
                       K=np.zeros_like(st["keep_K"]), cost=info["cost"], fn_pred=loop.T["fn_pred"].cpu().numpy())
        surface = (info["surface"] != 0).astype(np.uint8)
        r = KT._post_ref(st, loop.params, nothing, T["x0"], surface, obs[:, 14:21], variant, HORIZON)
        pol = r["valid_policy"] & ~r["unstable"] & ~r["bad"]
        tol = np.where(pol[:, None], KT.U64 * r["S"], 0.0)
        assert np.all(np.isfinite(tol)), tag
        err = np.abs(T["tau_cmd"] - tau_h)
        assert np.all(err <= tol), (tag, float(np.max(err - tol)))
        assert np.array_equal(s1["tau_prev"], T["tau_cmd"]), tag
        raw_tol = np.where(r["valid_policy"], KT.U64 * np.nan_to_num(r["S"]).max(1), 0.0)
        assert _close(info["tau_raw_inf"], hi["tau_raw_inf"], raw_tol), tag
        assert _close(info["tau_cmd_inf"], hi["tau_cmd_inf"], tol.max(1)), tag
        # the filter changed the command: it differs from the clipped policy torque
        n_filtered += int(np.any(np.abs(T["tau_cmd"] - np.clip(r["unclipped"], -lim, lim)) > tol + 1e-9))
    res = loop.results()
    assert res["solved"].shape == (TICKS, B) and res["solved"].dtype == bool
    assert res["solved"][0].all() and not res["solved"].all()
    assert (res["solved"] & ((np.arange(TICKS) % PERIOD) != 0)[:, None]).any()  # off the period grid: the mode switch
    assert n_filtered > 0
    host.close()
    loop.close()


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_scheduled_loop_reproducible_tick_equals_run_and_state_round_trip(variant):
    loop, *_ = _setup(variant)
    s0 = loop.state()
    assert set(("since", "age")) <= set(s0)
    logs, mid = [], None
    for how in ("run", "run", "tick", "resume"):
        loop.load_state(s0 if how != "resume" else mid)
        if how != "resume":
            loop.log_info.fill_(float("nan"))
            loop.log_obs.fill_(float("nan"))
            loop.log_need.fill_(7)
        if how == "run":
            loop.run(TICKS)
        elif how == "tick":
            for k in range(TICKS):
                loop.tick()
                if k == 13:  # the middle of a period for the instances on the grid (13 % 3 == 1)
                    mid = loop.state()
        else:  # from the saved state, over the logs of the run before: the later rows are rewritten
            assert mid["k"] == 14 and np.any(mid["since"] > 0) and np.any(mid["age"] > 0)
            loop.log_info[14:].fill_(float("nan"))
            loop.log_need[14:].fill_(7)
            loop.run(TICKS - 14)
        r = loop.results()
        assert r["info"].shape == (TICKS, B, _abi.FLEET_INFO_W) and r["solved"].shape == (TICKS, B)
        assert not np.any(r["plant_fail"]) and np.all(np.isfinite(r["obs"]))
        logs.append(r)
    for how, other in zip(("run", "tick", "resume"), logs[1:]):
        assert np.array_equal(logs[0]["info"], other["info"], equal_nan=True), how
        assert np.array_equal(logs[0]["obs"], other["obs"]), how
        assert np.array_equal(logs[0]["solved"], other["solved"]), how
    assert logs[0]["solved"].any() and not logs[0]["solved"].all()
    loop.close()


def test_period_one_without_filter_is_the_unscheduled_loop():
    """solve_period = 1 and no filter enqueue the unscheduled calls: same logs as no argument at all."""
    logs = []
    for period in (None, 1):
        loop, *_ = _setup("classical", use_filter=False, period=period)
        assert loop.sched is None
        loop.run(10)
        logs.append(loop.results())
        loop.close()
    assert np.array_equal(logs[0]["info"], logs[1]["info"], equal_nan=True)
    assert logs[1]["solved"].all() and logs[1]["solved"].shape == (10, B)


@pytest.mark.parametrize("noise", [None, "philox"])
def test_scheduled_sweep_short(noise):
    """0.1 s is 20 ticks: the contact phase (from t = 0.8) is not reached, so its
    three statistics are NaN, as in tests/test_gpu_fleet_loop_sweep.py."""
    scen = ("flat", "tilted_10") if noise is None else ("flat", "actuation_uncertainty")
    out = FL.run_sweep(scenarios=scen, seeds=2, total_time=0.1, verbose=False, device_loop=True, solve_period=2,
                       device_noise=noise)
    assert out["instances"] == 4 and out["ticks"] == 20
    nan_keys = ("rms_tangential_error_contact_phase", "contact_loss_contact_phase_pct", "fn_mean_contact_phase")
    for k, v in out["per_instance"].items():
        assert v.shape == (4,)
        assert np.all(np.isnan(v)) if k in nan_keys else np.all(np.isfinite(v)), k
    st = out["solved_ticks"]
    assert st.shape == (4,) and np.all(st >= 10) and np.all(st < 20)
