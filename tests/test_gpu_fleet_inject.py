"""GPU: the uncertainty injector on the device.  The two kernels alone against
BatchedUncertaintyInjector (bit for bit, mixed fleet, strided plant records),
the device Philox source against uncertainty.philox_normals, DeviceFleetLoop
with injected instances tick by tick against a host injector fed the plant's
true state, reproducibility in both noise modes, and run_sweep(device_loop=
True, device_noise=...)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_fleet_inject_cpu as CT_  # noqa: E402  (seeds, ticks, the delayed profile)
from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp import uncertainty as U  # noqa: E402
from ffddp.config import classical_preset  # noqa: E402
from ffddp.fleet_loop import DeviceFleetLoop  # noqa: E402
from ffddp.trajectory import benchmark_traj  # noqa: E402

DT = CT_.DT
# |z_dev - z_host|: r = sqrt(-2 ln u1) <= 8.6 (u1 >= 2^-53); the argument 2 pi u2 (<= 2 pi) is one rounding in
# both, the two libraries' sin / cos / log / sqrt are each within a few ulp: r * (few ulp of 1) + (few ulp of
# ln) / r -- about 2.4e-14 at the worst, below 256 * 2^-53 = 2.84e-14.  Derived, not measured.
Z_TOL = 256.0 * 2.0 ** -53


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _seed_tensor(seeds):
    return _dev(np.array([int(s) for s in seeds], dtype=np.uint64).view(np.int64))


@pytest.mark.parametrize("delays", [(2, 1), (0, 0)])
def test_inject_kernels_equal_host_class(delays):
    B, ticks, OBS_W = 5, 9, _abi.PLANT_OBS
    row = np.array([0, -1, 1, -1, 2], np.int32)
    on = row >= 0
    cfgs = [U.UncertaintyProfileConfig(seed=s, **(CT_.DELAYED if delays == (2, 1) else {})) for s in (15, 1500003, 7)]
    bat = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs)
    assert (bat.obs_delay_steps, bat.cmd_delay_steps) == delays
    a, b, z = U.predraw(cfgs, ticks)
    solver = BatchedBoxFDDP(classical_preset(2), max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    zt = _dev(z)
    obs = torch.zeros(B, OBS_W, dtype=torch.float64, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    J = dict(row=_dev(row), a=_dev(a), b=_dev(b), obs_ring=f64(delays[0] + 1, B, 14), cmd_ring=f64(delays[1] + 1, B, 7),
             tau_hat_filt=f64(B, 7), z_cmd=f64(B, 7), qv_ctrl=f64(B, 14), tau_hat=f64(B, 7), tau_ctrl=f64(B, 7),
             q=obs[:, 0:7], v=obs[:, 7:14], tau_filt=f64(B, 7), tau_cmd=f64(B, 7), tau_app=f64(B, 7))
    inj = solver.fleet_inject(J, delays[0], delays[1], bat.sig, 0.2, "numpy")
    rng = np.random.default_rng(11)
    for k in range(ticks):
        rec = rng.normal(size=(B, OBS_W))
        tau_cmd, tau_post, tau_filt = rng.normal(size=(B, 7)) * 10, rng.normal(size=(B, 7)), rng.normal(size=(B, 7))
        obs.copy_(_dev(rec))
        J["tau_filt"].copy_(_dev(tau_filt))
        solver.fleet_inject_obs_dev(J, inj, k, z=zt[k], stream=stream)
        J["tau_cmd"].copy_(_dev(tau_cmd))
        J["tau_app"].copy_(_dev(tau_post))  # what post would have written: scale * tau_cmd
        solver.fleet_inject_cmd_dev(J, inj, k, stream=stream)
        torch.cuda.synchronize()
        q, v = rec[:, 0:7], rec[:, 7:14]
        qh, vh = bat.observation_for_controller(q[on], v[on])
        th, thf = bat.tau_hat.copy(), bat.tau_hat_filt.copy()
        app = bat.command_for_plant(tau_cmd[on])
        qv, tau_hat, tau_ctrl, tau_app = (J[n].cpu().numpy() for n in ("qv_ctrl", "tau_hat", "tau_ctrl", "tau_app"))
        assert np.array_equal(qv[on, :7], qh) and np.array_equal(qv[on, 7:], vh), k
        assert np.array_equal(tau_hat[on], th) and np.array_equal(tau_ctrl[on], thf), k
        assert np.array_equal(J["tau_hat_filt"].cpu().numpy()[on], thf), k
        assert np.array_equal(tau_app[on], app), k
        # no injector: the plant's record, its torque filter, post's actuation
        assert np.array_equal(qv[~on], rec[~on, :14]), k
        assert np.array_equal(tau_hat[~on], tau_filt[~on]) and np.array_equal(tau_ctrl[~on], tau_filt[~on]), k
        assert np.array_equal(tau_app[~on], tau_post[~on]), k
        assert np.all(J["tau_hat_filt"].cpu().numpy()[~on] == 0.0) and np.all(J["obs_ring"].cpu().numpy()[:, ~on] == 0.0)
    solver.close()


def test_device_philox_equals_numpy_restatement():
    seeds, B = CT_.PHILOX_SEEDS, len(CT_.PHILOX_SEEDS)
    solver = BatchedBoxFDDP(classical_preset(2), max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    sd = _seed_tensor(seeds)
    worst = 0.0
    for k in CT_.PHILOX_TICKS:
        z = torch.full((B, 28), float("nan"), dtype=torch.float64, device="cuda")
        w = torch.zeros(B, 7, 4, dtype=torch.int64, device="cuda")
        solver.fleet_noise_dev(sd, k, z, words=w, stream=stream)
        z2 = torch.full((B, 28), float("nan"), dtype=torch.float64, device="cuda")
        solver.fleet_noise_dev(sd, k, z2, stream=stream)  # words are optional
        torch.cuda.synchronize()
        zh, wh = U.philox_normals(seeds, k, return_words=True)
        assert np.array_equal(w.cpu().numpy().view(np.uint64), wh), k
        zd = z.cpu().numpy()
        assert np.all(np.isfinite(zd)) and np.array_equal(zd, z2.cpu().numpy()), k
        worst = max(worst, float(np.max(np.abs(zd - zh))))
        print(f"tick {k}: max |z_dev - z_host| = {np.max(np.abs(zd - zh)):.3e} (bound {Z_TOL:.3e})")
        assert np.all(np.abs(zd - zh) <= Z_TOL), (k, worst)
    solver.close()


def test_inject_kernel_error_codes():
    B = 3
    solver = BatchedBoxFDDP(classical_preset(2), max_batch=B, device=0)
    lib, h = solver._lib, solver._h
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(int(buf.data_ptr()))
    row0 = torch.zeros(B, dtype=torch.int32, device="cuda")
    ptrs = ("row", "a", "b", "seed", "obs_ring", "cmd_ring", "tau_hat_filt", "z_cmd")

    def make(**kw):
        inj = _abi.FleetInject()
        for n in ptrs:
            setattr(inj, n, int((row0 if n == "row" else buf).data_ptr()))
        inj.rows = 1
        for n, v in kw.items():
            setattr(inj, n, v)
        return inj

    def obs(inj, B_=B, k=0, z=p, q=p, qv=p, ld=7, h_=h):
        return lib.ffddp_fleet_inject_obs_dev(h_, B_, C.byref(inj) if inj is not None else None, k, z, q, q, ld, None, qv,
                                              None, None, None)

    def cmd(inj, B_=B, k=0, tc=p, ta=p, h_=h):
        return lib.ffddp_fleet_inject_cmd_dev(h_, B_, C.byref(inj) if inj is not None else None, k, tc, ta, None)

    ok = make()
    assert obs(ok) == 0 and cmd(ok) == 0
    assert obs(ok, B_=B + 1) == -4 and cmd(ok, B_=B + 1) == -4 and lib.ffddp_fleet_noise_dev(h, B + 1, p, 0, p, None, None) == -4
    assert obs(ok, h_=None) == -1 and cmd(ok, h_=None) == -1 and obs(None) == -1 and cmd(None) == -1
    assert obs(ok, B_=0) == -1 and cmd(ok, k=-1) == -1 and obs(ok, ld=6) == -1
    assert obs(make(d_obs=-1)) == -1 and cmd(make(d_cmd=-1)) == -1 and obs(make(noise=2)) == -1
    assert obs(ok, z=None) == -1 and obs(ok, q=None) == -1 and obs(ok, qv=None) == -1
    assert cmd(ok, tc=None) == -1 and cmd(ok, ta=None) == -1
    assert obs(make(noise=1), z=None) == 0 and obs(make(noise=1, seed=0), z=None) == -1  # philox: seed, no table
    for n in ptrs:
        if n != "seed":
            assert obs(make(**{n: 0})) == -1 and cmd(make(**{n: 0})) == -1, n
    assert lib.ffddp_fleet_noise_dev(h, B, None, 0, p, None, None) == -1 and lib.ffddp_fleet_noise_dev(h, B, p, 0, None, None, None) == -1
    assert lib.ffddp_fleet_noise_dev(h, B, p, -1, p, None, None) == -1
    torch.cuda.synchronize()
    solver.close()


# -- the loop -----------------------------------------------------------------------------------
B, HORIZON, TICKS, T0 = 4, 8, 12, 0.7
INJECTED = (0, 2)


def _setup(variant, noise):
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
    tilt = np.array([0.0, 5.0, 10.0, -5.0])
    scale = np.array([1.0, 0.9, 1.1, 0.95])[:, None] * np.linspace(0.95, 1.05, 7)
    ucfgs = [U.UncertaintyProfileConfig(seed=100 + b, **CT_.DELAYED) if b in INJECTED else None for b in range(B)]
    loop = DeviceFleetLoop(variant, B, traj, cfg, q0, tilt_deg=tilt, torque_scale=scale, steps=TICKS, calibration=cal,
                           t0=T0, uncertainty=ucfgs, noise=noise)
    return loop, ucfgs, scale


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_device_loop_injector_tick_by_tick(variant):
    loop, ucfgs, scale = _setup(variant, "numpy")
    assert loop.dt == DT and (loop.inject.d_obs, loop.inject.d_cmd) == (2, 1)
    idx, rest = list(INJECTED), [b for b in range(B) if b not in INJECTED]
    host = U.BatchedUncertaintyInjector(dt=loop.dt, nu=7, configs=[ucfgs[b] for b in idx])
    for k in range(TICKS):
        tau_filt0 = loop.P["tau_filt"].cpu().numpy()
        loop.tick()
        obs = loop.P["obs"].cpu().numpy()  # what tick k saw: the plant steps at the start of tick k + 1
        x0, tau_cmd, tau_app = (loop.T[n].cpu().numpy() for n in ("x0", "tau_cmd", "tau_app"))
        qh, vh = host.observation_for_controller(obs[idx, 0:7], obs[idx, 7:14])
        assert np.array_equal(x0[idx, 0:7], qh) and np.array_equal(x0[idx, 7:14], vh), (variant, k)
        assert not np.array_equal(x0[idx, :14], obs[idx, :14])
        if variant == "ff":
            assert np.array_equal(x0[idx, 14:21], host.tau_hat_filt), (variant, k)
            assert np.array_equal(x0[rest, 14:21], tau_filt0[rest]), (variant, k)
        assert np.array_equal(tau_app[idx], host.command_for_plant(tau_cmd[idx])), (variant, k)
        assert np.array_equal(x0[rest, :14], obs[rest, :14]), (variant, k)
        assert np.array_equal(tau_app[rest], tau_cmd[rest] * scale[rest]), (variant, k)
        assert np.all(np.isfinite(tau_cmd))
    r = loop.results()
    assert np.array_equal(r["inject_a"][idx], host.a) and np.array_equal(r["inject_b"][idx], host.b)
    assert np.all(np.isnan(r["inject_a"][rest])) and np.all(np.isnan(r["inject_b"][rest]))
    assert not np.any(r["plant_fail"])
    loop.close()


@pytest.mark.parametrize("variant,noise", [("classical", "numpy"), ("classical", "philox"), ("ff", "numpy"), ("ff", "philox")])
def test_device_loop_injector_reproducible_and_tick_equals_run(variant, noise):
    loop, *_ = _setup(variant, noise)
    s0 = loop.state()
    assert all(n in s0 for n in ("obs_ring", "cmd_ring", "tau_hat_filt", "z_cmd"))
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
        r["x0"], r["tau_app"] = loop.T["x0"].cpu().numpy(), loop.T["tau_app"].cpu().numpy()
        assert not np.any(r["plant_fail"]) and np.all(np.isfinite(r["obs"])) and np.all(np.isfinite(r["info"][..., 1]))
        logs.append(r)
    for other in logs[1:]:
        assert np.array_equal(logs[0]["info"], other["info"], equal_nan=True)
        assert np.array_equal(logs[0]["obs"], other["obs"])
        assert np.array_equal(logs[0]["x0"], other["x0"]) and np.array_equal(logs[0]["tau_app"], other["tau_app"])
    loop.close()


@pytest.mark.parametrize("noise", ["numpy", "philox"])
def test_device_loop_sweep_with_injector(noise):
    """0.1 s ends before the contact phase (t >= 0.8 s), so the three statistics
    over that phase are NaN by definition (runlog.summary_metrics on an empty
    phase), as on the host path; every other one must be finite."""
    kw = dict(scenarios=("flat", "actuation_uncertainty"), seeds=2, total_time=0.1, verbose=False, device_loop=True,
              device_noise=noise)
    a = FL.run_sweep(**kw)
    b = FL.run_sweep(**kw)
    assert set(a["per_instance"]) == set(FL.SUMMARY_KEYS) and a["ticks"] == 20 and a["instances"] == a["n_all"] == 4
    assert list(a["names"]) == ["flat", "flat", "actuation_uncertainty", "actuation_uncertainty"]
    undefined = {"rms_tangential_error_contact_phase", "contact_loss_contact_phase_pct", "fn_mean_contact_phase"}
    for k in FL.SUMMARY_KEYS:
        va = a["per_instance"][k]
        assert va.shape == (4,), k
        assert np.all(np.isnan(va)) if k in undefined else np.all(np.isfinite(va)), (k, va)
        assert np.array_equal(va, b["per_instance"][k], equal_nan=True), k
    host = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=[U.config_for_scenario("actuation_uncertainty", seed=int(s))
                                                              for s in a["seed"][2:]])
    for key, want in (("inject_a", host.a), ("inject_b", host.b)):
        assert np.all(np.isnan(a[key][:2])) and np.array_equal(a[key][2:], want), key
        assert np.array_equal(a[key], b[key], equal_nan=True)
    assert FL.gather_summaries(a, a["n_all"]).shape == (4, len(FL.SUMMARY_KEYS))
