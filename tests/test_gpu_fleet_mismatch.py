"""GPU: per-instance plant physics and uncertainty profiles.  The plant kernel
with one physics row per instance against oracle/plant.py (one prm dict per
instance), the handle's plumbing (rows equal to the struct, back to the struct,
refusals), the per-row injector kernels alone against the mixed host class,
DeviceFleetLoop with mixed profiles and mixed plant rows tick by tick, and
run_sweep(plant_spread=..., uncertainty_spread=...) on both paths."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_fleet_mismatch_cpu as CM  # noqa: E402  (the mixed configs, the per-row kernels' restatement)
from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp import uncertainty as U  # noqa: E402
from ffddp.config import classical_preset  # noqa: E402
from ffddp.fleet_loop import DeviceFleetLoop  # noqa: E402
from ffddp.trajectory import benchmark_traj  # noqa: E402
from oracle import plant as OP  # noqa: E402
from test_closed_loop import _contact_pose  # noqa: E402
from test_gpu_fleet_inject import Z_TOL  # noqa: E402

DT = CM.DT


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# -- the plant kernel against the oracle ------------------------------------------------------------
PLANT_B = 70  # two 64-thread blocks, the second with a tail


def _plant_inputs(seed: int, B: int = PLANT_B):
    """test_gpu_plant._states' recipe, the contact-pose noise 0.0004 for b % 4 == 0 and 0.004 for b % 4 == 2
    (shallow and deep penetrations: every impedance branch), then one physics row per instance from the same
    generator."""
    rng = np.random.default_rng(seed)
    q0 = _contact_pose()
    qs, vs, taus, tilts = [], [], [], []
    for b in range(B):
        if b % 2 == 0:
            q = q0 + rng.normal(scale=0.0004 if b % 4 == 0 else 0.004, size=7)
        else:
            q = np.array([0.0, -0.758, 0.0, -2.22, 0.0, 1.43, 0.0]) + rng.uniform(-0.3, 0.3, 7)
        qs.append(q)
        vs.append(rng.normal(scale=0.2, size=7))
        taus.append(rng.normal(scale=5.0, size=7))
        tilts.append([0.0, 5.0, 10.0, 15.0][b % 4])
    phys = []
    for b in range(B):
        arm, damp = rng.uniform(0.05, 0.2, 7), rng.uniform(0.5, 2.0, 7)
        r_tool, margin = 0.03 + rng.uniform(-0.002, 0.002), rng.uniform(0.0005, 0.002)
        solref = (rng.uniform(0.01, 0.04), rng.uniform(0.7, 1.3))
        d0 = rng.uniform(0.80, 0.94)
        solimp = (d0, rng.uniform(d0 + 0.01, 0.99), rng.uniform(0.001, 0.006), rng.uniform(0.3, 0.7),
                  float([1, 2, 3][b % 3]))
        phys.append(PL.PlantPhysics(armature=arm, damping=damp, r_tool=r_tool, margin=margin, solref=solref,
                                    solimp=solimp))
    return np.array(qs), np.array(vs), np.array(taus), np.array(tilts), phys


@functools.lru_cache(maxsize=None)
def _plant_case(seed: int, integrate: bool):
    """The inputs and the oracle's step of every instance with its own prm dict, computed once; and, from the
    oracle's side, the instances in contact and their impedance branch: saturated (x >= 1), power 1, x <= mid,
    x > mid, with x = |dist - margin| / width at the forward pass the record describes."""
    q, v, tau, tilt, phys = _plant_inputs(seed)
    ref, branches, fmax, finite = [], [0, 0, 0, 0], 0.0, True
    for b, p in enumerate(phys):
        prm = OP.default_params(0.001, 5)
        prm.update(armature=np.asarray(p.armature, float), damping=np.asarray(p.damping, float), r_tool=p.r_tool,
                   margin=p.margin, solref=p.solref, solimp=p.solimp)
        n, p0 = PL.table_plane(tilt[b])
        qo, vo, o = OP.step(prm, q[b], v[b], tau[b], n, p0, integrate=integrate)
        ref.append((qo, vo, o))
        finite = finite and all(np.all(np.isfinite(np.asarray(x, float))) for x in (qo, vo, *o.values()))
        if o["ncon"]:
            fmax = max(fmax, float(o["fn"]))
            d0, dmax, width, mid, pw = p.solimp
            x = abs(float(n @ (o["ee_pos"] - p0)) - p.r_tool - p.margin) / width
            branches[3 if x >= 1.0 else 0 if pw == 1.0 else 1 if x <= mid else 2] += 1
    return dict(q=q, v=v, tau=tau, tilt=tilt, phys=phys, ref=ref, ncon=sum(branches), branches=tuple(branches),
                fmax=fmax, finite=finite)


@pytest.mark.parametrize("integrate", [False, True])
def test_plant_rows_kernel_matches_oracle(integrate):
    """Tolerances: tests/test_gpu_plant.py's.  With the rows drawn instance by instance in the order of
    _plant_inputs the oracle alone gives, for default_rng(3), 35 (forward only) and 34 (integrated) instances in
    contact, branch counts (power 1, x <= mid, x > mid, saturated) (3, 6, 4, 22) and (2, 6, 2, 24), everything
    finite and forces up to 650 N; default_rng(5) and (7) give 32-34 in contact and at least 2 per branch too."""
    case = _plant_case(3, integrate)
    B = PLANT_B
    print(f"integrate={integrate}: in contact {case['ncon']}, branches {case['branches']}, max force {case['fmax']:.1f} N")
    assert case["finite"] and case["ncon"] >= 8 and min(case["branches"]) >= 2, (case["ncon"], case["branches"])
    bp = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, physics=case["phys"])
    bp.q, bp.v = case["q"].copy(), case["v"].copy()
    bp.set_tilt(case["tilt"])
    obs = bp.step(case["tau"], integrate=integrate).copy()
    for b in range(B):
        qo, vo, o = case["ref"][b]
        np.testing.assert_allclose(bp.q[b], qo, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(bp.v[b], vo, rtol=1e-10, atol=1e-10)
        r = obs[b]
        np.testing.assert_allclose(r[0:7], qo, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r[14:21], o["bias"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(r[21:28], o["tau_c"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r[28:31], o["ee_pos"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r[31:34], o["ee_vel"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(r[34:43].reshape(3, 3), o["ee_R"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r[43:46], o["f_world"], rtol=1e-9, atol=1e-9)
        assert r[46] == pytest.approx(o["fn"], rel=1e-9, abs=1e-9), b
        assert r[47] == o["ncon"], b
        np.testing.assert_allclose(r[48:69].reshape(3, 7), o["J"], rtol=1e-12, atol=1e-12)
    bp.close()


def test_plant_rows_plumbing():
    B = 12
    q, v, tau, tilt, phys = _plant_inputs(5, B)

    def step(bp, n=B):
        bp.q, bp.v = q[:n].copy(), v[:n].copy()
        bp.set_tilt(tilt[:n])
        return bp.step(tau[:n]).copy(), bp.q.copy(), bp.v.copy()

    plain = PL.BatchedPlant(B, timestep=0.001, n_substeps=5)
    ref = step(plain)
    assert plain.physics is None and np.any(ref[0][:, 47] == 1.0)
    # rows all equal to the handle's struct: the same bits as no rows
    bp = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, physics=[PL.PlantPhysics()] * B)
    assert bp.physics.shape == (B, _abi.PLANT_ROW_W)
    for got, want in zip(step(bp), ref):
        assert np.array_equal(got, want)
    # other rows move the result; an invalid row is refused and the previous rows stay in force
    bp.set_physics(phys)
    mixed = step(bp)
    assert not np.array_equal(mixed[0], ref[0])
    bad = PL.plant_rows(phys)
    bad[7, _abi.PLANT_ROW_SOLREF] = 0.0
    with pytest.raises(ValueError, match="plant rows"):
        bp.set_physics(bad)
    assert bp.lib.ffddp_plant_set_instance_params(bp._h, B, _abi.dptr(bad)) == -1
    bad[7, _abi.PLANT_ROW_SOLREF] = np.nan
    assert bp.lib.ffddp_plant_set_instance_params(bp._h, B, _abi.dptr(bad)) == -1
    with pytest.raises(ValueError, match="rows for"):
        bp.set_physics(phys[:5])
    for got, want in zip(step(bp), mixed):
        assert np.array_equal(got, want)
    # the array form, and instance b takes row b: the rows reversed on the states reversed
    bp.set_physics(PL.plant_rows(phys))
    for got, want in zip(step(bp), mixed):
        assert np.array_equal(got, want)
    # B > n is refused; B <= n steps the first B with their rows
    good = PL.plant_rows(phys)
    assert bp.lib.ffddp_plant_set_instance_params(bp._h, 5, _abi.dptr(good[:5].copy())) == 0
    with pytest.raises(RuntimeError, match="ffddp_plant_step"):
        step(bp)
    assert bp.lib.ffddp_plant_set_instance_params(bp._h, B + 1, _abi.dptr(np.tile(good[0], (B + 1, 1)))) == -1
    assert bp.lib.ffddp_plant_set_instance_params(bp._h, 0, _abi.dptr(good)) == -1
    five = PL.BatchedPlant(5, timestep=0.001, n_substeps=5, physics=phys[:5])
    for got, want in zip(step(five, 5), mixed):
        assert np.array_equal(got, want[:5])
    five.close()
    # back to the handle's struct
    bp.set_physics(None)
    assert bp.physics is None
    for got, want in zip(step(bp), ref):
        assert np.array_equal(got, want)
    bp.close()
    plain.close()


# -- the per-row injector kernels alone ---------------------------------------------------------------
ROW = np.array([0, -1, 1, 2, -1, 3, 4, 5, 6], np.int32)
ROW_DELAYS = ((0, 0), (4, 3), (2, 1), (0, 3), (4, 0), (1, 2), (3, 3))  # 0 and the ring depth (4, 3) on both lines
SENTINEL = 123.0  # in the ring slots above an instance's own delay: never written


def _inject_arrays(B, delay, a, b, sigma, seed=None):
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    d_obs, d_cmd = int(delay[:, 0].max()), int(delay[:, 1].max())
    obs = f64(B, _abi.PLANT_OBS)
    J = dict(row=_dev(ROW[:B]), a=_dev(a), b=_dev(b), obs_ring=f64(d_obs + 1, B, 14), cmd_ring=f64(d_cmd + 1, B, 7),
             tau_hat_filt=f64(B, 7), z_cmd=f64(B, 7), qv_ctrl=f64(B, 14), tau_hat=f64(B, 7), tau_ctrl=f64(B, 7),
             q=obs[:, 0:7], v=obs[:, 7:14], tau_filt=f64(B, 7), tau_cmd=f64(B, 7), tau_app=f64(B, 7), obs=obs,
             d_obs=_dev(delay[:, 0].astype(np.int32)), d_cmd=_dev(delay[:, 1].astype(np.int32)), sigma=_dev(sigma))
    if seed is not None:
        J["seed"] = _dev(np.array(seed, dtype=np.uint64).view(np.int64))
    return J, d_obs, d_cmd


def _fill_unused_slots(J, delay):
    """The sentinel into every ring slot above an instance's own delay; returns the masks (slot, instance)."""
    masks = []
    for ring, d in ((J["obs_ring"], delay[:, 0]), (J["cmd_ring"], delay[:, 1])):
        own = np.full(ROW.shape[0], -1)  # an uninjected instance owns no slot
        own[ROW >= 0] = d[ROW[ROW >= 0]]
        unused = np.arange(ring.shape[0])[:, None] > own[None, :]
        host = ring.cpu().numpy()
        host[unused] = SENTINEL
        ring.copy_(_dev(host))
        masks.append(unused)
    return masks


def test_inject_rows_kernels_equal_mixed_host_class():
    B, ticks, OBS_W = ROW.shape[0], 12, _abi.PLANT_OBS
    on = ROW >= 0
    cfgs = CM.mixed_configs(ROW_DELAYS, seed0=15)
    bat = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs)
    assert np.array_equal(bat.delay, np.array(ROW_DELAYS)) and bat.sig is None
    a, b, z = U.predraw(cfgs, ticks)
    solver = BatchedBoxFDDP(classical_preset(2), max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    zt = _dev(z)
    J, d_obs, d_cmd = _inject_arrays(B, bat.delay, a, b, bat.sigma)
    assert (d_obs, d_cmd) == (4, 3)
    unused = _fill_unused_slots(J, bat.delay)
    inj = solver.fleet_inject(J, d_obs, d_cmd, (9.0, 9.0, 9.0), 0.2, "numpy")  # the scalars are not used: rows given
    rows = solver.fleet_inject_rows(J)
    rng = np.random.default_rng(11)
    for k in range(ticks):
        rec = rng.normal(size=(B, OBS_W))
        tau_cmd, tau_post, tau_filt = rng.normal(size=(B, 7)) * 10, rng.normal(size=(B, 7)), rng.normal(size=(B, 7))
        J["obs"].copy_(_dev(rec))
        J["tau_filt"].copy_(_dev(tau_filt))
        solver.fleet_inject_obs_dev(J, inj, k, z=zt[k], stream=stream, rows=rows)
        J["tau_cmd"].copy_(_dev(tau_cmd))
        J["tau_app"].copy_(_dev(tau_post))  # what post would have written: scale * tau_cmd
        solver.fleet_inject_cmd_dev(J, inj, k, stream=stream, rows=rows)
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
        # no injector: the plant's record, its torque filter, post's actuation, no state touched
        assert np.array_equal(qv[~on], rec[~on, :14]), k
        assert np.array_equal(tau_hat[~on], tau_filt[~on]) and np.array_equal(tau_ctrl[~on], tau_filt[~on]), k
        assert np.array_equal(tau_app[~on], tau_post[~on]), k
        assert np.all(J["tau_hat_filt"].cpu().numpy()[~on] == 0.0) and np.all(J["z_cmd"].cpu().numpy()[~on] == 0.0)
        # the slots above an instance's own delay (all of an uninjected one's) are never written
        for ring, m in zip((J["obs_ring"], J["cmd_ring"]), unused):
            host = ring.cpu().numpy()
            assert np.all(host[m] == SENTINEL) and not np.any(host[~m] == SENTINEL), k
    # a delay beyond the ring is refused before upload
    J2 = dict(J, d_obs=_dev(np.array([0, 5, 0, 0, 0, 0, 0], np.int32)))
    with pytest.raises(ValueError, match="d_obs"):
        solver.fleet_inject_rows(J2)
    with pytest.raises(ValueError, match="d_cmd"):
        solver.fleet_inject_rows(dict(J, d_cmd=_dev(np.array([0, -1, 0, 0, 0, 0, 0], np.int32))))
    solver.close()


def test_inject_rows_null_is_the_old_entry_points():
    """rows = NULL and a struct of three NULL members through the new entry points against the old ones, on
    separate copies of the state; and per-row arrays that repeat the scalars."""
    B, ticks = ROW.shape[0], 6
    cfgs = [U.UncertaintyProfileConfig(seed=s, delta_obs_cycles=10, delta_cmd_s=5.0e-3) for s in range(20, 27)]
    bat = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs)
    assert (bat.obs_delay_steps, bat.cmd_delay_steps) == (2, 1) and bat.sig is not None
    a, b, z = U.predraw(cfgs, ticks)
    solver = BatchedBoxFDDP(classical_preset(2), max_batch=B, device=0)
    lib, h = solver._lib, solver._h
    zt = _dev(z)
    sets = [_inject_arrays(B, bat.delay, a, b, bat.sigma)[0] for _ in range(4)]
    injs = [solver.fleet_inject(J, 2, 1, bat.sig, 0.2, "numpy") for J in sets]
    empty = _abi.FleetInjectRows()
    same = solver.fleet_inject_rows(sets[3])
    p = lambda t: C.c_void_p(int(t.data_ptr()))  # noqa: E731
    rng = np.random.default_rng(12)
    for k in range(ticks):
        rec, tau_cmd, tau_post = rng.normal(size=(B, 69)), rng.normal(size=(B, 7)) * 10, rng.normal(size=(B, 7))
        for J, inj, how in zip(sets, injs, ("old", None, empty, same)):
            J["obs"].copy_(_dev(rec))
            if how == "old":
                solver.fleet_inject_obs_dev(J, inj, k, z=zt[k])
            else:
                r = C.byref(how) if how is not None else None
                assert lib.ffddp_fleet_inject_obs_rows_dev(h, B, C.byref(inj), k, p(zt[k]), p(J["q"]), p(J["v"]), 69, None,
                                                           p(J["qv_ctrl"]), p(J["tau_hat"]), p(J["tau_ctrl"]), r, None) == 0
            J["tau_cmd"].copy_(_dev(tau_cmd))
            J["tau_app"].copy_(_dev(tau_post))
            if how == "old":
                solver.fleet_inject_cmd_dev(J, inj, k)
            else:
                assert lib.ffddp_fleet_inject_cmd_rows_dev(h, B, C.byref(inj), k, p(J["tau_cmd"]), p(J["tau_app"]), r,
                                                           None) == 0
        torch.cuda.synchronize()
        for J in sets[1:]:
            for n in ("qv_ctrl", "tau_hat", "tau_ctrl", "tau_app", "obs_ring", "cmd_ring", "tau_hat_filt", "z_cmd"):
                assert np.array_equal(J[n].cpu().numpy(), sets[0][n].cpu().numpy()), (k, n)
    # error codes as the sibling calls'
    J, inj = sets[3], injs[3]
    r = C.byref(same)
    assert lib.ffddp_fleet_inject_cmd_rows_dev(h, B + 1, C.byref(inj), 0, p(J["tau_cmd"]), p(J["tau_app"]), r, None) == -4
    assert lib.ffddp_fleet_inject_cmd_rows_dev(h, B, C.byref(inj), -1, p(J["tau_cmd"]), p(J["tau_app"]), r, None) == -1
    assert lib.ffddp_fleet_inject_cmd_rows_dev(h, B, C.byref(inj), 0, None, p(J["tau_app"]), r, None) == -1
    assert lib.ffddp_fleet_inject_cmd_rows_dev(h, B, None, 0, p(J["tau_cmd"]), p(J["tau_app"]), r, None) == -1
    assert lib.ffddp_fleet_inject_obs_rows_dev(h, B, C.byref(inj), 0, p(zt[0]), p(J["q"]), p(J["v"]), 6, None,
                                               p(J["qv_ctrl"]), None, None, r, None) == -1
    assert lib.ffddp_fleet_inject_obs_rows_dev(h, B, C.byref(inj), 0, None, p(J["q"]), p(J["v"]), 69, None,
                                               p(J["qv_ctrl"]), None, None, r, None) == -1
    torch.cuda.synchronize()
    solver.close()


def test_inject_rows_philox_through_host_arithmetic():
    """The device Philox source under per-row sigmas and delays: the outputs against uncertainty.philox_normals
    run through the host arithmetic (CM.RowsRestatement).  Bound per output: its sigma times Z_TOL (the normals'
    derived bound, tests/test_gpu_fleet_inject.py) plus the roundings of a sum of three terms of that size;
    the filter is a convex combination of such values and keeps the bound."""
    B, ticks = ROW.shape[0], 8
    on = ROW >= 0
    cfgs = CM.mixed_configs(ROW_DELAYS, seed0=2 ** 32 + 3)
    delay = np.array(ROW_DELAYS)
    sigma = np.array([(c.sigma_q, c.sigma_dq, c.sigma_tau) for c in cfgs])
    a, b, _ = U.draw_gain_bias(cfgs)
    seeds = [c.seed for c in cfgs]
    solver = BatchedBoxFDDP(classical_preset(2), max_batch=B, device=0)
    J, d_obs, d_cmd = _inject_arrays(B, delay, a, b, sigma, seed=seeds)
    inj = solver.fleet_inject(J, d_obs, d_cmd, (9.0, 9.0, 9.0), 0.2, "philox")
    rows = solver.fleet_inject_rows(J)
    host = CM.RowsRestatement(ROW, a, b, delay[:, 0], delay[:, 1], sigma, 0.2)
    rng = np.random.default_rng(13)
    eps = 2.0 ** -52
    sg = sigma[ROW[on]]
    for k in range(ticks):
        rec, tau_cmd = rng.normal(size=(B, 69)), rng.normal(size=(B, 7)) * 10
        J["obs"].copy_(_dev(rec))
        solver.fleet_inject_obs_dev(J, inj, k, rows=rows)
        J["tau_cmd"].copy_(_dev(tau_cmd))
        solver.fleet_inject_cmd_dev(J, inj, k, rows=rows)
        torch.cuda.synchronize()
        zk = U.philox_normals(seeds, k)
        qv, th, thf = host.obs(k, zk, rec[:, 0:7], rec[:, 7:14])
        app = host.cmd(k, tau_cmd, np.zeros((B, 7)))
        dq = np.abs(J["qv_ctrl"].cpu().numpy() - qv)[on]
        scale = 4.0 * eps * max(np.max(np.abs(qv)), np.max(np.abs(th)), np.max(np.abs(app)), 1.0)
        assert np.all(dq[:, :7] <= sg[:, 0:1] * Z_TOL + scale) and np.all(dq[:, 7:] <= sg[:, 1:2] * Z_TOL + scale), k
        for dev, want in ((J["tau_hat"], th), (J["tau_ctrl"], thf), (J["tau_app"], app)):
            assert np.all(np.abs(dev.cpu().numpy() - want)[on] <= sg[:, 2:3] * Z_TOL + scale), k
    solver.close()


# -- the loop ---------------------------------------------------------------------------------------
LB, HORIZON, TICKS, T0, K_SAVE = 6, 8, 40, 0.7, 17
LOOP_DELAYS = ((0, 0), (2, 1), (0, 3), (4, 0))
INJECTED = (0, 2, 3, 5)


def _loop_setup(variant):
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (LB, 7))
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    traj, meta = benchmark_traj(obs_n.ee_pos)
    cal = FL.site_calibration(obs_n)
    dt = nominal.dt
    nominal.close()
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    cfg = make(dt, meta["z_contact"], horizon=HORIZON)
    tilt = np.array([0.0, 5.0, 10.0, -5.0, 0.0, 5.0])
    scale = np.array([1.0, 0.9, 1.1, 0.95, 1.05, 1.0])[:, None] * np.linspace(0.95, 1.05, 7)
    mixed = CM.mixed_configs(LOOP_DELAYS, seed0=100)
    ucfgs = [None] * LB
    for b, c in zip(INJECTED, mixed):
        ucfgs[b] = c
    phys = [PL.PlantPhysics(armature=0.05 + 0.03 * b, damping=np.linspace(0.5, 1.5, 7) * (1.0 + 0.1 * b),
                            r_tool=0.03 + 0.0002 * b, margin=0.001 + 0.0001 * b, solref=(0.01 + 0.004 * b, 0.8 + 0.08 * b),
                            solimp=(0.85 + 0.01 * b, 0.95, 0.001 * (1 + b), 0.4 + 0.04 * b, float(1 + b % 3)))
            for b in range(LB)]
    make_loop = lambda: DeviceFleetLoop(variant, LB, traj, cfg, q0, tilt_deg=tilt, torque_scale=scale, steps=TICKS,  # noqa: E731
                                        calibration=cal, t0=T0, uncertainty=ucfgs, noise="numpy", plant_physics=phys)
    return make_loop, ucfgs, scale, phys


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_device_loop_mixed_profiles_and_plant_rows(variant):
    make_loop, ucfgs, scale, phys = _loop_setup(variant)
    loop = make_loop()
    idx, rest = list(INJECTED), [b for b in range(LB) if b not in INJECTED]
    assert loop.dt == DT and (loop.inject.d_obs, loop.inject.d_cmd) == (4, 3) and loop.inject_rows is not None
    assert tuple(loop.J["obs_ring"].shape) == (5, LB, 14) and tuple(loop.J["cmd_ring"].shape) == (4, LB, 7)
    host = U.BatchedUncertaintyInjector(dt=loop.dt, nu=7, configs=[ucfgs[b] for b in idx])
    # a second plant with the same rows, stepped with the torques the loop applied
    twin = PL.BatchedPlant(LB, timestep=0.001, n_substeps=5, physics=phys)
    twin.q, twin.v = loop.P["q"].cpu().numpy(), loop.P["v"].cpu().numpy()
    twin.plane = loop.P["plane"].cpu().numpy()
    assert np.array_equal(twin.step(np.zeros((LB, 7)), integrate=False), loop.P["obs"].cpu().numpy())  # the start
    assert not loop.hints[0] and loop.hints[TICKS - 1]  # the run crosses the references' contact switch
    saved = None
    for k in range(TICKS):
        if k == K_SAVE:
            saved = loop.state()
        tau_filt0 = loop.P["tau_filt"].cpu().numpy()
        loop.tick()
        obs = loop.P["obs"].cpu().numpy()  # what tick k saw: the plant steps at the start of tick k + 1
        if k > 0:
            assert np.array_equal(obs, twin.obs), (variant, k)
        x0, tau_cmd, tau_app = (loop.T[n].cpu().numpy() for n in ("x0", "tau_cmd", "tau_app"))
        qh, vh = host.observation_for_controller(obs[idx, 0:7], obs[idx, 7:14])
        assert np.array_equal(x0[idx, 0:7], qh) and np.array_equal(x0[idx, 7:14], vh), (variant, k)
        if variant == "ff":
            assert np.array_equal(x0[idx, 14:21], host.tau_hat_filt), (variant, k)
            assert np.array_equal(x0[rest, 14:21], tau_filt0[rest]), (variant, k)
        assert np.array_equal(tau_app[idx], host.command_for_plant(tau_cmd[idx])), (variant, k)
        assert np.array_equal(x0[rest, :14], obs[rest, :14]), (variant, k)
        assert np.array_equal(tau_app[rest], tau_cmd[rest] * scale[rest]), (variant, k)
        assert np.all(np.isfinite(tau_cmd))
        twin.step(tau_app)
    r = loop.results()
    assert np.array_equal(r["obs"][TICKS], twin.obs[:, [28, 29, 30, 46, 47]])
    assert np.array_equal(r["inject_a"][idx], host.a) and np.array_equal(r["inject_b"][idx], host.b)
    assert np.array_equal(r["inject_delay"][idx], np.array(LOOP_DELAYS)) and np.all(r["inject_delay"][rest] == -1)
    assert np.array_equal(r["inject_sigma"][idx], host.sigma) and np.all(np.isnan(r["inject_sigma"][rest]))
    assert np.array_equal(r["plant_rows"], PL.plant_rows(phys)) and not np.any(r["plant_fail"])
    r["x0"], r["tau_app"] = loop.T["x0"].cpu().numpy(), loop.T["tau_app"].cpu().numpy()
    loop.close()
    twin.close()
    # tick() equals run(); and a loop continued from the state saved at tick K_SAVE equals the uninterrupted one
    other = make_loop()
    other.run(TICKS)
    for lo in (0, K_SAVE):
        if lo:
            assert saved["obs_ring"].shape == (5, LB, 14) and saved["cmd_ring"].shape == (4, LB, 7)
            other.load_state(saved)
            other.log_info[lo:].fill_(float("nan"))
            other.log_obs[lo:].fill_(float("nan"))
            other.run(TICKS - lo)
        o = other.results()
        assert np.array_equal(o["info"], r["info"], equal_nan=True) and np.array_equal(o["obs"], r["obs"]), (variant, lo)
        assert np.array_equal(other.T["x0"].cpu().numpy(), r["x0"]), (variant, lo)
        assert np.array_equal(other.T["tau_app"].cpu().numpy(), r["tau_app"]), (variant, lo)
    other.close()


# -- the sweep ----------------------------------------------------------------------------------------
def test_sweep_with_plant_and_uncertainty_spread():
    """Against the host path at the bounds of the existing sweep tests (tests/test_gpu_fleet_inject.py,
    tests/test_gpu_fleet_loop_sweep.py): the same keys and counts, the statistics over the contact phase (which
    0.2 s does not reach) NaN and the others finite, a second run the same bits, and the tracking error within
    rtol 1e-3 of the host loop's."""
    kw = dict(scenarios=("flat", "actuation_uncertainty"), seeds=3, total_time=0.2, verbose=False,
              plant_spread=(0.5, 0.5), uncertainty_spread=(0.5, 3))
    host = FL.run_sweep(**kw)
    a = FL.run_sweep(device_loop=True, device_noise="numpy", **kw)
    b = FL.run_sweep(device_loop=True, device_noise="numpy", **kw)
    assert set(a["per_instance"]) == set(host["per_instance"]) == set(FL.SUMMARY_KEYS)
    assert a["ticks"] == host["ticks"] == 40 and a["instances"] == a["n_all"] == host["n_all"] == 6
    assert list(a["names"]) == list(host["names"]) == ["flat"] * 3 + ["actuation_uncertainty"] * 3
    assert not np.any(a["plant_fail"])
    undefined = {"rms_tangential_error_contact_phase", "contact_loss_contact_phase_pct", "fn_mean_contact_phase"}
    for k in FL.SUMMARY_KEYS:
        va, vh = a["per_instance"][k], host["per_instance"][k]
        assert va.shape == vh.shape == (6,), k
        if k in undefined:
            assert np.all(np.isnan(va)) and np.all(np.isnan(vh)), (k, va)
        else:
            assert np.all(np.isfinite(va)) and np.all(np.isfinite(vh)), (k, va, vh)
        assert np.array_equal(va, b["per_instance"][k], equal_nan=True), k
    print("rms_3d_error device", a["per_instance"]["rms_3d_error"], "host", host["per_instance"]["rms_3d_error"])
    assert np.allclose(a["per_instance"]["rms_3d_error"], host["per_instance"]["rms_3d_error"], rtol=1e-3)
    # the reported rows and profiles are the draws, restated
    rows, delay, sigma = np.zeros((6, 23)), np.full((6, 2), -1), np.full((6, 3), np.nan)
    for i, s in enumerate(a["seed"]):
        u = np.random.default_rng([int(s), 2]).uniform(-1.0, 1.0, 2)
        rows[i] = PL.PlantPhysics(damping=1.0 * (1.0 + 0.5 * u[1]), solref=(0.02 * (1.0 + 0.5 * u[0]), 1.0)).row()
        if i >= 3:
            g = np.random.default_rng([int(s), 3])
            f = 1.0 + 0.5 * g.uniform(-1.0, 1.0)
            delay[i] = g.integers(0, 4, 2)
            sigma[i] = (5.0e-4 * f, 2.0e-3 * f, 5.0e-2 * f)
    assert len({tuple(d) for d in delay[3:]}) > 1 or np.any(delay[3:] > 0)  # the spread does delay someone
    for res in (a, host):
        assert np.array_equal(res["plant_rows"], rows)
        assert np.array_equal(res["inject_delay"], delay) and np.array_equal(res["inject_sigma"], sigma, equal_nan=True)
    inj = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=[
        FL.sweep_uncertainty_config("actuation_uncertainty", int(s), DT, (0.5, 3)) for s in a["seed"][3:]])
    assert np.array_equal(a["inject_a"][3:], inj.a) and np.array_equal(a["inject_b"][3:], inj.b)
    assert np.array_equal(inj.delay, delay[3:]) and np.array_equal(inj.sigma, sigma[3:])
    assert FL.gather_summaries(a, a["n_all"]).shape == (6, len(FL.SUMMARY_KEYS))
