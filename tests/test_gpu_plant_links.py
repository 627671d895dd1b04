"""GPU: per-instance link inertial parameters in the plant stand-in
(ffddp_plant_set_instance_links).  The plant kernel with one link-model row
per instance -- alone and together with per-instance physics rows -- against
oracle/plant.py under oracle.panda's inertial arrays monkeypatched per
instance; bit identity with own-model handles, with no rows, and under NaN
padding; the handle's plumbing and refusals; the gravity torque a row gives
against the host model code and the solve's reading of the same row;
DeviceFleetLoop(plant_link_models=...) against the plain loop and a loop
stepped by hand; run_sweep(plant_payload_spread=..., payload_known=...)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_fleet_mismatch_cpu as CM  # noqa: E402
import test_gpu_fleet_mismatch as FM  # noqa: E402  (_plant_inputs, the loop's shapes)
import test_gpu_force_ref as FR  # noqa: E402  (_same_results)
import test_gpu_link_model as LM  # noqa: E402  (the six models, oracle.panda under a model)
from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp.config import classical_preset, link_model_rows  # noqa: E402
from ffddp.fleet_loop import LPF_ALPHA, DeviceFleetLoop  # noqa: E402
from ffddp.trajectory import benchmark_traj  # noqa: E402
from oracle import plant as OP  # noqa: E402

PLANT_B = FM.PLANT_B  # 70: two 64-thread blocks, the second with a tail
PADDING = np.array([16 * j + k for j in range(7) for k in (13, 14, 15)] + list(range(112, 128)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _instance_models(B):
    """Instance b carries model b % 6 of test_gpu_link_model._models."""
    six = LM._models()
    return [six[b % 6] for b in range(B)]


# -- the kernel against the oracle ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(integrate: bool, with_phys: bool):
    """test_gpu_fleet_mismatch._plant_inputs(3) and the oracle's step of every instance under its own link model
    (oracle.panda's LINK_MASS / LINK_COM / LINK_INERTIA replaced for the call) and, with_phys, its own physics
    row; computed once.  Branch counts as test_gpu_fleet_mismatch._plant_case's."""
    q, v, tau, tilt, phys = FM._plant_inputs(3)
    models = _instance_models(PLANT_B)
    ref, branches, fmax, finite = [], [0, 0, 0, 0], 0.0, True
    for b in range(PLANT_B):
        p = phys[b] if with_phys else PL.PlantPhysics()
        prm = OP.default_params(0.001, 5)
        if with_phys:
            prm.update(armature=np.asarray(p.armature, float), damping=np.asarray(p.damping, float), r_tool=p.r_tool,
                       margin=p.margin, solref=p.solref, solimp=p.solimp)
        n, p0 = PL.table_plane(tilt[b])
        with LM._patched(models[b]):
            qo, vo, o = OP.step(prm, q[b], v[b], tau[b], n, p0, integrate=integrate)
        ref.append((qo, vo, o))
        finite = finite and all(np.all(np.isfinite(np.asarray(x, float))) for x in (qo, vo, *o.values()))
        if o["ncon"]:
            fmax = max(fmax, float(o["fn"]))
            d0, dmax, width, mid, pw = p.solimp
            x = abs(float(n @ (o["ee_pos"] - p0)) - p.r_tool - p.margin) / width
            branches[3 if x >= 1.0 else 0 if pw == 1.0 else 1 if x <= mid else 2] += 1
    return dict(q=q, v=v, tau=tau, tilt=tilt, phys=phys, models=models, ref=ref, ncon=sum(branches),
                branches=tuple(branches), fmax=fmax, finite=finite)


@pytest.mark.parametrize("with_phys", [False, True])
@pytest.mark.parametrize("integrate", [False, True])
def test_plant_link_rows_kernel_matches_oracle(integrate, with_phys):
    """Tolerances: tests/test_gpu_plant.py::test_plant_kernel_matches_oracle's.  For default_rng(3) and model
    b % 6 the oracle alone gives: link rows alone, 35 instances in contact forward only and integrated (the
    scene's solimp: all saturated but one), forces up to 662 N and 463 N; with the physics rows 35 (forward only,
    the geometry of the existing test) and 34 (integrated) in contact, branch counts (power 1, x <= mid, x > mid,
    saturated) (3, 6, 4, 22) and (2, 6, 2, 24), forces up to 1052 N and 532 N; everything finite."""
    case = _oracle_case(integrate, with_phys)
    print(f"integrate={integrate} physics={with_phys}: in contact {case['ncon']}, branches {case['branches']}, "
          f"max force {case['fmax']:.1f} N")
    assert case["finite"] and case["ncon"] >= 8, case["ncon"]
    if with_phys:
        assert min(case["branches"]) >= 2, case["branches"]
    bp = PL.BatchedPlant(PLANT_B, timestep=0.001, n_substeps=5, physics=case["phys"] if with_phys else None,
                         link_models=case["models"])
    assert bp.link_rows.shape == (PLANT_B, _abi.LINK_W) and (bp.physics is not None) == with_phys
    bp.q, bp.v = case["q"].copy(), case["v"].copy()
    bp.set_tilt(case["tilt"])
    obs = bp.step(case["tau"], integrate=integrate).copy()
    for b in range(PLANT_B):
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


# -- bit identity ----------------------------------------------------------------------------------
IB = 12


def _host_step(bp, q, v, tau, tilt, integrate=True):
    n = q.shape[0]
    bp.q, bp.v = q.copy(), v.copy()
    bp.set_tilt(tilt[:n])
    obs = bp.step(tau, integrate=integrate).copy()
    return obs, bp.q.copy(), bp.v.copy()


def _dev_step(bp, q, v, tau, tilt, integrate=True):
    """The same through ffddp_plant_step_dev on device tensors; also the failure flags."""
    qd, vd, td = _dev(q), _dev(v), _dev(tau)
    plane = _dev(np.stack([np.concatenate(PL.table_plane(t)) for t in tilt]))
    obs = torch.full((q.shape[0], _abi.PLANT_OBS), 123.0, dtype=torch.float64, device="cuda")
    fail = torch.full((q.shape[0],), 7, dtype=torch.int32, device="cuda")
    bp.step_dev(qd, vd, td, plane, obs, fail=fail, integrate=integrate)
    torch.cuda.synchronize()
    assert not fail.cpu().numpy().any()
    return obs.cpu().numpy(), qd.cpu().numpy(), vd.cpu().numpy()


def _same(got, want, tag):
    for g, w, name in zip(got, want, ("obs", "q", "v")):
        assert np.array_equal(g, w), (tag, name)


@pytest.mark.parametrize("with_phys", [False, True])
def test_rows_give_the_bits_of_own_model_handles(with_phys):
    """Each instance's q, v and whole record under row b against a handle created with that model
    (BatchedPlant(1, robot=model)) stepping the instance alone, through ffddp_plant_step and ffddp_plant_step_dev;
    with_phys: both sides under the instance's physics row as well."""
    q, v, tau, tilt, phys = FM._plant_inputs(5, IB)
    models = _instance_models(IB)
    bp = PL.BatchedPlant(IB, timestep=0.001, n_substeps=5, link_models=models, physics=phys if with_phys else None)
    for integrate in (True, False):
        host = _host_step(bp, q, v, tau, tilt, integrate)
        dev = _dev_step(bp, q, v, tau, tilt, integrate)
        _same(dev, host, ("dev == host", integrate))
        assert np.any(host[0][:, 47] == 1.0) and np.any(host[0][:, 47] == 0.0)  # both contact branches
        for b in range(IB):
            own = PL.BatchedPlant(1, timestep=0.001, n_substeps=5, robot=models[b],
                                  physics=[phys[b]] if with_phys else None)
            assert own.link_rows is None
            s = slice(b, b + 1)
            want = _host_step(own, q[s], v[s], tau[s], tilt[s], integrate)
            _same([a[s] for a in host], want, ("host", b, integrate))
            _same(_dev_step(own, q[s], v[s], tau[s], tilt[s], integrate), want, ("dev", b, integrate))
            own.close()
    # the models matter: instances b and b + 6 aside, the plain handle gives other bits where the model is not nominal
    plain = PL.BatchedPlant(IB, timestep=0.001, n_substeps=5, physics=phys if with_phys else None)
    ref = _host_step(plain, q, v, tau, tilt)
    host = _host_step(bp, q, v, tau, tilt)
    for b in range(IB):
        assert np.array_equal(host[0][b], ref[0][b]) == (b % 6 == 0), b
    plain.close()
    bp.close()


@pytest.mark.parametrize("with_phys", [False, True])
def test_nominal_rows_none_and_nan_padding(with_phys):
    q, v, tau, tilt, phys = FM._plant_inputs(5, IB)
    kw = dict(timestep=0.001, n_substeps=5, physics=phys if with_phys else None)
    plain = PL.BatchedPlant(IB, **kw)
    ref = {i: (_host_step(plain, q, v, tau, tilt, i), _dev_step(plain, q, v, tau, tilt, i)) for i in (True, False)}
    assert plain.link_rows is None

    def check(bp, want, tag):
        for i in (True, False):
            _same(_host_step(bp, q, v, tau, tilt, i), want[i][0], (tag, "host", i))
            _same(_dev_step(bp, q, v, tau, tilt, i), want[i][1], (tag, "dev", i))

    # nominal rows (as models, as None entries, as an array): the bits of no rows
    bp = PL.BatchedPlant(IB, link_models=[R.LinkModel()] * IB, **kw)
    check(bp, ref, "nominal models")
    bp.set_link_models([None] * IB)
    check(bp, ref, "None entries")
    bp.set_link_models(link_model_rows([None] * IB))
    check(bp, ref, "array")
    # distinct rows, clean and with NaN in every padding entry: the same bits; then back to no rows
    rows = link_model_rows(_instance_models(IB))
    bp.set_link_models(rows)
    assert np.array_equal(bp.link_rows, rows)
    mixed = {i: (_host_step(bp, q, v, tau, tilt, i), _dev_step(bp, q, v, tau, tilt, i)) for i in (True, False)}
    assert not np.array_equal(mixed[True][0][0], ref[True][0][0])
    dirty = rows.copy()
    dirty[:, PADDING] = np.nan
    bp.set_link_models(dirty)
    check(bp, mixed, "NaN padding")
    assert bp.lib.ffddp_plant_set_instance_links(bp._h, IB, _abi.dptr(dirty)) == 0  # the raw call takes them too
    check(bp, mixed, "NaN padding, raw")
    bp.set_link_models(None)
    assert bp.link_rows is None
    check(bp, ref, "back to none")
    bp.close()
    plain.close()


# -- plumbing ------------------------------------------------------------------------------------------
def test_plant_link_rows_plumbing():
    B = IB
    q, v, tau, tilt, phys = FM._plant_inputs(5, B)
    models = _instance_models(B)
    rows = link_model_rows(models)
    step = lambda bp, n=B: _host_step(bp, q[:n], v[:n], tau[:n], tilt[:n])  # noqa: E731
    plain = PL.BatchedPlant(B, timestep=0.001, n_substeps=5)
    ref = step(plain)
    bp = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, link_models=models)
    links = step(bp)
    assert not np.array_equal(links[0], ref[0])
    fn = bp.lib.ffddp_plant_set_instance_links
    # an invalid row is refused through Python and through the raw call, and the previous rows stay in force
    for e, bad in ((16 * 3, 0.0), (16 * 3, -2.0), (16 * 3, np.nan), (16 * 6, np.inf), (16 * 2 + 2, np.nan),
                   (16 * 5 + 4 + 8, -np.inf)):
        wrong = rows.copy()
        wrong[7, e] = bad
        with pytest.raises(ValueError, match="finite"):
            bp.set_link_models(wrong)
        assert fn(bp._h, B, _abi.dptr(wrong)) == -1, (e, bad)
    mass = R.MASS.copy()
    mass[1] = -1.0
    with pytest.raises(ValueError, match="finite"):
        bp.set_link_models(models[:-1] + [R.LinkModel(mass=mass)])
    with pytest.raises(ValueError, match="rows for"):
        bp.set_link_models(models[:5])
    assert np.array_equal(bp.link_rows, rows)
    _same(step(bp), links, "after refusals")
    # n < 1, n > max_batch, a null handle
    assert fn(bp._h, 0, _abi.dptr(rows)) == -1 and fn(bp._h, -3, _abi.dptr(rows)) == -1
    assert fn(bp._h, B + 1, _abi.dptr(np.tile(rows[0], (B + 1, 1)))) == -1
    assert fn(None, B, _abi.dptr(rows)) == -1
    _same(step(bp), links, "after refused counts")
    # n rows with B > n fails the step (host and device entry point); B <= n steps the first B with their rows
    assert fn(bp._h, 5, _abi.dptr(rows[:5].copy())) == 0
    with pytest.raises(RuntimeError, match="ffddp_plant_step"):
        step(bp)
    with pytest.raises(RuntimeError, match="ffddp_plant_step_dev"):
        _dev_step(bp, q, v, tau, tilt)
    five = PL.BatchedPlant(5, timestep=0.001, n_substeps=5, link_models=models[:5])
    _same(step(five, 5), [a[:5] for a in links], "five")
    five.close()
    # physics rows and link rows are set and cleared independently of each other
    both_ref = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, physics=phys, link_models=models)
    both = step(both_ref)
    both_ref.close()
    phys_ref = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, physics=phys)
    only_phys = step(phys_ref)
    phys_ref.close()
    assert not np.array_equal(both[0], only_phys[0]) and not np.array_equal(both[0], links[0])
    bp.set_link_models(models)
    bp.set_physics(phys)
    _same(step(bp), both, "both")
    bp.set_link_models(None)
    assert bp.link_rows is None and bp.physics is not None
    _same(step(bp), only_phys, "links cleared, physics kept")
    bp.set_link_models(rows)
    bp.set_physics(None)
    assert bp.physics is None and np.array_equal(bp.link_rows, rows)
    _same(step(bp), links, "physics cleared, links kept")
    # either set alone bounds B: physics rows for 5 under link rows for all
    assert bp.lib.ffddp_plant_set_instance_params(bp._h, 5, _abi.dptr(PL.plant_rows(phys[:5]))) == 0
    with pytest.raises(RuntimeError, match="ffddp_plant_step"):
        step(bp)
    bp.set_physics(None)
    bp.set_link_models(None)
    _same(step(bp), ref, "back to the handle")
    bp.close()
    plain.close()


# -- the same row, read the same way by the plant, the host model code and the solve ----------------------
def test_bias_at_rest_is_the_gravity_torque_of_the_row():
    """v = 0, out of contact, forward only: qfrc_bias (obs[:, 14:21]) under row m against the host
    ffddp_gravity_torque of make_robot(m) and against the device solve's gravity torque under the same rows, within
    the 1e-10 the plant test uses for the bias."""
    models = LM._models()
    B = len(models)
    q = LM._postures(B)
    rows = link_model_rows(models)
    bp = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, link_models=rows)
    bp.q, bp.v = q.copy(), np.zeros((B, 7))
    obs = bp.step(np.zeros((B, 7)), integrate=False).copy()
    assert not obs[:, 47].any()  # out of contact
    bias = obs[:, 14:21]
    host = np.stack([_abi.gravity_torque(q[i], _abi.make_robot(m))[0] for i, m in enumerate(models)])
    np.testing.assert_allclose(bias, host, rtol=1e-10, atol=1e-10)
    solver = BatchedBoxFDDP(classical_preset(4), max_batch=B)
    tau = torch.full((B, 7), 123.0, dtype=torch.float64, device="cuda")
    solver.gravity_torque_dev(_dev(q), tau, link_model=_dev(rows))
    torch.cuda.synchronize()
    np.testing.assert_allclose(bias, tau.cpu().numpy(), rtol=1e-10, atol=1e-10)
    solver.close()
    # the rows carry the load: every model but the nominal one moves the bias
    nominal = _abi.gravity_torque(q)
    assert np.max(np.abs(bias[0] - nominal[0])) < 1e-10
    assert np.all(np.max(np.abs(bias[1:] - nominal[1:]), 1) > 0.05)
    bp.close()


# -- the device loop -----------------------------------------------------------------------------------
LB, TICKS, T0 = FM.LB, FM.TICKS, FM.T0


def _loop(variant, **kw):
    """test_gpu_fleet_mismatch._loop_setup's loop (six instances, mixed injector profiles, mixed physics rows, a
    tilt and a command scale per instance, a run across the contact switch), with the device metrics on."""
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (LB, 7))
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    traj, meta = benchmark_traj(obs_n.ee_pos)
    cal = FL.site_calibration(obs_n)
    dt = nominal.dt
    nominal.close()
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    cfg = make(dt, meta["z_contact"], horizon=FM.HORIZON)
    tilt = np.array([0.0, 5.0, 10.0, -5.0, 0.0, 5.0])
    scale = np.array([1.0, 0.9, 1.1, 0.95, 1.05, 1.0])[:, None] * np.linspace(0.95, 1.05, 7)
    mixed = CM.mixed_configs(FM.LOOP_DELAYS, seed0=100)
    ucfgs = [None] * LB
    for b, c in zip(FM.INJECTED, mixed):
        ucfgs[b] = c
    phys = [PL.PlantPhysics(armature=0.05 + 0.03 * b, damping=np.linspace(0.5, 1.5, 7) * (1.0 + 0.1 * b),
                            r_tool=0.03 + 0.0002 * b, margin=0.001 + 0.0001 * b, solref=(0.01 + 0.004 * b, 0.8 + 0.08 * b),
                            solimp=(0.85 + 0.01 * b, 0.95, 0.001 * (1 + b), 0.4 + 0.04 * b, float(1 + b % 3)))
            for b in range(LB)]
    loop = DeviceFleetLoop(variant, LB, traj, cfg, q0, tilt_deg=tilt, torque_scale=scale, steps=TICKS, calibration=cal,
                           t0=T0, uncertainty=ucfgs, noise="numpy", plant_physics=phys, metrics=True,
                           t_contact_phase=meta["t_contact_phase"], **kw)
    return loop, tilt, phys


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_nominal_plant_models_equal_the_plain_loop(variant):
    plain, _, _ = _loop(variant)
    nom, _, _ = _loop(variant, plant_link_models=[R.LinkModel()] * LB)
    non, _, _ = _loop(variant, plant_link_models=[None] * LB)
    assert plain.plant.link_rows is None and np.array_equal(nom.plant.link_rows, non.plant.link_rows)
    assert nom.md is None and nom.link_rows is None  # the controllers' rows are another argument
    for loop in (plain, nom, non):
        loop.run(TICKS)
    rp, ra, rl = plain.results(), nom.results(), non.results()
    assert (rp["surface"] != 0).any() and not (rp["surface"] != 0).all()  # the run crosses the contact switch
    FR._same_results(ra, rp, (variant, "models"))
    FR._same_results(rl, rp, (variant, "none"))
    assert np.array_equal(ra["metrics"], rp["metrics"], equal_nan=True)
    assert np.array_equal(rl["metrics"], rp["metrics"], equal_nan=True)
    assert set(nom.state()) == set(plain.state())  # nothing new in the saved state
    for loop in (plain, nom, non):
        loop.close()


def _hand_run(loop, bp, tilt, ticks):
    """DeviceFleetLoop's start sequence and ticks through the entry points themselves, the plant steps through
    `bp` (a BatchedPlant carrying the rows) in place of the loop's own plant."""
    P, T, J, s = loop.P, loop.T, loop.J, loop.solver
    plane = lambda t: _dev(np.stack([np.concatenate(PL.table_plane(x)) for x in t]))  # noqa: E731

    def plant_step(integrate, fail):
        bp.step_dev(P["q"], P["v"], P["tau_app"], P["plane"], P["obs"], fail=fail, integrate=integrate,
                    stream=loop._stream)

    # the start: the bias torque on a level table is the classical controllers' first command
    P["plane"].copy_(plane(np.zeros(LB)))
    plant_step(False, loop.log_fail[0])
    if loop.variant == "classical":
        loop.S["tau_prev"].copy_(P["obs"][:, 14:21])
    P["plane"].copy_(plane(tilt))
    plant_step(False, loop.log_fail[0])
    for k in range(ticks):
        if k > 0:
            plant_step(True, loop.log_fail[k])
            j = k - 1  # the metrics fold of the record after tick j's command
            s.fleet_metrics_dev(loop.acc, P["obs"], loop.t_phase, float(loop.cfg.fn_des), info=loop.log_info[j],
                                need=None, plant_fail=loop.log_fail[k], stream=loop._stream, p_ref=loop.p_tab[j],
                                ts=float(loop.times[j]) + loop.dt)
        T["info"], T["log_obs"] = loop.log_info[k], loop.log_obs[k]
        T["node_ref1"] = loop.ref_table[k]
        s.fleet_inject_obs_dev(J, loop.inject, k, z=loop.z_table[k], stream=loop._stream, rows=loop.inject_rows)
        s.fleet_pre_dev(T, loop.params, bool(loop.hints[k]), stream=loop._stream, tasks=None)
        s.solve_dev(T, maxiter=int(loop.cfg.max_iters), is_feasible=False, stream=loop._stream)
        s.fleet_post_dev(T, loop.params, lpf=LPF_ALPHA, stream=loop._stream)
        s.fleet_inject_cmd_dev(J, loop.inject, k, stream=loop._stream, rows=loop.inject_rows)
    # results() takes the closing step and its fold: leave them to it, through the hand's plant
    loop.plant.close()
    loop.plant = bp
    loop.k, loop.m_k, loop._stepped = ticks, ticks - 1, False


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_distinct_plant_models_equal_the_hand_stepped_loop(variant):
    models = LM._models()
    assert len(models) == LB
    a, tilt, phys = _loop(variant, plant_link_models=models)
    assert np.array_equal(a.plant.link_rows, link_model_rows(models))
    assert np.array_equal(a.plant.physics, PL.plant_rows(phys)) and a.md is None
    a.run(TICKS)
    ra = a.results()
    o, _, _ = _loop(variant)
    bp = PL.BatchedPlant(LB, timestep=0.001, n_substeps=5, physics=phys, link_models=link_model_rows(models))
    _hand_run(o, bp, tilt, TICKS)
    ro = o.results()
    FR._same_results(ra, ro, variant)
    assert np.array_equal(ra["metrics"], ro["metrics"], equal_nan=True)
    # after the run: no plant step failed, every summary is finite, and the arms' payloads show
    assert not np.any(ra["plant_fail"])
    for k, val in ra["summary"].items():
        assert np.all(np.isfinite(np.asarray(val, float))), (k, val)
    plain, _, _ = _loop(variant)
    plain.run(TICKS)
    rp = plain.results()
    assert not np.array_equal(rp["info"], ra["info"], equal_nan=True) and not np.array_equal(rp["obs"], ra["obs"])
    assert np.array_equal(rp["obs"][:, 0], ra["obs"][:, 0])  # instance 0 carries the nominal model
    for b in range(1, LB):
        assert not np.array_equal(rp["obs"][:, b], ra["obs"][:, b]), b
    for loop in (a, o, plain):
        loop.close()


def test_loop_plant_models_combine_with_controller_models():
    """plant_link_models beside link_models (and the physics rows, the injectors): each goes where it belongs."""
    models = LM._models()
    loop, _, _ = _loop("classical", plant_link_models=models, link_models=models[::-1])
    assert np.array_equal(loop.plant.link_rows, link_model_rows(models))
    assert np.array_equal(loop.link_rows, link_model_rows(models[::-1]))
    loop.run(8)
    r = loop.results()
    assert not np.any(r["plant_fail"]) and np.all(np.isfinite(r["obs"]))
    assert np.all(np.isfinite(r["cost"])) and np.all(np.isfinite(r["tau_cmd_inf"]))
    # against the loop whose controllers plan with the nominal model: the same plants, other plans
    other, _, _ = _loop("classical", plant_link_models=models)
    other.run(8)
    assert not np.array_equal(other.results()["cost"], r["cost"])
    other.close()
    loop.close()


# -- the sweep ------------------------------------------------------------------------------------------
WHOLE_RUN = ("rms_tangential_error", "rms_3d_error", "avg_abs_force_err", "max_fn", "unstable_ticks",
             "neg_accepted_ticks", "solve_not_ok_ticks")  # 0.1 s has no contact phase: the other keys are NaN


def test_sweep_with_a_plant_payload_spread():
    kw = dict(scenarios=("flat", "tilted_10"), seeds=2, total_time=0.1, verbose=False)
    plain = FL.run_sweep(device_loop=True, **kw)
    unknown = FL.run_sweep(device_loop=True, plant_payload_spread=(0.5, 3.0), **kw)
    known = FL.run_sweep(device_loop=True, plant_payload_spread=(0.5, 3.0), payload_known=True, **kw)
    dev = FL.run_sweep(device_loop=True, plant_payload_spread=(0.5, 3.0), device_summary=True, **kw)
    host = FL.run_sweep(plant_payload_spread=(0.5, 3.0), **kw)
    assert "plant_payload_mass" not in plain and unknown["instances"] == 4 and unknown["ticks"] == 20
    want = FL.sweep_plant_payload_masses(unknown["seed"], (0.5, 3.0))
    assert np.all((want >= 0.5) & (want <= 3.0))
    for res in (unknown, known, dev, host):
        assert np.array_equal(res["plant_payload_mass"], want)
        assert "payload_mass" not in res  # the controller-side sweep's key stays its own
        for k in WHOLE_RUN:
            assert np.all(np.isfinite(res["per_instance"][k])), k
    assert known["payload_known"] is True and unknown["payload_known"] is False and host["payload_known"] is False
    assert not np.any(unknown["plant_fail"]) and not np.any(known["plant_fail"])
    e = "rms_3d_error"
    assert np.all(unknown["per_instance"][e] != plain["per_instance"][e])
    assert np.all(known["per_instance"][e] != plain["per_instance"][e])
    assert np.all(known["per_instance"][e] != unknown["per_instance"][e])
    assert np.all(host["per_instance"][e] != FL.run_sweep(**kw)["per_instance"][e])
    print("rms_3d_error plain", plain["per_instance"][e], "unknown", unknown["per_instance"][e], "known",
          known["per_instance"][e], "host", host["per_instance"][e])
