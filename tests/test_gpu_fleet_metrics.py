"""GPU: the sweep's task metrics accumulated on the device.

1. ffddp_fleet_metrics_dev alone against runlog.accumulate_metrics, fed the
   reference positions the standalone device sampler returns at the same
   times: every field array_equal (the per-tick terms are IEEE add, multiply
   and square root in one order and both sides add in call order).
2. DeviceFleetLoop(metrics=True) against the numpy summary of
   fleet._run_sweep_device built from the same run's logs: counters, maxima
   and percentages exact; a sum S of n non-negative terms within
   (2 n + 8) 2^-53 S + c (sequential against pairwise summation; c covers the
   device sincos against numpy's in circle-phase references, TOL_REF per
   coordinate: n_circle (2 e_max sqrt(3) eps + 3 eps^2) for the squared sums,
   n_circle sqrt(3) eps for the sum of norms, 0 for the force sums).
   The measured maxima are printed (DESIGN.md §16 records them: at most 6.4
   units of 2^-53 S against the bound of 88).  Every run has samples in and
   out of the contact phase.  The classical fleet makes contact in these 40
   ticks and its runs assert so; the force-feedback fleet, from t0 = 0.7 with
   this horizon, does not reach the table within them (measured: normal force
   0 in every instance and tick, in both modes), so its runs assert that the
   device counts no contact where the logs show none, and check the tracking
   sums and the counters.
3. The same loop without logs (steps = 4, 40 ticks): the same accumulators;
   a state saved at tick 17 continues to them in a fresh loop.
4. run_sweep(device_summary=True) against the logged summary."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_fleet_tasks_cpu as TC  # noqa: E402  (the tasks)
import test_gpu_fleet_loop_kernels as KT  # noqa: E402  (synthetic observations)
import test_gpu_fleet_tasks as TG  # noqa: E402  (the heterogeneous loop)
from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import uncertainty as U  # noqa: E402
from ffddp.config import classical_preset  # noqa: E402
from ffddp.runlog import accumulate_metrics, metrics_accumulators, metrics_from_accumulators, summary_metrics  # noqa: E402
from ffddp.trajectory import sample_records, task_records  # noqa: E402

TOL_REF = TG.TOL_REF
U53 = 2.0 ** -53
SENTINEL = KT.SENTINEL
F = {k: i for i, k in enumerate(_abi.FLEET_METRICS_FIELDS)}
COUNTERS = ("unstable_ticks", "neg_accepted_ticks", "not_ok_ticks", "solved_ticks")
_dev = TG._dev


# -- 1. the kernel alone --------------------------------------------------------------------
def _kernel_inputs(rng, B):
    _, od, rec = KT._observations(rng, B, True)
    info = rng.normal(size=(B, _abi.FLEET_INFO_W))
    info[:, 0], info[:, 4], info[:, 7] = rng.random(B) < 0.8, rng.random(B) < 0.2, rng.integers(0, 3, B)
    need = (rng.random(B) < 0.4).astype(np.uint8)
    fail = (rng.random(B) < 0.05).astype(np.int32)
    return od["obs"], rec, info, need, fail


def _sampler_positions(solver, rec_d, ts):
    """The device sampler's knot 0 at ts with a zero site offset, mapped back to the world frame (exact)."""
    node, _ = TG._sample_dev(solver, rec_d, np.zeros(3), ts)
    return np.stack([-node[:, 0, 0], -node[:, 0, 1], node[:, 0, 2]], 1)


def test_metrics_kernel_matches_accumulate_metrics():
    B, ld, calls, dt, fn_des = 300, 320, 24, 0.005, 1.5  # two blocks, the second partly filled
    base = TC.make_tasks()
    tasks = [dataclasses.replace(base[b % 6], delay=(b % 7) * 0.0013) for b in range(B)]  # no multiples of dt
    rec = task_records(tasks)
    rec_d = _dev(rec)
    t_phase = np.array([float(k.t_contact_phase) for k in tasks])
    t_phase[5::11] = np.inf  # instances without a contact phase
    solver = BatchedBoxFDDP(classical_preset(TG.HORIZON), max_batch=B, device=0)
    rng = np.random.default_rng(23)
    acc_d = _dev(metrics_accumulators(B, ld))
    acc_d[:, B:] = SENTINEL
    acc = metrics_accumulators(B, ld)
    acc[:, B:] = SENTINEL
    tp_d = _dev(t_phase)
    ktasks = solver.fleet_tasks(rec_d, np.zeros(3))
    circle = phase_seen = 0
    for k in range(calls):
        t = 0.3 + 0.04 * k
        obs_d, obs, info, need, fail = _kernel_inputs(rng, B)
        if k == 7:  # a NaN force with the flag up, a NaN position, a NaN force with the flag down
            obs[3, 46], obs[3, 47], obs[9, 29], obs[200, 46], obs[200, 47] = np.nan, 1.0, np.nan, np.nan, 0.0
            obs_d.copy_(_dev(obs))
        ts = (t - rec[:, -1]) + dt
        p_ref = _sampler_positions(solver, rec_d, ts)
        assert np.max(np.abs(p_ref - sample_records(rec, ts)[0])) <= TOL_REF
        accumulate_metrics(acc, obs, p_ref, ts, t_phase, fn_des, info, need, fail)
        ktasks.t = t
        solver.fleet_metrics_dev(acc_d, obs_d, tp_d, fn_des, tasks=ktasks, dt=dt, info=_dev(info), need=_dev(need),
                                 plant_fail=_dev(fail))
        circle += int((ts >= rec[:, 20]).sum())
        phase_seen += int((ts >= t_phase).sum())
    torch.cuda.synchronize()
    got = acc_d.cpu().numpy()
    assert circle > 0 and 0 < phase_seen < B * calls
    assert np.all(got[:, B:] == SENTINEL)  # the tail beyond B is untouched
    for name, i in F.items():
        assert np.array_equal(got[i, :B], acc[i, :B], equal_nan=True), (name, np.nanmax(np.abs(got[i, :B] - acc[i, :B])))
    assert np.all(got[F["sum_contact_phase"], :3] > 0) and np.all(got[F["sum_contact"], :3] > got[F["sum_contact_phase"], :3])
    assert np.all(got[F["n"], :B] == calls) and np.all(got[F["n_phase"], 5::11][: B // 11] == 0)
    # NaN propagates into the sums and, as in np.max, into both maxima -- and only where it entered
    assert np.isnan(got[F["max_fn"], 3]) and np.isnan(got[F["sum_abs_fn_err"], 3]) and np.isfinite(got[F["sum_3d2"], 3])
    assert np.isnan(got[F["max_fn"], 200]) and np.isfinite(got[F["max_err_3d"], 200])
    assert np.isnan(got[F["max_err_3d"], 9]) and np.isnan(got[F["sum_tan2"], 9]) and np.isfinite(got[F["max_fn"], 9])
    assert np.isfinite(got[:, :B][:, [0, 1, 2, 299]]).all()

    # the table mode: one shared reference row and time; info = NULL leaves the four counters, need = NULL solves all
    acc2_d, acc2 = _dev(metrics_accumulators(B, ld)), metrics_accumulators(B, ld)
    for k in range(3):
        obs_d, obs, info, need, fail = _kernel_inputs(rng, B)
        p, ts1 = rng.normal(0.0, 0.3, 3), 0.79 + 0.005 * k
        kw = [dict(), dict(info=info), dict(info=info, need=need, plant_fail=fail)][k]
        accumulate_metrics(acc2, obs, p, ts1, t_phase, fn_des, **kw)
        solver.fleet_metrics_dev(acc2_d, obs_d, tp_d, fn_des, p_ref=_dev(p), ts=ts1, **{a: _dev(v) for a, v in kw.items()})
        if k == 0:
            torch.cuda.synchronize()
            assert not acc2_d.cpu().numpy()[[F[c] for c in COUNTERS + ("plant_fail",)]].any()
    torch.cuda.synchronize()
    got2 = acc2_d.cpu().numpy()
    assert np.array_equal(got2, acc2, equal_nan=True)
    assert np.all(got2[F["solved_ticks"], :B] == 1.0 + (need != 0)) and 0 < got2[F["n_phase"], :B].sum() < 3 * B

    # fewer records than instances: the others have no reference (NaN errors, the force fields go on), no read past them
    rows = B - 10
    acc3_d, acc3 = _dev(metrics_accumulators(B, ld)), metrics_accumulators(B, ld)
    obs_d, obs, info, need, fail = _kernel_inputs(rng, B)
    rec_short = _dev(rec[:rows])  # its own allocation, rows records long
    short = solver.fleet_tasks(rec_short, np.zeros(3), 0.9)
    ts = (0.9 - rec[:, -1]) + dt
    p_ref = _sampler_positions(solver, rec_d, ts)
    ts[rows:], p_ref[rows:] = np.nan, np.nan
    accumulate_metrics(acc3, obs, p_ref, ts, t_phase, fn_des)
    solver.fleet_metrics_dev(acc3_d, obs_d, tp_d, fn_des, tasks=short, dt=dt, rows=rows)
    torch.cuda.synchronize()
    got3 = acc3_d.cpu().numpy()
    assert np.array_equal(got3, acc3, equal_nan=True)
    assert np.all(np.isnan(got3[F["sum_3d2"], rows:B])) and np.all(np.isfinite(got3[F["max_fn"], rows:B]))
    assert np.all(got3[F["n"], rows:B] == 1.0) and not got3[F["n_phase"], rows:B].any()

    # argument checks
    lib, h, p = solver._lib, solver._h, obs_d.data_ptr()
    call = lambda B_=B, ld_=ld, obs_=p, ldo=_abi.PLANT_OBS, T=ktasks, pr=None, tp=p, acc_=p: (  # noqa: E731
        lib.ffddp_fleet_metrics_dev(h, B_, ld_, obs_, ldo, T, B, dt, pr, 0.0, tp, fn_des, None, None, None, acc_, None))
    assert call(B_=0) == -1 and call(obs_=None) == -1 and call(tp=None) == -1 and call(acc_=None) == -1
    assert call(T=_abi.FleetTasks()) == -1  # neither a record pointer nor a reference row
    assert call(ld_=B - 1) == -1 and call(ldo=47) == -1
    assert call(B_=B + 1, ld_=B + 1) == -4
    assert lib.ffddp_fleet_metrics_dev(None, B, ld, p, 69, ktasks, B, dt, None, 0.0, p, fn_des, None, None, None, p, None) == -1
    torch.cuda.synchronize()
    solver.close()


# -- 2. / 3. the loop -----------------------------------------------------------------------
TICKS = TG.HET_TICKS
CASES = [("classical", "inject"), ("ff", "inject"), ("classical", "period3"), ("ff", "period3")]


def _case_kw(mode):
    if mode == "inject":
        ucfgs = [U.UncertaintyProfileConfig(seed=100 + b) if b in (1, 4) else None for b in range(TG.B)]
        return dict(uncertainty=ucfgs, noise="philox")
    return dict(solve_period=3)


@functools.lru_cache(maxsize=None)
def _logged(variant, mode):
    """The logged loop with metrics: its results, shared by tests 2 and 3 and left unchanged."""
    loop = TG._loop(variant, "trajectory", TICKS, tasks=TG._het_tasks(), metrics=True, **_case_kw(mode))
    loop.run(TICKS)
    r = loop.results()
    fn_des, dt = float(loop.cfg.fn_des), loop.dt
    loop.close()
    return r, fn_des, dt


def _numpy_summary(r, tasks, fn_des, dt):
    """fleet._run_sweep_device's numpy code on the logs r: the series, summary_metrics per instance, the counters."""
    rec = task_records(tasks)
    steps, B = r["t_task"].shape
    t_series = r["t_task"] + dt
    p_ref = np.stack([sample_records(rec, t_series[k])[0] for k in range(steps)])
    t_cps = np.array([float(k.t_contact_phase) for k in tasks])
    obs = r["obs"][1:]
    err = obs[:, :, 0:3] - p_ref
    fnm = obs[:, :, 3] * (obs[:, :, 4] > 0.5)
    series = dict(t=t_series, err_tan=np.linalg.norm(err[:, :, :2], axis=2), err_3d=np.linalg.norm(err, axis=2),
                  fn_meas=fnm, contact=(fnm > 0.5).astype(float))
    per = [summary_metrics(series["t"][:, b], series["err_tan"][:, b], series["err_3d"][:, b], series["fn_meas"][:, b],
                           series["contact"][:, b], fn_des, float(t_cps[b])) for b in range(B)]
    summ = {k: np.array([s[k] for s in per]) for k in per[0]}
    summ.update(unstable_ticks=(r["unstable"] != 0).sum(0).astype(float),
                neg_accepted_ticks=(r["neg_accepted"] > 0).sum(0).astype(float),
                solve_not_ok_ticks=(r["ok"] == 0).sum(0).astype(float), solved_ticks=r["solved"].sum(0).astype(float),
                max_err_3d=series["err_3d"].max(0))
    phase = t_series >= t_cps[None, :]
    circle = t_series >= rec[None, :, 20]
    return summ, series, phase, circle


@pytest.mark.parametrize("variant,mode", CASES)
def test_loop_summary_equals_the_numpy_summary_of_its_logs(variant, mode):
    r, fn_des, dt = _logged(variant, mode)
    tasks = TG._het_tasks()
    want, series, phase, circle = _numpy_summary(r, tasks, fn_des, dt)
    got, acc = r["summary"], r["metrics"]
    B, n = TG.B, TICKS
    assert acc.shape == (_abi.FLEET_METRICS_W, B) and np.all(acc[F["n"]] == n)
    # the run shows something: samples in and out of the contact phase, contact made, finite logs
    print(f"{variant} {mode}: ticks in contact {acc[F['sum_contact']]}, max fn {acc[F['max_fn']]}, in phase {phase.sum(0)}")
    assert phase.any() and (~phase).any() and np.array_equal(acc[F["n_phase"]], phase.sum(0).astype(float))
    # contact: the classical fleet reaches the table in these 40 ticks (measured: 0 to 18 ticks in contact per
    # instance, forces up to 980 N), the force-feedback fleet does not (measured: normal force 0 in every
    # instance and tick, with the injector and with period 3) -- its runs check the tracking sums and the counters,
    # and that the device counts no contact where the logs show none
    assert np.any(acc[F["sum_contact"]] > 0) == np.any(series["contact"] > 0) == (variant == "classical")
    assert np.all(np.isfinite(r["obs"])) and not np.any(r["plant_fail"]) and not acc[F["plant_fail"]].any()
    if mode == "period3":
        assert 0 < acc[F["solved_ticks"]].sum() < B * n
    # exact: counters, maxima, percentages
    for k in ("unstable_ticks", "neg_accepted_ticks", "solve_not_ok_ticks", "solved_ticks", "max_fn", "max_err_3d",
              "contact_loss_pct", "contact_loss_contact_phase_pct"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])
    # the sums: (2 n + 8) u S + c
    e_max, n_circle = series["err_3d"].max(0), circle.sum(0)
    c2 = n_circle * (2.0 * e_max * np.sqrt(3.0) * TOL_REF + 3.0 * TOL_REF ** 2)
    c1 = n_circle * np.sqrt(3.0) * TOL_REF
    fe = np.abs(series["fn_meas"] - fn_des)
    sums = dict(sum_tan2=(series["err_tan"] ** 2, None, c2), sum_3d2=(series["err_3d"] ** 2, None, c2),
                sum_abs_tan=(np.abs(series["err_tan"]), None, c1), sum_abs_fn_err=(fe, None, 0.0),
                sum_tan2_phase=(series["err_tan"] ** 2, phase, c2), sum_fn_phase=(series["fn_meas"], phase, 0.0),
                sum_contact=(series["contact"], None, 0.0), sum_contact_phase=(series["contact"], phase, 0.0))
    worst, tol_s = 0.0, {}
    for name, (terms, mask, c) in sums.items():
        c = np.broadcast_to(c, (B,))
        for b in range(B):
            x = terms[:, b] if mask is None else terms[mask[:, b], b]
            s_np, m = float(np.sum(x)), x.size
            tol = (2 * m + 8) * U53 * s_np + c[b]
            tol_s[name, b] = tol
            d = abs(acc[F[name], b] - s_np)
            worst = max(worst, d / (U53 * s_np) if s_np > 0 else 0.0)
            assert d <= tol, (name, b, acc[F[name], b], s_np, tol)
    print(f"{variant} {mode}: max |S_dev - S_np| = {worst:.2f} x 2^-53 S_np (bound {2 * n + 8}), circle samples "
          f"{int(n_circle.sum())}")
    # the summary values the sums determine: the sum's tolerance through the value's derivative in the sum
    worst_v = 0.0
    n_p = phase.sum(0)
    for k, name, m, root in (("rms_tangential_error", "sum_tan2", np.full(B, n), True),
                             ("rms_3d_error", "sum_3d2", np.full(B, n), True),
                             ("rms_tangential_error_contact_phase", "sum_tan2_phase", n_p, True),
                             ("avg_abs_position_err", "sum_abs_tan", np.full(B, n), False),
                             ("avg_abs_force_err", "sum_abs_fn_err", np.full(B, n), False),
                             ("fn_mean_contact_phase", "sum_fn_phase", n_p, False)):
        for b in range(B):
            assert np.isnan(got[k][b]) == np.isnan(want[k][b]) == (m[b] == 0), (k, b)
            if m[b] == 0 or want[k][b] == 0.0:
                assert m[b] == 0 or got[k][b] == 0.0
                continue
            tol = tol_s[name, b] / m[b] / (2.0 * want[k][b] if root else 1.0)
            d = abs(got[k][b] - want[k][b])
            worst_v = max(worst_v, d / (U53 * abs(want[k][b])))
            assert d <= tol, (k, b, got[k][b], want[k][b], tol)
    print(f"{variant} {mode}: max |summary_dev - summary_np| = {worst_v:.2f} x 2^-53 |value|")
    # the summary is the accumulators' (nothing else enters it)
    again = metrics_from_accumulators(acc)
    assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in got)


@pytest.mark.parametrize("variant,mode", [("classical", "period3"), ("ff", "inject")])
def test_loop_without_logs_runs_past_steps_to_the_same_accumulators(variant, mode):
    r, _, _ = _logged(variant, mode)
    kw = dict(tasks=TG._het_tasks(), metrics=True, logs=False, **_case_kw(mode))
    a = TG._loop(variant, "trajectory", 4, **kw)  # sized for 4 ticks: without logs nothing is
    assert a.unbounded and a.log_info.shape[0] == 1 and a.log_obs.shape[0] == 1 and a.log_need.shape[0] == 1
    a.run(17)
    s17 = a.state()
    assert s17["k"] == 17 and s17["metrics_k"] == 16 and not s17["stepped"]
    a.run(TICKS - 17)
    ra = a.results()
    assert set(ra) == {"ticks", "plant_fail", "metrics", "summary"} | ({"inject_a", "inject_b"} if mode == "inject" else set())
    assert ra["ticks"] == TICKS and np.array_equal(ra["plant_fail"], r["plant_fail"])
    assert np.array_equal(ra["metrics"], r["metrics"], equal_nan=True)
    rb = a.results()  # twice: the closing plant step and its fold happen once
    assert np.array_equal(rb["metrics"], ra["metrics"], equal_nan=True) and a.m_k == TICKS
    assert all(np.array_equal(rb["summary"][k], r["summary"][k], equal_nan=True) for k in r["summary"])
    a.close()
    b = TG._loop(variant, "trajectory", 4, **kw)
    b.load_state(s17)
    b.run(TICKS - 17)
    assert np.array_equal(b.results()["metrics"], r["metrics"], equal_nan=True)
    b.close()


def test_a_table_still_bounds_the_run_without_logs():
    ee = TG._scene()[0]
    a = TG._loop("classical", "trajectory", 4, traj=TG.benchmark_traj(ee)[0], metrics=True, logs=False, t_contact_phase=0.8)
    assert not a.unbounded
    a.run(4)
    with pytest.raises(RuntimeError, match="sized for 4 ticks"):
        a.run(1)
    r = a.results()
    assert r["ticks"] == 4 and np.all(r["metrics"][F["n"]] == 4) and np.all(np.isfinite(r["summary"]["rms_3d_error"]))
    a.close()


# -- 4. the sweep ---------------------------------------------------------------------------
def test_sweep_with_device_summary():
    kw = dict(device_loop=True, device_refs=True, seeds=2, total_time=0.2, scenarios=("flat", "tilted_10"), verbose=False)
    logged = FL.run_sweep(**kw)
    dev = FL.run_sweep(device_summary=True, **kw)
    n = dev["ticks"]
    assert n == logged["ticks"] and n >= 39 and np.array_equal(dev["solved_ticks"], logged["solved_ticks"])
    assert dev["solved"].shape == (n, 4)
    worst = 0.0
    for k in FL.SUMMARY_KEYS:  # 0.2 s stays in the pre phase: numpy's references, c = 0
        a, b = dev["per_instance"][k], logged["per_instance"][k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(b)
        assert np.all(np.abs(a[ok] - b[ok]) <= (2 * n + 8) * U53 * np.abs(b[ok])), (k, a, b)
        if ok.any() and np.all(b[ok] != 0):
            worst = max(worst, float(np.max(np.abs(a[ok] - b[ok]) / (U53 * np.abs(b[ok])))))
    print(f"sweep: max |dev - logged| = {worst:.2f} x 2^-53 |value| (bound {2 * n + 8})")
    for k in ("max_fn", "unstable_ticks", "neg_accepted_ticks", "solve_not_ok_ticks"):
        assert np.array_equal(dev["per_instance"][k], logged["per_instance"][k]), k
    assert np.all(np.isfinite(dev["per_instance"]["rms_3d_error"]))
    bare = FL.run_sweep(device_summary=True, keep_logs=False, **kw)
    assert "solved" not in bare and "surface" not in bare
    for k in FL.SUMMARY_KEYS:
        assert np.array_equal(bare["per_instance"][k], dev["per_instance"][k], equal_nan=True), k
    assert np.array_equal(bare["solved_ticks"], dev["solved_ticks"])
