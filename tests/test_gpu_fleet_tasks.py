"""GPU: per-instance tasks and start delays in the device fleet loop.

1. The device task sampler alone (ffddp_fleet_task_refs_dev) against
   trajectory.sample_records: flags exact, every entry of a knot outside the
   circle phase bit for bit (the sampler is compiled without contraction in
   trajectory.py's order), circle-phase entries within TOL_REF = 1e-13
   (tests/test_gpu_build.py's bound for the device sincos against numpy's).
2. ffddp_fleet_pre_task_dev against the standalone sampler (references, hint)
   and, instance by instance, against ffddp_fleet_pre_dev /
   ffddp_fleet_pre_sched_dev fed that instance's references and hint.
3. DeviceFleetLoop(tasks=one task) against a table loop whose table the
   sampler tabulated (the test's own substitution): every log and the final
   state are equal.
4. A heterogeneous fleet (radii, speeds, delays): single instances against
   table loops, the switches spread over the ticks, the solves of a period-3
   loop spread over the residues, and an injected run reproducible.
5. run_sweep(device_refs=..., task_spread=..., stagger=...)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_fleet_tasks_cpu as TC  # noqa: E402  (the tasks and the times)
import test_gpu_fleet_loop_kernels as KT  # noqa: E402  (synthetic state and observations)
from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import controller as CT  # noqa: E402
from ffddp import fleet as FL  # noqa: E402
from ffddp import plant as PL  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp import uncertainty as U  # noqa: E402
from ffddp.config import classical_preset, ff_preset  # noqa: E402
from ffddp.fleet_loop import DeviceFleetLoop  # noqa: E402
from ffddp.trajectory import benchmark_task, benchmark_traj, sample_records, task_records  # noqa: E402

TOL_REF = 1e-13  # tests/test_gpu_build.py: device sincos against numpy's
P_OFF = np.array([0.0125, -0.021, 0.1034])
B, HORIZON, T0 = 6, 8, 0.7
SENTINEL = KT.SENTINEL


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _frame(P, V, p_off):
    """k_build's frame map: R_MJ_FROM_PIN = diag(-1, -1, 1), minus p_site_minus_frame."""
    return np.stack([-P[:, 0] - p_off[0], -P[:, 1] - p_off[1], P[:, 2] - p_off[2], -V[:, 0], -V[:, 1], V[:, 2]], 1)


def _oracle(rec, t, N, dt_ocp, p_off):
    """(node_ref [n][N+1][6], surface [n][N+1], circle [n][N+1]) by sample_records at t + k dt_ocp."""
    n = rec.shape[0]
    ref, surf, circ = np.zeros((n, N + 1, 6)), np.zeros((n, N + 1), bool), np.zeros((n, N + 1), bool)
    for k in range(N + 1):
        tk = t + k * dt_ocp
        P, V, S = sample_records(rec, tk)
        ref[:, k], surf[:, k] = _frame(P, V, p_off), S
        circ[:, k] = S & ~(tk < rec[:, 20])
    return ref, surf, circ


def _sample_dev(solver, rec_d, p_off, t):
    n = t.shape[0]
    node = torch.full((n, solver.N + 1, 6), SENTINEL, dtype=torch.float64, device="cuda")
    hint = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    solver.fleet_task_refs_dev(solver.fleet_tasks(rec_d, p_off), _dev(t), node, hint)
    torch.cuda.synchronize()
    return node.cpu().numpy(), hint.cpu().numpy()


# -- 1. the sampler alone -------------------------------------------------------------------
def test_task_sampler_matches_sample_records():
    tasks = TC.make_tasks()
    rec1 = task_records(tasks)
    rows, times = [], []
    for b, task in enumerate(tasks):
        t = TC.task_times(task)
        rows.append(np.repeat(rec1[b:b + 1], t.size, 0))
        times.append(t)
    rec, t = np.concatenate(rows), np.concatenate(times)
    n = t.size  # 6 tasks x 65 times: more than one block of 256 (instance, knot) threads
    solver = BatchedBoxFDDP(classical_preset(HORIZON), max_batch=n, device=0)
    dt_ocp = float(solver.cfg.dt)
    got, hint = _sample_dev(solver, _dev(rec), P_OFF, t)
    ref, surf, circ = _oracle(rec, t, HORIZON, dt_ocp, P_OFF)
    assert np.array_equal(hint != 0, surf[:, 0]) and set(hint.tolist()) == {0, 1}
    assert circ.any() and (surf & ~circ).any() and (~surf).any() and (t < 0).any()
    exact = ~circ
    assert np.array_equal(got[exact], ref[exact]), float(np.max(np.abs(got[exact] - ref[exact])))
    err = float(np.max(np.abs(got[circ] - ref[circ])))
    print("circle-phase max |dev - numpy| =", err)
    assert err <= TOL_REF
    # argument checks: a null record pointer, a null output
    lib, h, p = solver._lib, solver._h, _dev(t).data_ptr()
    good = solver.fleet_tasks(_dev(rec), P_OFF)
    assert lib.ffddp_fleet_task_refs_dev(h, n, _abi.FleetTasks(), p, p, p, None) == -1
    assert lib.ffddp_fleet_task_refs_dev(h, n, good, None, p, p, None) == -1
    assert lib.ffddp_fleet_task_refs_dev(h, 0, good, p, p, p, None) == -1
    assert lib.ffddp_fleet_task_refs_dev(h, n + 1, good, p, p, p, None) == -4
    torch.cuda.synchronize()
    solver.close()


# -- 2. the pre kernel ----------------------------------------------------------------------
PRE_DELAYS = (0.0, 0.015, 0.0, 0.04, 0.005, 0.1)
PRE_OUT = ("x0", "surface", "inst_ref", "node_ref", "xs_init", "us_init")


def _pre_inputs(rng, variant, N, nx):
    st = KT._state(rng, B, N, nx)
    st["valid"] = np.array([1, 1, 0, 1, 0, 1], np.uint8)
    st["prev_mode"] = np.array([0, 1, -1, 1, 0, 0], np.int8)
    _, od, _ = KT._observations(rng, B, True)
    q_nom = R.Q_NEUTRAL + rng.normal(0.0, 0.2, (B, 7))
    return st, od, q_nom


def _pre_tensors(st, od, q_nom, variant, N, nx, sched):
    t = KT._up(st)
    t.update({k: od[k] for k in ("q", "v", "fn_meas", "ee_z", "contact")})
    if variant == "ff":
        t["tau_hat"] = od["tau_hat"]
    t["q_nom"] = _dev(q_nom)
    full = lambda *s, dtype=torch.float64: torch.full(s, SENTINEL, dtype=dtype, device="cuda")  # noqa: E731
    t.update(x0=full(B, nx), inst_ref=full(B, 21), node_ref=full(B, N + 1, 6), xs_init=full(B, N + 1, nx),
             us_init=full(B, N, 7), surface=torch.full((B,), 7, dtype=torch.uint8, device="cuda"))
    if sched:
        t.update(since=_dev(np.array([0, 1, 2, 2, 0, 1], np.int32)), age=_dev(np.array([0, 1, 2, 9, 0, 3], np.int32)),
                 need=torch.full((B,), 7, dtype=torch.uint8, device="cuda"))
    return t


@pytest.mark.parametrize("variant,sched", [("classical", False), ("ff", False), ("classical", True), ("ff", True)])
def test_pre_task_equals_pre_fed_the_sampler(variant, sched):
    N = HORIZON
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    tasks = [dataclasses.replace(k, delay=d) for k, d in zip(TC.make_tasks(), PRE_DELAYS)]
    rec = task_records(tasks)
    rec_d = _dev(rec)
    delay = rec[:, -1]
    Q = None
    if sched:
        Q = _abi.FleetSched()
        Q.period, Q.apply_filter, Q.dt = 3, 0, 0.005
    rng = np.random.default_rng(11)
    hints_seen, need_seen = set(), set()
    keys = PRE_OUT + (("need",) if sched else ())
    # task times before, at (instance 0 at 0.25 + 0.55) and after the instances' switches; 0.02 gives negative ones
    for t_tick in (0.25 + 0.55, 0.3, 0.02, 1.1):
        for ps in (0, 1):
            P = KT._params(phase_source=ps, posture_mode=ps, torque_mode=ps)
            st, od, q_nom = _pre_inputs(rng, variant, N, nx)
            t_task = t_tick - delay
            node_s, hint_s = _sample_dev(solver, rec_d, P_OFF, t_task)
            ref, surf, _ = _oracle(rec, t_task, N, float(cfg.dt), P_OFF)
            assert np.array_equal(hint_s != 0, surf[:, 0])
            hints_seen |= set(hint_s.tolist())
            a = _pre_tensors(st, od, q_nom, variant, N, nx, sched)
            solver.fleet_pre_dev(a, P, stream=stream, sched=Q, tasks=solver.fleet_tasks(rec_d, P_OFF, t_tick))
            A = KT._down(a, keys + KT.STATE_KEYS)
            tag = (variant, sched, t_tick, ps)
            assert np.array_equal(_bits(A["node_ref"]), _bits(node_s)), tag
            if ps == 0:
                assert np.array_equal(A["surface"], hint_s), tag
            for b in range(B):
                o = _pre_tensors(st, od, q_nom, variant, N, nx, sched)
                o["node_ref1"] = _dev(node_s[b])
                solver.fleet_pre_dev(o, P, bool(hint_s[b]), stream=stream, sched=Q)
                O = KT._down(o, keys + KT.STATE_KEYS)
                for k in keys + KT.STATE_KEYS:
                    assert np.array_equal(A[k][b], O[k][b], equal_nan=True), (tag, b, k)
            if sched:
                need_seen |= set(A["need"].tolist())
    assert hints_seen == {0, 1} and (not sched or need_seen == {0, 1})
    # a null record pointer, and a scheduled call without its counters
    a = _pre_tensors(st, od, q_nom, variant, N, nx, sched)
    with pytest.raises(RuntimeError, match="null pointer"):
        solver.fleet_pre_dev(a, P, stream=stream, sched=Q, tasks=_abi.FleetTasks())
    bad = _abi.FleetSched()
    bad.period = 3
    lib, p = solver._lib, a["x0"].data_ptr()
    st_ = solver._fleet_state(a)
    rc = lib.ffddp_fleet_pre_task_dev(solver._h, B, C.byref(P), C.byref(st_), p, p, p, None, p, 7, 1, p, 7, p,
                                      solver.fleet_tasks(rec_d, P_OFF), p, p, p, p, p, p, C.byref(bad), None)
    assert rc == -1
    torch.cuda.synchronize()
    solver.close()


# -- 3. / 4. the loop -----------------------------------------------------------------------
TILT = np.array([0.0, 5.0, 10.0, 15.0, -5.0, 2.5])
SCALE = np.array([1.0, 0.9, 1.1, 0.95, 1.05, 1.0])[:, None] * np.linspace(0.95, 1.05, 7)


@functools.lru_cache(maxsize=None)
def _scene():
    nominal = PL.PandaTablePlant(n_substeps=5, timestep=0.001)
    obs_n = nominal.reset("neutral")
    ee, cal, dt = obs_n.ee_pos.copy(), FL.site_calibration(obs_n), nominal.dt
    nominal.close()
    return ee, cal, dt


def _loop(variant, phase_source, ticks, traj=None, tasks=None, **kw):
    ee, cal, dt = _scene()
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (B, 7))
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    cfg = make(dt, benchmark_task(ee).z_contact, horizon=HORIZON, phase_source=phase_source)
    return DeviceFleetLoop(variant, B, traj, cfg, q0, tilt_deg=TILT, torque_scale=SCALE, steps=ticks, calibration=cal,
                           t0=T0, tasks=tasks, **kw)


def _tabulate(loop, rec_row, t_task):
    """The table (ticks, N+1, 6) and hints of one record at the task times t_task, by the device sampler."""
    rec_d = _dev(np.repeat(rec_row[None], B, 0))
    p_off = _scene()[1][1]
    table, hints = [], []
    for k0 in range(0, len(t_task), B):
        t = np.resize(t_task[k0:k0 + B], B)  # the last chunk is padded
        node, hint = _sample_dev(loop.solver, rec_d, p_off, t)
        table.append(node)
        hints.append(hint)
    return np.concatenate(table)[: len(t_task)], np.concatenate(hints)[: len(t_task)] != 0


def _table_loop(variant, phase_source, ticks, rec_row, delay, **kw):
    ee = _scene()[0]
    loop = _loop(variant, phase_source, ticks, traj=benchmark_traj(ee)[0], **kw)
    table, hints = _tabulate(loop, rec_row, loop.times - delay)
    loop.ref_table.copy_(_dev(table))
    loop.hints[:] = hints
    return loop


def _equal(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


@pytest.mark.parametrize("variant,phase_source", [("classical", "trajectory"), ("ff", "trajectory"),
                                                  ("classical", "force_latch"), ("ff", "force_latch")])
def test_uniform_task_loop_equals_table_loop(variant, phase_source):
    ticks = 30  # the switch is at tick 20
    ee = _scene()[0]
    task = benchmark_task(ee)
    a = _loop(variant, phase_source, ticks, tasks=task)
    assert a.ref_table is None and a.refs is None and a.hints is None
    b = _loop(variant, phase_source, ticks, traj=task.traj())
    host_hints = b.hints.copy()
    table, hints = _tabulate(b, task_records([task])[0], b.times)
    assert np.array_equal(hints, host_hints) and not hints[19] and hints[20]
    b.ref_table.copy_(_dev(table))
    a.run(ticks)
    b.run(ticks)
    ra, rb = a.results(), b.results()
    assert np.array_equal(ra.pop("t_task"), np.repeat(b.times[:, None], B, 1))
    assert set(ra) == set(rb)
    for k in rb:
        assert _equal(ra[k], rb[k]), (variant, phase_source, k)
    assert np.all(np.isfinite(ra["obs"])) and np.any(ra["surface"] == 0)
    if phase_source == "trajectory":  # the hint is the surface flag; the latch engages on force or near the table
        assert np.array_equal(ra["surface"] != 0, np.repeat(hints[:, None], B, 1))
    sa, sb = a.state(), b.state()
    assert set(sa) == set(sb)
    for k in sb:
        assert _equal(sa[k], sb[k]), (variant, phase_source, k)
    a.close()
    b.close()


HET_TICKS = 40
HET_DELAY_TICKS = np.array([0, 1, 2, 3, 5, 8])


def _het_tasks():
    ee, _, dt = _scene()
    return [benchmark_task(ee, radius=r, omega=w, delay=d * dt)
            for r, w, d in zip(np.linspace(0.06, 0.14, B), np.linspace(1.0, 2.0, B), HET_DELAY_TICKS)]


def _first_surface(surface):
    assert np.all(surface.any(0))
    return np.argmax(surface != 0, 0)


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_heterogeneous_fleet_rows_equal_single_task_table_loops(variant):
    tasks = _het_tasks()
    rec = task_records(tasks)
    a = _loop(variant, "trajectory", HET_TICKS, tasks=tasks)
    a.run(HET_TICKS)
    ra, sa = a.results(), a.state()
    tau_a = a.T["tau_cmd"].cpu().numpy()
    assert np.array_equal(ra["t_task"], a.times[:, None] - rec[None, :, -1])
    # the switches: where sample_records puts them, and on different ticks (the delays 0, 2, 5, 8 ticks are two
    # or more apart, so those four differ whatever the rounding of t - delay does to a single tick)
    flips = _first_surface(ra["surface"])
    want = np.array([np.argmax([sample_records(rec[b], t)[2][0] for t in ra["t_task"][:, b]]) for b in range(B)])
    assert np.array_equal(flips, want), (flips, want)
    assert len(set(flips[[0, 2, 4, 5]].tolist())) == 4 and np.all(np.diff(flips) >= 0) and flips[0] >= 19
    assert np.all(np.isfinite(ra["obs"])) and not np.any(ra["plant_fail"])
    for b in (0, 3, 5):
        o = _table_loop(variant, "trajectory", HET_TICKS, rec[b], rec[b, -1])
        o.run(HET_TICKS)
        ro, so = o.results(), o.state()
        for k in ("info", "obs", "solved"):
            assert _equal(ra[k][:, b], ro[k][:, b]), (variant, b, k)
        assert np.array_equal(tau_a[b], o.T["tau_cmd"].cpu().numpy()[b]), (variant, b)
        for k in ("tau_prev", "keep_xs", "keep_us", "q", "v"):
            assert np.array_equal(sa[k][b], so[k][b]), (variant, b, k)
        o.close()
    a.close()


def test_staggered_fleet_spreads_the_solves_of_a_period():
    tasks = _het_tasks()
    a = _loop("classical", "trajectory", HET_TICKS, tasks=tasks, solve_period=3)
    a.run(HET_TICKS)
    r = a.results()
    flips = _first_surface(r["surface"])
    k0 = int(flips.max()) + 1  # every instance has switched and solved at its switch
    assert HET_TICKS - k0 >= 9
    assert np.all(r["solved"][flips, np.arange(B)])  # a mode switch solves at once
    solved = r["solved"][k0:]
    residues = {int(k % 3) for k in np.nonzero(solved.any(1))[0] + k0}
    per_instance = [{int(k % 3) for k in np.nonzero(solved[:, b])[0] + k0} for b in range(B)]
    print("solving residues", residues, per_instance, "share per tick", solved.mean(1))
    assert len(residues) >= 2
    assert 0.0 < float(solved.mean()) < 1.0
    a.close()


def test_heterogeneous_fleet_with_injector_is_reproducible():
    tasks = _het_tasks()
    ucfgs = [U.UncertaintyProfileConfig(seed=100 + b) if b in (1, 4) else None for b in range(B)]
    a = _loop("classical", "trajectory", HET_TICKS, tasks=tasks, uncertainty=ucfgs, noise="philox", solve_period=3)
    s0 = a.state()
    logs = []
    for _ in range(2):
        a.load_state(s0)
        a.log_info.fill_(float("nan"))
        a.log_obs.fill_(float("nan"))
        a.run(HET_TICKS)
        logs.append(a.results())
    for k in ("info", "obs", "solved", "t_task"):
        assert _equal(logs[0][k], logs[1][k]), k
    assert np.all(np.isfinite(logs[0]["obs"])) and np.all(np.isfinite(logs[0]["inject_a"][[1, 4]]))
    assert len(set(_first_surface(logs[0]["surface"]).tolist())) >= 4
    a.close()


# -- 5. the sweep ---------------------------------------------------------------------------
def test_sweep_with_device_refs_task_spread_and_stagger():
    kw = dict(device_loop=True, seeds=2, total_time=0.2, scenarios=("flat", "tilted_10"), verbose=False)
    table = FL.run_sweep(**kw)
    refs = FL.run_sweep(device_refs=True, **kw)
    whole_run = ("rms_tangential_error", "rms_3d_error", "avg_abs_force_err", "max_fn", "unstable_ticks",
                 "neg_accepted_ticks", "solve_not_ok_ticks")  # the contact-phase keys are NaN: 0.2 s has no contact phase
    for k in whole_run:
        assert np.all(np.isfinite(refs["per_instance"][k])), k
    for k in FL.SUMMARY_KEYS:
        # 0.2 s stays in the pre phase, where the device sampler carries numpy's bits: the same run
        assert np.array_equal(refs["per_instance"][k], table["per_instance"][k], equal_nan=True), k
    assert refs["solved"].shape == (refs["ticks"], 4)
    het = FL.run_sweep(device_refs=True, task_spread=(0.3, 0.3), stagger=4, **kw)
    m = het["per_instance"]["rms_3d_error"]
    assert all(np.all(np.isfinite(het["per_instance"][k])) for k in whole_run)
    for s in ("flat", "tilted_10"):
        sel = het["names"] == s
        assert sel.sum() == 2 and m[sel][0] != m[sel][1], s
    assert not np.array_equal(m, refs["per_instance"]["rms_3d_error"])
