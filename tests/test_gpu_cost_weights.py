"""GPU: per-instance scalar cost weights (cost_w / cost_weights) of the device
solve, of calc_diff and of the device fleet loop.

Three references, none of them stored numbers:
- the same library without the argument (rows that repeat the configuration
  must give its bits);
- a second handle created with one instance's weights in its configuration,
  solving that instance alone: the kernels without the feature, the weight a
  constant;
- the numpy oracle (oracle.fddp.SolverBoxFDDP) over oracle_cfg of that same
  per-instance configuration, at tests/test_gpu_parity.py's tolerances.

Solves run at N = 12, B = 6, maxiter 10 on test_gpu_force_ref.py's SOLVE_CASES:
13 nodes of 16 lanes put nodes of two instances into one k_node wave, 80
rollout lanes per instance do the same in k_forward_g8, B <= 819 runs the row
layout and the wide first pass; the mask test at B = 300 covers the four
slices and the two-groups-per-row layout.  Oracle solves run in spawned
workers that import this module, so nothing at module level touches the
device or imports the product."""
from __future__ import annotations

import copy
import functools
from concurrent.futures import ProcessPoolExecutor
from multiprocessing import get_context
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import fddp, ocp

import test_gpu_force_ref as FR
from test_gpu_force_ref import ISENT, MAXITER, OUT, SENTINEL, SOLVE_CASES, _dev, _fresh_outputs, _host, _inputs, _solve_dev, _torch

pytestmark = pytest.mark.gpu

N_SOLVE, B_SOLVE = 12, 6
FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0)
STAT_COLS = [0, 1, 2, 3, 4, 8, 9]  # [5..7] count line-search passes, which follow the slice's active count
IN_KEYS = ("x0", "node_ref", "inst_ref", "xs_init", "us_init", "surface")


def _scaled_names(variant, contact):
    names = ["w_fn", "w_tangent_pos", "w_tangent_vel", "w_tau", "w_posture", "w_plane_z"]
    if variant == "ff":
        names += ["w_w", "w_y"]
    if contact == "point3d":
        names += ["w_friction_cone"]
    return names


def _factors(variant, contact, B):
    """(B, names) factors from FACTORS; instance 0 has all factors 1."""
    names = _scaled_names(variant, contact)
    rng = np.random.default_rng(31)
    f = rng.choice(FACTORS, size=(B, len(names)))
    f[0] = 1.0
    return names, f


def _cfg_of(cfg, names, factors):
    """cfg with the named weights scaled: the configuration a per-instance handle, and the oracle, take."""
    c = copy.deepcopy(cfg)
    for n, s in zip(names, factors):
        setattr(c, n, float(getattr(cfg, n)) * float(s))
    return c


def _rows(cfg, names, f):
    from ffddp.config import cost_weight_row

    return np.stack([cost_weight_row(cfg, **{n: float(getattr(cfg, n)) * float(s) for n, s in zip(names, f[b])})
                     for b in range(f.shape[0])])


def _sub(b, idx):
    return SimpleNamespace(**{k: np.ascontiguousarray(np.asarray(getattr(b, k))[idx]) for k in IN_KEYS})


# -- the oracle: one configuration per instance ----------------------------------------------
def _solve_one(args):
    ocfg, prob, xs_init, us_init, consts = args
    s = fddp.SolverBoxFDDP(ocfg, prob, box=True, consts=consts)
    ok = s.solve(xs_init, us_init, MAXITER, False)
    st = s.stats
    return dict(ok=bool(ok), iter=int(s.iter), xs=s.xs, us=s.us, K=s.K, cost=float(s.cost), iters_run=st.iters_run,
                trials=st.trials, reg_retries=st.reg_retries, forward_errors=st.forward_errors,
                neg_branch=st.neg_branch, neg_accepted=st.neg_accepted, clamped=st.clamped)


def _oracle_solves(cfgs, batch, consts_list):
    """One oracle solve per (consts, instance), instance i under cfgs[i].  Returns {consts index: [dict per instance]}."""
    from helpers import oracle_cfg, oracle_problem
    from oracle_pool import _workers

    N = cfgs[0].horizon
    jobs = [(oracle_cfg(cfgs[i]), oracle_problem(batch, i, N), np.array(batch.xs_init[i]), np.array(batch.us_init[i]), c)
            for c in consts_list for i in range(len(cfgs))]
    n = _workers(len(jobs))
    if n == 1:
        res = [_solve_one(j) for j in jobs]
    else:
        with ProcessPoolExecutor(max_workers=n, mp_context=get_context("spawn")) as ex:
            res = list(ex.map(_solve_one, jobs))
    return {c: res[c * len(cfgs):(c + 1) * len(cfgs)] for c in range(len(consts_list))}


# -- 1. rows that repeat the configuration ---------------------------------------------------
@pytest.mark.parametrize("surf", [1, 0])
@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_rows_of_the_configuration_reproduce_the_call_without(variant, contact, cone, surf):
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import cost_weight_row
    from helpers import make_batch

    torch = _torch()
    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=41 + surf, surface=surf)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    assert hasattr(solver._lib, "ffddp_solve_batch_wts_dev")
    w = _dev(np.tile(cost_weight_row(cfg), (B, 1)))
    assert tuple(w.shape) == (B, _abi.COST_W)
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    full = torch.full((B, N + 1), float(cfg.fn_des), dtype=torch.float64, device="cuda")
    plain = _solve_dev(solver, b)
    runs = {"rows": _solve_dev(solver, b, cost_weights=w),
            "rows+mask": _solve_dev(solver, b, cost_weights=w, active=ones),
            "rows+fref": _solve_dev(solver, b, cost_weights=w, force_ref=full),
            "rows+mask+fref": _solve_dev(solver, b, cost_weights=w, active=ones, force_ref=full)}
    assert np.all(plain["iters"] > 0) and np.all(plain["xs"] != SENTINEL)
    for tag, r in runs.items():
        for k in OUT:
            assert np.array_equal(r[k], plain[k], equal_nan=True), (tag, k)
    solver.close()


# -- 2. / 3. distinct rows -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distinct(variant, contact, cone):
    """The case's batch solved once with distinct rows, and every instance solved alone by a handle of its own whose
    configuration carries that instance's weights (the kernels without the feature).  Shared by tests 2 and 3."""
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=43, surface=1)
    names, f = _factors(variant, contact, B)
    rows = _rows(cfg, names, f)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    got = _solve_dev(solver, b, cost_weights=_dev(rows))
    plain = _solve_dev(solver, b)
    solver.close()
    cfgs = [_cfg_of(cfg, names, f[i]) for i in range(B)]
    alone = []
    for i in range(B):
        s = BatchedBoxFDDP(cfgs[i], max_batch=1)
        alone.append(_solve_dev(s, _sub(b, [i])))
        s.close()
    return SimpleNamespace(cfg=cfg, cfgs=cfgs, batch=b, names=names, f=f, rows=rows, got=got, plain=plain, alone=alone)


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_equal_per_configuration_handles(variant, contact, cone):
    import test_gpu_parity as TP
    from helpers import elem_err, rel_err

    d = _distinct(variant, contact, cone)
    key = (variant, contact, 1, cone)
    tol, tol_k = TP.CASE_TOL.get(key, (TP.TOL_SOLVE, TP.TOL_K))
    tol_ke = TP.CASE_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
    got = d.got
    assert np.all(d.f[0] == 1.0) and len({tuple(r) for r in d.f}) == B_SOLVE
    bits = True
    for i, a in enumerate(d.alone):
        assert got["iters"][i] == a["iters"][0] and got["ok"][i] == a["ok"][0], i
        assert np.array_equal(got["stats"][i][STAT_COLS], a["stats"][0][STAT_COLS]), i
        e = {k: rel_err(got[k][i], a[k][0]) for k in ("xs", "us", "cost", "fn_pred")}
        e_k, e_ke = rel_err(got["K"][i], a["K"][0]), elem_err(got["K"][i], a["K"][0])
        assert all(v < tol for v in e.values()) and e_k < tol_k and e_ke < tol_ke, (i, e, e_k, e_ke)
        bits = bits and all(np.array_equal(got[k][i], a[k][0], equal_nan=True) for k in ("xs", "us", "K", "cost", "fn_pred"))
    print("distinct rows against per-configuration handles: bit-identical =", bits)
    # only the source of a weight changes, so the batch's instance is the per-configuration handle's, bit for bit
    assert bits
    # the rows matter: instance 0 (all factors 1) is the plain solve's, the others are not
    assert all(np.array_equal(got[k][0], d.plain[k][0], equal_nan=True) for k in ("xs", "us", "K", "cost", "iters"))
    assert all(np.any(got["xs"][i] != d.plain["xs"][i]) for i in range(1, B_SOLVE))


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_match_oracle(variant, contact, cone):
    """test_gpu_parity.test_solve_matches_oracle's checks and tolerance table, one oracle solve per instance under
    that instance's configuration; no instance is left out.  The per-configuration handles of the test above (the
    kernels without the feature) are held to the same table first, so an excess of the batch would be the feature's."""
    import test_gpu_parity as TP

    d = _distinct(variant, contact, cone)
    key = (variant, contact, 1, cone)
    name = f"wts/{variant}/{contact}/cone{cone}"
    handles = {k: np.stack([a[k][0] for a in d.alone]) for k in OUT}
    if key in TP.CROCODDYL_FORM_TOL:
        ref = _oracle_solves(d.cfgs, d.batch, [TP.SOLVE_FORM, None])
        tight, tight_k = TP.CASE_TOL.get(key, (TP.TOL_SOLVE, TP.TOL_K))
        tight_ke = TP.CASE_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        tol, tol_k = TP.CROCODDYL_FORM_TOL[key]
        tol_ke = TP.CROCODDYL_FORM_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        for tag, o in (("handles", handles), ("rows", d.got)):
            s = FR._as_solver(o)
            TP._check_solves(f"{name}/{tag}/solve_form", d.cfg, d.batch, s, ref[0], tight, tight_k, tight_ke)
            TP._check_solves(f"{name}/{tag}/crocoddyl_form", d.cfg, d.batch, s, ref[1], tol, tol_k, tol_ke)
        return
    ref = _oracle_solves(d.cfgs, d.batch, [None])[0]
    for tag, o in (("handles", handles), ("rows", d.got)):
        TP._check_solves(f"{name}/{tag}", d.cfg, d.batch, FR._as_solver(o), ref, TP.TOL_SOLVE, TP.TOL_K, TP.TOL_K_ELEM)


# -- 4. calc_diff ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,contact,surf,cone", FR.NODE_CASES)
def test_calc_diff_with_distinct_rows_matches_oracle(variant, contact, surf, cone):
    import test_gpu_parity as TP
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, oracle_cfg, oracle_problem, rel_err

    N, B = 4, 3
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=11 + surf, surface=surf)
    names = _scaled_names(variant, contact if cone else "normal_1d") + ["w_ee_pos", "w_ee_ori", "w_v", "w_unilateral"]
    f = np.random.default_rng(32).choice(FACTORS, size=(B, len(names)))
    f[0] = 1.0
    rows = _rows(cfg, names, f)
    rng = np.random.default_rng(7)
    xs = b.xs_init + 0.02 * rng.normal(size=b.xs_init.shape)
    us = b.us_init + 0.5 * rng.normal(size=b.us_init.shape)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    out = solver.calc_diff(b, xs, us, cost_weights=rows)
    worst = {}
    for i in range(B):
        ocfg = oracle_cfg(_cfg_of(cfg, names, f[i]))
        prob = oracle_problem(b, i, N)
        run = ocp.running_eval(ocfg, prob, slice(0, N), xs[i, :N], us[i], True)
        term = ocp.terminal_eval(ocfg, prob, xs[i, N], True)
        errs = {k: rel_err(out[k][i, :N], run[k]) for k in ("Fx", "Fu", "Lx", "Lu", "Lxx", "Lxu", "Luu", "cost", "xnext")}
        errs["Lx_T"] = rel_err(out["Lx"][i, N], term["Lx"])
        errs["Lxx_T"] = rel_err(out["Lxx"][i, N], term["Lxx"])
        errs["cost_T"] = rel_err(out["cost"][i, N], term["cost"])
        if surf:
            errs["lam"] = rel_err(out["lam"][i, :N, :ocfg.nc], run["lam"])
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    print("calc_diff worst", worst)
    for k, e in worst.items():
        assert e < TP.TOL_NODE, (k, e)
    # rows of the configuration are the call without, with and without a force_ref of fn_des; distinct rows are not
    plain = solver.calc_diff(b, xs, us)
    same = solver.calc_diff(b, xs, us, cost_weights=_rows(cfg, names, np.ones_like(f)))
    both = solver.calc_diff(b, xs, us, cost_weights=_rows(cfg, names, np.ones_like(f)),
                            force_ref=np.full((B, N + 1), float(cfg.fn_des)))
    for k in out:
        assert np.array_equal(same[k], plain[k], equal_nan=True) and np.array_equal(both[k], plain[k], equal_nan=True), k
        assert np.array_equal(out[k][0], plain[k][0], equal_nan=True), k
    assert np.all(out["cost"][1:] != plain["cost"][1:])
    solver.close()


# -- 5. mask, four slices, the two-groups-per-row layout -------------------------------------
@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_masked_rows_equal_their_own_batch(variant):
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, product_cfg

    torch = _torch()
    N, B = 8, 300
    cfg = product_cfg(variant, N)
    b = make_batch(variant, B, N, seed=1234)
    assert 0 < int(np.sum(np.asarray(b.surface) != 0)) < B
    names = _scaled_names(variant, "normal_1d") + ["w_ee_pos"]
    f = np.random.default_rng(33).choice(FACTORS, size=(B, len(names)))
    rows = _rows(cfg, names, f)
    mask = np.zeros(B, np.uint8)
    mask[::3] = 1
    on = mask != 0
    small = BatchedBoxFDDP(cfg, max_batch=int(on.sum()))
    alone = _solve_dev(small, _sub(b, on), cost_weights=_dev(rows[on]))
    small.close()
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    t = _inputs(b)
    off = torch.from_numpy(~on).cuda()
    t["xs_init"][off] = float("nan")
    t["us_init"][off] = float("nan")
    rp = rows.copy()
    rp[~on] = np.nan
    t.update(_fresh_outputs(B, N, cfg.nx))
    sent = _host(t)
    solver.solve_dev(t, maxiter=MAXITER, active=_dev(mask), cost_weights=_dev(rp))
    got = _host(t)
    for k in OUT:
        a, r = (got[k][on], alone[k]) if k != "stats" else (got[k][on][:, STAT_COLS], alone[k][:, STAT_COLS])
        assert np.array_equal(a, r, equal_nan=True), k
        assert np.array_equal(got[k][~on], sent[k][~on], equal_nan=True), k
    assert np.all(np.isfinite(got["xs"][on])) and len(np.unique(got["iters"][on])) > 1
    plain = _solve_dev(solver, b)
    assert np.any(plain["xs"][on] != got["xs"][on])
    solver.close()


# -- 6. a term the handle does not build -----------------------------------------------------
@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_entries_of_absent_terms_are_not_used(variant):
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import cost_weight_row
    from helpers import make_batch, product_cfg

    N, B = N_SOLVE, B_SOLVE
    cfg = product_cfg(variant, N)
    cfg.w_vz = 0.0
    b = make_batch(variant, B, N, seed=45, surface=1)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    rows = np.tile(cost_weight_row(cfg), (B, 1))
    rng = np.random.default_rng(34)
    absent = ["w_vz", "w_friction_cone"] + ([] if variant == "ff" else ["w_w", "w_w_soft_limits", "w_y"])
    for n in absent:  # the handle builds none of these: normal_1d has no cone, the classical solve no augmentation
        assert rows[0, _abi.COST_INDEX[n]] == 0.0
        rows[:, _abi.COST_INDEX[n]] = rng.uniform(1.0, 900.0, B)
    plain = _solve_dev(solver, b)
    got = _solve_dev(solver, b, cost_weights=_dev(rows))
    for k in OUT:
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    d = solver.calc_diff(b, b.xs_init, b.us_init)
    dw = solver.calc_diff(b, b.xs_init, b.us_init, cost_weights=rows)
    for k in d:
        assert np.array_equal(dw[k], d[k], equal_nan=True), k
    # an entry of 0 for a term that exists is legal: the term contributes zeros
    rows0 = np.tile(cost_weight_row(cfg, w_fn=0.0), (B, 1))
    cfg0 = copy.deepcopy(cfg)
    got0 = _solve_dev(solver, b, cost_weights=_dev(rows0))
    assert np.all(np.isfinite(got0["xs"])) and np.any(got0["xs"] != plain["xs"])
    cfg0.w_fn = 0.0
    s0 = BatchedBoxFDDP(cfg0, max_batch=B)
    ref0 = _solve_dev(s0, b)
    s0.close()
    assert np.array_equal(got0["iters"], ref0["iters"]) and np.allclose(got0["xs"], ref0["xs"], rtol=0.0, atol=1e-9)
    solver.close()


# -- 7. errors -------------------------------------------------------------------------------
def test_errors():
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import cost_weight_row
    from helpers import make_batch, product_cfg

    torch = _torch()
    N, B = 4, 3
    cfg = product_cfg("classical", N)
    b = make_batch("classical", B, N, seed=5, surface=1)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    t = _inputs(b)
    t.update(_fresh_outputs(B, N, cfg.nx))
    good = _dev(np.tile(cost_weight_row(cfg), (B, 1)))
    for bad in (good[:, :24].contiguous(), good[: B - 1], good.to(torch.float32), good.cpu(), good.t().contiguous().t(),
                np.tile(cost_weight_row(cfg), (B, 1))):
        with pytest.raises(ValueError, match="cost_weights"):
            solver.solve_dev(t, maxiter=MAXITER, cost_weights=bad)
    with pytest.raises(ValueError, match="cost_weights"):
        solver.calc_diff(b, b.xs_init, b.us_init, cost_weights=np.zeros((B, 24)))
    p = lambda k: t[k].data_ptr()  # noqa: E731
    args = (p("x0"), p("node_ref"), p("inst_ref"), p("surface"), p("xs_init"), p("us_init"), MAXITER, 0, p("xs"),
            p("us"), p("K"), p("cost"), p("iters"), p("ok"), p("fn_pred"), p("stats"))
    lib, h, w = solver._lib, solver._h, good.data_ptr()
    assert lib.ffddp_solve_batch_wts_dev(None, B, *args, None, None, w, None) == -1
    assert lib.ffddp_solve_batch_wts_dev(h, -1, *args, None, None, w, None) == -1
    assert lib.ffddp_solve_batch_wts_dev(h, B + 1, *args, None, None, w, None) == -4
    assert lib.ffddp_solve_batch_wts_dev(h, 0, *args, None, None, w, None) == 0
    assert lib.ffddp_calc_diff_wts(None, B, *([None] * 18)) == -1
    torch.cuda.synchronize()
    assert np.all(_host(t)["xs"] == SENTINEL) and np.all(_host(t)["iters"] == ISENT)  # nothing ran
    solver.close()
    with pytest.raises(ValueError, match="unknown cost weight"):
        cost_weight_row(cfg, w_nope=1.0)
    with pytest.raises(ValueError, match="does not build"):
        cost_weight_row(cfg, w_friction_cone=5.0)  # normal_1d
    with pytest.raises(ValueError, match="does not build"):
        cost_weight_row(cfg, w_y=1.0)  # classical
    assert cost_weight_row(cfg, w_y=0.0)[_abi.COST_INDEX["w_y"]] == 0.0


# -- 8. the device loop ----------------------------------------------------------------------
LB, LN, LTICKS = 5, 8, 8


def _ctrl_cfg(variant):
    import test_gpu_fleet_tasks as TG
    from ffddp import controller as CT
    from ffddp.trajectory import benchmark_task

    ee, cal, dt = TG._scene()
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    return make(dt, benchmark_task(ee).z_contact, horizon=LN, phase_source="trajectory"), ee, cal, dt


def _loop(variant, period, steps=LTICKS, t0=0.78, tilt=(0.0, 5.0, 10.0, -5.0, 0.0), **kw):
    """test_gpu_force_ref._loop with the run's length, start and tilts as arguments.  Instance 4 is instance 0 in
    everything but what **kw gives it."""
    from ffddp import robot as R
    from ffddp.fleet_loop import DeviceFleetLoop
    from ffddp.trajectory import benchmark_task

    cfg, ee, cal, dt = _ctrl_cfg(variant)
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (LB, 7))
    q0[4] = q0[0]
    radius, omega = np.array([0.10, 0.07, 0.12, 0.09, 0.10]), np.array([1.5, 1.1, 1.9, 1.3, 1.5])
    tasks = [benchmark_task(ee, radius=r, omega=w, delay=d * dt) for r, w, d in zip(radius, omega, FR.L_DELAY_TICKS)]
    return DeviceFleetLoop(variant, LB, None, cfg, q0, tilt_deg=np.asarray(tilt, float), steps=steps, calibration=cal,
                           t0=t0, tasks=tasks, solve_period=period, **kw)


def _loop_overrides(cfg, variant):
    s = lambda n, x: {n: float(getattr(cfg, n)) * x}  # noqa: E731
    ff = s("w_y", 2.0) if variant == "ff" else {}
    return [None, {**s("w_fn", 2.0), **s("w_tangent_pos", 0.5), **s("w_ee_pos", 2.0)},
            {**s("w_tau", 4.0), **s("w_posture", 0.25), **ff}, {**s("w_tangent_vel", 2.0), **s("w_plane_z", 0.5), **s("w_ee_ori", 0.5)},
            {**s("w_fn", 0.25), **s("w_ee_pos", 0.5), **s("w_v", 2.0)}]


def _hand_tick(loop, cw_d):
    """DeviceFleetLoop's tick through the entry points themselves, the rows passed by hand."""
    from ffddp.fleet_loop import LPF_ALPHA

    k, T, s = loop.k, loop.T, loop.solver
    if not loop._stepped:
        loop._plant_step()
    r = loop._row(k)
    T["info"], T["log_obs"] = loop.log_info[r], loop.log_obs[r]
    loop.ktasks.t = loop._tick_time(k)
    kw, sel = {}, {}
    if loop.sched is not None:
        T["need"] = loop.log_need[r]
        kw, sel = dict(sched=loop.sched), dict(active=T["need"])
    s.fleet_pre_dev(T, loop.params, False, stream=loop._stream, tasks=loop.ktasks, **kw)
    s.solve_dev(T, maxiter=int(loop.cfg.max_iters), is_feasible=False, stream=loop._stream, cost_weights=cw_d, **sel)
    s.fleet_post_dev(T, loop.params, lpf=LPF_ALPHA, stream=loop._stream, **kw)
    loop._stepped = False
    loop.k = k + 1


@pytest.mark.parametrize("variant,period", FR.LOOP_CASES)
def test_loop_rows_of_the_configuration_equal_the_plain_loop(variant, period):
    from ffddp.config import cost_weight_row

    plain = _loop(variant, period, metrics=True)
    row = cost_weight_row(plain.solver.cfg)
    arr = _loop(variant, period, metrics=True, cost_weights=np.tile(row, (LB, 1)))
    lst = _loop(variant, period, metrics=True, cost_weights=[None, {}, None, {"w_fn": float(plain.cfg.w_fn)}, None])
    assert plain.cw is None and arr.cw is not None and np.array_equal(arr.cost_rows, lst.cost_rows)
    for loop in (plain, arr, lst):
        loop.run(LTICKS)
    rp, ra, rl = plain.results(), arr.results(), lst.results()
    print("ticks with surface = 1 per instance", (rp["surface"] != 0).sum(0))
    FR._same_results(ra, rp, (variant, period, "array"), skip=("cost_rows",))
    FR._same_results(rl, rp, (variant, period, "list"), skip=("cost_rows",))
    assert np.array_equal(ra["metrics"], rp["metrics"], equal_nan=True)
    assert np.array_equal(rl["metrics"], rp["metrics"], equal_nan=True)
    assert set(arr.state()) == set(plain.state())
    for loop in (plain, arr, lst):
        loop.close()


@pytest.mark.parametrize("variant,period", FR.LOOP_CASES)
def test_loop_distinct_rows_equal_the_hand_stepped_loop(variant, period):
    from ffddp.fleet_loop import cost_weight_rows

    o = _loop(variant, period)
    over = _loop_overrides(o.solver.cfg, variant)
    a = _loop(variant, period, cost_weights=over)
    rows = cost_weight_rows(o.solver.cfg, variant, over, LB)
    assert np.array_equal(a.cost_rows, rows) and len({tuple(r) for r in rows}) == LB
    cw_d = _dev(rows)
    a.run(LTICKS)
    for _ in range(LTICKS):
        _hand_tick(o, cw_d)
    ra, ro = a.results(), o.results()
    FR._same_results(ra, ro, (variant, period), skip=("cost_rows",))
    # instances 0 and 4 share the task, the start and the plant: their rows tell them apart; and the loop differs
    # from the plain one
    assert not np.array_equal(ra["info"][:, 0], ra["info"][:, 4], equal_nan=True)
    plain = _loop(variant, period)
    plain.run(LTICKS)
    rp = plain.results()
    assert not np.array_equal(rp["info"], ra["info"], equal_nan=True)
    assert np.array_equal(rp["info"][:, 0], ra["info"][:, 0], equal_nan=True)  # None: the configuration's weights
    for loop in (a, o, plain):
        loop.close()


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_distinct_rows_forty_ticks_flat(variant):
    ticks = 40
    over = _loop_overrides(_ctrl_cfg(variant)[0], variant)
    loop = _loop(variant, None, steps=ticks, t0=0.7, tilt=(0.0,) * LB, metrics=True, cost_weights=over)
    loop.run(ticks)
    r = loop.results()
    print("ticks with surface = 1 per instance", (r["surface"] != 0).sum(0))
    assert not np.any(r["plant_fail"])
    for k, v in r["summary"].items():
        assert np.all(np.isfinite(np.asarray(v, float))), (k, v)
    loop.close()
