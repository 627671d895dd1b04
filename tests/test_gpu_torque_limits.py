"""GPU: per-instance torque limits (tau_lim / torque_limits) of the device
solve, of calc_diff, of the fleet post kernel and of the device fleet loop.

Three references, none of them stored numbers:
- the same library without the argument (rows of the configuration's limits
  must give its bits);
- a second handle created with one instance's tau_limits in its configuration,
  solving that instance alone: the kernels without the feature, the limits
  constants;
- the numpy oracle (oracle.fddp.SolverBoxFDDP) over oracle_cfg of that same
  per-instance configuration, at tests/test_gpu_parity.py's tolerances.

Solves run at test_gpu_cost_weights.py's shapes (N = 12, B = 6, maxiter 10, its
SOLVE_CASES): nodes of two instances share a k_node wave and a k_forward_g8
wave, the row layout and the wide first pass run; the mask test at B = 300
covers the four slices and the two-groups-per-row layout.  Oracle solves run in
spawned workers that import test_gpu_cost_weights, so nothing at module level
touches the device or imports the product."""
from __future__ import annotations

import copy
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import ocp

import test_gpu_cost_weights as CW
import test_gpu_force_ref as FR
from test_gpu_force_ref import MAXITER, OUT, SENTINEL, SOLVE_CASES, _dev, _fresh_outputs, _host, _inputs, _solve_dev, _torch

pytestmark = pytest.mark.gpu

N_SOLVE, B_SOLVE = CW.N_SOLVE, CW.B_SOLVE
STAT_COLS = CW.STAT_COLS
# instance 0 keeps the configuration's limits; the others a uniform scale each from {1/16, 1/8, 1/4, 1/2}, the last
# one factor per joint from that set (a joint-index mix-up would show there).  Which instance takes which scale
# follows the kernels without the feature: on this batch (seed 42) a handle of the classical point3d + cone case
# whose configuration carries the limits misses test_gpu_parity's tight table on instance 2 at every scale but
# 1/16 (xs 1.13e-8 against 1e-8 at scales 1, 1/2 and 1/4 alike, 4.3e-6 at 1/8) and, against the explicit-inverse
# oracle, on instance 3 at 1, 1/2 and 1/4 (K element-wise 1.8e-4 against 3e-5): the instance's conditioning, whatever
# the limit.  So instance 2 takes 1/16 and instance 3 takes 1/8, where those handles are inside the table; no factor
# of the set is left out and no tolerance is widened.
SCALES = np.array([[1.0] * 7, [0.25] * 7, [0.0625] * 7, [0.125] * 7, [0.5] * 7,
                   [0.5, 0.25, 0.125, 0.0625, 0.5, 0.25, 0.125]])


def _cfg_of(cfg, f):
    """cfg with tau_limits scaled per joint: the configuration a per-instance handle, and the oracle, take."""
    c = copy.deepcopy(cfg)
    c.tau_limits = np.asarray(cfg.tau_limits, float) * np.asarray(f, float)
    return c


def _rows(cfg, f):
    from ffddp.config import torque_limit_rows

    return torque_limit_rows(cfg, np.asarray(cfg.tau_limits, float)[None] * np.asarray(f, float))


# -- 1. rows of the configuration's limits ---------------------------------------------------
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
    assert hasattr(solver._lib, "ffddp_solve_batch_lim_dev")
    ul = _dev(_rows(cfg, np.ones((B, 7))))
    assert tuple(ul.shape) == (B, _abi.TAU_LIM_W)
    w = _dev(np.tile(cost_weight_row(cfg), (B, 1)))
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    full = torch.full((B, N + 1), float(cfg.fn_des), dtype=torch.float64, device="cuda")
    plain = _solve_dev(solver, b)
    runs = {"rows": _solve_dev(solver, b, torque_limits=ul),
            "rows+mask": _solve_dev(solver, b, torque_limits=ul, active=ones),
            "rows+fref": _solve_dev(solver, b, torque_limits=ul, force_ref=full),
            "rows+cw": _solve_dev(solver, b, torque_limits=ul, cost_weights=w),
            "rows+mask+fref+cw": _solve_dev(solver, b, torque_limits=ul, active=ones, force_ref=full, cost_weights=w)}
    assert np.all(plain["iters"] > 0) and np.all(plain["xs"] != SENTINEL)
    for tag, r in runs.items():
        for k in OUT:
            assert np.array_equal(r[k], plain[k], equal_nan=True), (tag, k)
    solver.close()


# -- 2. / 3. distinct rows -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distinct(variant, contact, cone):
    """The case's batch solved once with distinct rows, and every instance solved alone by a handle of its own whose
    configuration carries that instance's tau_limits (the kernels without the feature).  Shared by tests 2 and 3."""
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=42, surface=1)
    f = SCALES
    rows = _rows(cfg, f)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    got = _solve_dev(solver, b, torque_limits=_dev(rows))
    plain = _solve_dev(solver, b)
    solver.close()
    cfgs = [_cfg_of(cfg, f[i]) for i in range(B)]
    alone, unit = [], []
    one = BatchedBoxFDDP(cfg, max_batch=1)
    for i in range(B):
        s = BatchedBoxFDDP(cfgs[i], max_batch=1)
        alone.append(_solve_dev(s, CW._sub(b, [i])))
        s.close()
        unit.append(_solve_dev(one, CW._sub(b, [i])))  # the scale-1 handle on the same instance
    one.close()
    return SimpleNamespace(cfg=cfg, cfgs=cfgs, batch=b, f=f, rows=rows, got=got, plain=plain, alone=alone, unit=unit)


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_equal_per_configuration_handles(variant, contact, cone):
    d = _distinct(variant, contact, cone)
    got = d.got
    assert np.all(d.f[0] == 1.0) and len({tuple(r) for r in d.f}) == B_SOLVE
    lim = np.asarray(d.cfg.tau_limits, float)[None] * d.f
    for i, a in enumerate(d.alone):
        assert got["iters"][i] == a["iters"][0] and got["ok"][i] == a["ok"][0], i
        assert np.array_equal(got["stats"][i][STAT_COLS], a["stats"][0][STAT_COLS]), i
        for k in ("xs", "us", "K", "cost", "fn_pred"):
            assert np.array_equal(got[k][i], a[k][0], equal_nan=True), (i, k)
    # the test must not pass on unclamped solves: at least two instances with an active clamp
    at_limit = [bool(np.any(np.abs(got["us"][i]) == lim[i][None, :])) for i in range(B_SOLVE)]
    differs = [any(not np.array_equal(d.alone[i][k], d.unit[i][k], equal_nan=True) for k in ("xs", "us", "K", "cost"))
               for i in range(B_SOLVE)]
    print("instances with |us| at its limit", at_limit, "| differing from the scale-1 handle", differs)
    assert sum(1 for i in range(B_SOLVE) if at_limit[i] or differs[i]) >= 2
    assert np.all(np.isfinite(got["cost"]))
    # instance 0 (scale 1) is the plain solve's
    assert all(np.array_equal(got[k][0], d.plain[k][0], equal_nan=True) for k in ("xs", "us", "K", "cost", "iters"))


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_match_oracle(variant, contact, cone):
    """test_gpu_parity.test_solve_matches_oracle's checks and tolerance table, one oracle solve per instance under
    that instance's configuration.  The per-configuration handles (the kernels without the feature) are held to the
    same table first, so an excess of the batch would be the feature's."""
    import test_gpu_parity as TP

    d = _distinct(variant, contact, cone)
    key = (variant, contact, 1, cone)
    name = f"lim/{variant}/{contact}/cone{cone}"
    handles = {k: np.stack([a[k][0] for a in d.alone]) for k in OUT}
    if key in TP.CROCODDYL_FORM_TOL:
        ref = CW._oracle_solves(d.cfgs, d.batch, [TP.SOLVE_FORM, None])
        tight, tight_k = TP.CASE_TOL.get(key, (TP.TOL_SOLVE, TP.TOL_K))
        tight_ke = TP.CASE_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        tol, tol_k = TP.CROCODDYL_FORM_TOL[key]
        tol_ke = TP.CROCODDYL_FORM_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        for tag, o in (("handles", handles), ("rows", d.got)):
            s = FR._as_solver(o)
            TP._check_solves(f"{name}/{tag}/solve_form", d.cfg, d.batch, s, ref[0], tight, tight_k, tight_ke)
            TP._check_solves(f"{name}/{tag}/crocoddyl_form", d.cfg, d.batch, s, ref[1], tol, tol_k, tol_ke)
        return
    ref = CW._oracle_solves(d.cfgs, d.batch, [None])[0]
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
    f = np.array([[1.0] * 7, [0.0625] * 7, list(SCALES[5])])
    rows = _rows(cfg, f)
    rng = np.random.default_rng(7)
    xs = b.xs_init + 0.02 * rng.normal(size=b.xs_init.shape)
    us = b.us_init + 0.5 * rng.normal(size=b.us_init.shape)
    if variant == "ff":  # the barrier acts on the torque state, the w soft limit on the control
        xs[:, :, 14:] += 2.0 * rng.normal(size=xs[:, :, 14:].shape)
    # the barrier terms are live: the torque (and for force feedback the control w) exceeds the scaled soft bound
    tau = xs[:, :N, 14:] if variant == "ff" else us
    ts_ub, ws_lim = rows[:, 1:28:4], rows[:, 2:28:4]
    assert cfg.w_tau_soft_limits > 0.0 and np.any(np.abs(tau[1:]) > ts_ub[1:, None, :])
    if variant == "ff":
        assert cfg.w_w_soft_limits > 0.0 and np.any(np.abs(us[1:]) > ws_lim[1:, None, :])
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    out = solver.calc_diff(b, xs, us, torque_limits=rows)
    worst = {}
    for i in range(B):
        ocfg = oracle_cfg(_cfg_of(cfg, f[i]))
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
    # rows of the configuration are the call without, alone and with the other per-instance arguments
    from ffddp.config import cost_weight_row

    plain = solver.calc_diff(b, xs, us)
    same = solver.calc_diff(b, xs, us, torque_limits=_rows(cfg, np.ones((B, 7))))
    both = solver.calc_diff(b, xs, us, torque_limits=_rows(cfg, np.ones((B, 7))),
                            cost_weights=np.tile(cost_weight_row(cfg), (B, 1)),
                            force_ref=np.full((B, N + 1), float(cfg.fn_des)))
    for k in out:
        assert np.array_equal(same[k], plain[k], equal_nan=True) and np.array_equal(both[k], plain[k], equal_nan=True), k
        assert np.array_equal(out[k][0], plain[k][0], equal_nan=True), k
    assert np.all(out["cost"][1:, :N].sum(1) != plain["cost"][1:, :N].sum(1))
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
    f = np.random.default_rng(35).choice([1.0, 0.5, 0.25, 0.125], size=(B, 7))
    rows = _rows(cfg, f)
    mask = np.zeros(B, np.uint8)
    mask[::3] = 1
    on = mask != 0
    small = BatchedBoxFDDP(cfg, max_batch=int(on.sum()))
    alone = _solve_dev(small, CW._sub(b, on), torque_limits=_dev(rows[on]))
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
    solver.solve_dev(t, maxiter=MAXITER, active=_dev(mask), torque_limits=_dev(rp))
    got = _host(t)
    for k in OUT:
        a, r = (got[k][on], alone[k]) if k != "stats" else (got[k][on][:, STAT_COLS], alone[k][:, STAT_COLS])
        assert np.array_equal(a, r, equal_nan=True), k
        assert np.array_equal(got[k][~on], sent[k][~on], equal_nan=True), k
    assert np.all(np.isfinite(got["xs"][on])) and len(np.unique(got["iters"][on])) > 1
    plain = _solve_dev(solver, b)
    assert np.any(plain["xs"][on] != got["xs"][on])
    solver.close()


# -- 6. entries of terms the handle does not build -------------------------------------------
@pytest.mark.parametrize("variant,column,change", [("classical", 2, None), ("classical", 1, "w_tau_soft_limits"),
                                                   ("ff", 1, "w_tau_soft_limits"), ("classical", 0, "use_box_fddp"),
                                                   ("ff", 0, "use_box_fddp")])
def test_entries_of_absent_terms_are_not_used(variant, column, change):
    """NaN in the ws_lim column of a classical handle, in the ts_ub column with w_tau_soft_limits = 0 and in the u_ub
    column with use_box = 0 changes no bit."""
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, product_cfg

    N, B = N_SOLVE, B_SOLVE
    cfg = product_cfg(variant, N)
    if change == "w_tau_soft_limits":
        cfg.w_tau_soft_limits = 0.0
    elif change == "use_box_fddp":
        cfg.use_box_fddp = False
    b = make_batch(variant, B, N, seed=45, surface=1)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    rows = _rows(cfg, np.ones((B, 7)))
    rows[:, column:28:4] = np.nan
    plain = _solve_dev(solver, b)
    got = _solve_dev(solver, b, torque_limits=_dev(rows))
    assert np.all(np.isfinite(plain["xs"]))
    for k in OUT:
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    d = solver.calc_diff(b, b.xs_init, b.us_init)
    dw = solver.calc_diff(b, b.xs_init, b.us_init, torque_limits=rows)
    for k in d:
        assert np.array_equal(dw[k], d[k], equal_nan=True), k
    solver.close()


# -- 7. the post kernel, called directly -----------------------------------------------------
def _post_args(solver, t, params, lpf, sched):
    p = lambda k: C.c_void_p(int(t[k].data_ptr()) if t.get(k) is not None else 0)  # noqa: E731
    st = solver._fleet_state(t)
    obs = t.get("obs")
    args = (solver._h, int(t["x0"].shape[0]), C.byref(params), C.byref(st), p("xs"), p("us"), p("K"), p("cost"),
            p("iters"), p("ok"), p("fn_pred"), p("stats"), p("x0"), p("surface"), p("tau_bias"),
            int(t["tau_bias"].stride(0)), p("tau_cmd"), p("info"), p("scale"), p("tau_app"), p("tau_filt"), float(lpf),
            p("obs"), int(obs.stride(0)) if obs is not None else 0, p("log_obs"))
    sp = C.byref(solver._fleet_sched(t, sched)) if sched is not None else None
    return args, sp, (st, params)


@pytest.mark.parametrize("apply_filter", [False, True])
@pytest.mark.parametrize("variant,N,B", [("classical", 5, 16), ("ff", 4, 67)])
def test_post_clips_to_each_instances_own_limit(variant, N, B, apply_filter):
    import test_gpu_fleet_loop_kernels as KT
    import test_gpu_fleet_sched_kernels as SK
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset, ff_preset, torque_limit_rows

    torch = _torch()
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    assert hasattr(solver._lib, "ffddp_fleet_post_lim_dev")
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N * 100 + B + 3)
    # no feedback, no fallback: the raw command is the first-knot policy, far beyond every limit
    P = KT._params(use_feedback_policy=0, max_tau_raw_inf=1.0e12, ff_inverse_actuation_model=0)
    sign = rng.choice([-1.0, 1.0], size=(B, 7))
    d = KT._solve_outputs(rng, B, N, nx)
    st = KT._state(rng, B, N, nx)
    st["valid"][:] = 1
    d["K"][:] = 0.0
    d["us"][:] = 1.0e3 * sign[:, None, :]
    if variant == "ff":
        d["xs"][:, :, 14:] = 1.0e3 * sign[:, None, :]
    st["tau_prev"][:] = 1.0e3 * sign  # the filter steps from a previous command that is beyond the limits too
    lim = np.asarray(cfg.tau_limits, float)[None] * rng.choice([1.0, 0.5, 0.25, 0.125, 0.0625], size=(B, 7))
    rows = torque_limit_rows(cfg, lim)
    o, od, rec = KT._observations(rng, B, strided=B > 16)
    x0 = rng.normal(size=(B, nx))
    if variant == "ff":
        x0[:, 14:] = 1.0e3 * sign
    surface = (rng.random(B) < 0.6).astype(np.uint8)
    sched = SK._sched(1, apply_filter) if apply_filter else None

    def run(mode):
        t = KT._up(st)
        t.update(KT._up(d))
        t.update(KT._up(dict(x0=x0, surface=surface, since=np.zeros(B, np.int32), age=np.zeros(B, np.int32),
                             need=np.ones(B, np.uint8), scale=np.full((B, 7), 0.9), tau_filt=np.zeros((B, 7)))))
        t.update(tau_bias=od["tau_bias"], obs=od["obs"], tau_cmd=SK._full(B, 7), info=SK._full(B, _abi.FLEET_INFO_W),
                 tau_app=SK._full(B, 7), log_obs=SK._full(B, _abi.FLEET_LOG_W))
        if mode == "rows":
            solver.fleet_post_dev(t, P, lpf=0.2, stream=stream, sched=sched, torque_limits=_dev(rows))
        elif mode == "null":
            args, sp, keep = _post_args(solver, t, P, 0.2, sched)
            rc = solver._lib.ffddp_fleet_post_lim_dev(*args, sp, None, C.c_void_p(stream))
            assert rc == 0, solver._lib.ffddp_last_error(solver._h)
        else:
            solver.fleet_post_dev(t, P, lpf=0.2, stream=stream, sched=sched)
        return KT._down(t, KT.STATE_KEYS + ("tau_cmd", "info", "tau_app", "tau_filt", "log_obs", "since", "age"))

    got, null, plain = run("rows"), run("null"), run("plain")
    info = {k: got["info"][:, i] for i, k in enumerate(_abi.FLEET_INFO_FIELDS)}
    assert not info["unstable"].any() and np.all(info["tau_raw_inf"] > lim.max())
    assert np.array_equal(got["tau_cmd"], sign * lim)  # +-the row's limit per instance and joint, exactly
    assert np.array_equal(got["tau_prev"], sign * lim) and np.array_equal(info["tau_cmd_inf"], lim.max(1))
    assert np.array_equal(got["tau_app"], 0.9 * (sign * lim))
    # NULL rows: the existing entry points' bits, which clip to the handle-wide limit
    for k in plain:
        assert np.array_equal(null[k], plain[k], equal_nan=True), k
    assert np.array_equal(plain["tau_cmd"], sign * 0.8)
    for k in ("keep_xs", "keep_us", "keep_K", "valid", "since", "age", "log_obs"):
        assert np.array_equal(got[k], plain[k], equal_nan=True), k
    solver.close()


def test_post_lim_error_codes():
    from ffddp import BatchedBoxFDDP
    from ffddp.config import classical_preset

    solver = BatchedBoxFDDP(classical_preset(4), max_batch=2, device=0)
    lib, h = solver._lib, solver._h
    none = [None] * 2 + [None] * 10 + [None, 7, None, None, None, None, None, 0.0, None, 0, None]
    assert lib.ffddp_fleet_post_lim_dev(None, 2, *none, None, None, None) == -1
    assert lib.ffddp_fleet_post_lim_dev(h, 0, *none, None, None, None) == -1
    assert b"ffddp_fleet_post_lim_dev" in lib.ffddp_last_error(h)
    assert lib.ffddp_fleet_post_lim_dev(h, 3, *none, None, None, None) == -4
    assert lib.ffddp_fleet_post_lim_dev(h, 2, *none, None, None, None) == -1
    assert b"ffddp_fleet_post_lim_dev: null pointer" in lib.ffddp_last_error(h)
    solver.close()


# -- 8. the device loop ----------------------------------------------------------------------
LB, LTICKS = CW.LB, CW.LTICKS
LOOP_SCALES = np.array([[1.0] * 7, [0.25] * 7, [0.5] * 7, [0.5, 0.25, 0.125, 0.5, 0.25, 0.125, 0.5], [0.125] * 7])


def _hand_tick(loop, ul_d):
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
    s.solve_dev(T, maxiter=int(loop.cfg.max_iters), is_feasible=False, stream=loop._stream, torque_limits=ul_d, **sel)
    s.fleet_post_dev(T, loop.params, lpf=LPF_ALPHA, stream=loop._stream, torque_limits=ul_d, **kw)
    loop._stepped = False
    loop.k = k + 1


@pytest.mark.parametrize("variant,period", FR.LOOP_CASES)
def test_loop_rows_of_the_configuration_equal_the_plain_loop(variant, period):
    plain = CW._loop(variant, period, metrics=True)
    base = np.asarray(plain.cfg.tau_limits, float)
    arr = CW._loop(variant, period, metrics=True, torque_limits=np.tile(base, (LB, 1)))
    lst = CW._loop(variant, period, metrics=True, torque_limits=[1.0] * LB)
    assert plain.ul is None and arr.ul is not None and np.array_equal(arr.limit_rows, lst.limit_rows)
    assert np.array_equal(arr.tau_limits, np.tile(base, (LB, 1)))
    for loop in (plain, arr, lst):
        loop.run(LTICKS)
    rp, ra, rl = plain.results(), arr.results(), lst.results()
    print("ticks with surface = 1 per instance", (rp["surface"] != 0).sum(0))
    FR._same_results(ra, rp, (variant, period, "array"))
    FR._same_results(rl, rp, (variant, period, "scales"))
    assert np.array_equal(ra["metrics"], rp["metrics"], equal_nan=True)
    assert np.array_equal(rl["metrics"], rp["metrics"], equal_nan=True)
    sa, sp = arr.state(), plain.state()
    assert set(sa) == set(sp)
    for loop in (plain, arr, lst):
        loop.close()


@pytest.mark.parametrize("variant,period", FR.LOOP_CASES)
def test_loop_distinct_rows_equal_the_hand_stepped_loop(variant, period):
    from ffddp.config import torque_limit_rows

    o = CW._loop(variant, period)
    lim = np.asarray(o.cfg.tau_limits, float)[None] * LOOP_SCALES
    a = CW._loop(variant, period, torque_limits=lim)
    rows = torque_limit_rows(o.solver.cfg, lim)
    assert np.array_equal(a.limit_rows, rows) and len({tuple(r) for r in rows}) == LB
    ul_d = _dev(rows)
    a.run(LTICKS)
    for _ in range(LTICKS):
        _hand_tick(o, ul_d)
    ra, ro = a.results(), o.results()
    FR._same_results(ra, ro, (variant, period))
    assert np.all(ra["tau_cmd_inf"] <= lim.max(1)[None, :])
    # instances 0 and 4 share the task, the start and the plant: their limits tell them apart; and the loop differs
    # from the plain one, whose instance 0 (scale 1) it keeps
    assert not np.array_equal(ra["info"][:, 0], ra["info"][:, 4], equal_nan=True)
    plain = CW._loop(variant, period)
    plain.run(LTICKS)
    rp = plain.results()
    assert not np.array_equal(rp["info"], ra["info"], equal_nan=True)
    assert np.array_equal(rp["info"][:, 0], ra["info"][:, 0], equal_nan=True)
    for loop in (a, o, plain):
        loop.close()


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_distinct_rows_forty_ticks_flat(variant):
    ticks = 40
    base = np.asarray(CW._ctrl_cfg(variant)[0].tau_limits, float)
    lim = base[None] * LOOP_SCALES
    loop = CW._loop(variant, None, steps=ticks, t0=0.7, tilt=(0.0,) * LB, metrics=True, torque_limits=lim)
    loop.run(ticks)
    r = loop.results()
    print("ticks with surface = 1 per instance", (r["surface"] != 0).sum(0), "| max tau_cmd_inf", r["tau_cmd_inf"].max(0))
    assert not np.any(r["plant_fail"])
    for k, v in r["summary"].items():
        assert np.all(np.isfinite(np.asarray(v, float))), (k, v)
    assert np.all(r["tau_cmd_inf"] <= lim.max(1)[None, :])
    loop.close()
