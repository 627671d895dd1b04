"""GPU: the C entry points behind the Python wrappers, called directly.

include/ffddp.h documents every narrow call as the general one with NULL
for what it lacks: same kernels, same bits.  The Python wrappers call the
general entry points only, so the narrow ones are pinned here:

1. ffddp_solve_batch_dev, _sel_dev(active = NULL), _fref_dev(NULL, NULL) and
   _wts_dev(NULL, NULL, NULL) write the same bits, and those of solve_dev;
2. ffddp_calc_diff, _fref(NULL) and _wts(NULL, NULL) likewise;
3. every fleet pre / post / inject entry point names itself in its error
   text, and the solve's argument check keeps its order and texts.

The expected strings are the library's (ffddp_last_error), written out here.
No call of part 3 launches a kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ffddp import BatchedBoxFDDP, _abi  # noqa: E402

from helpers import make_batch, product_cfg  # noqa: E402

N = 3
MAXITER = 2
OUT = ("xs", "us", "K", "cost", "iters", "ok", "fn_pred", "stats")


def _inputs(batch):
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k))).cuda()
         for k in ("x0", "node_ref", "inst_ref", "xs_init", "us_init")}
    t["surface"] = torch.from_numpy(np.ascontiguousarray(batch.surface, dtype=np.uint8)).cuda()
    return t


def _fresh_outputs(B, nx):
    """Float outputs NaN, integer outputs a value no solve writes."""
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    return dict(xs=f(B, N + 1, nx), us=f(B, N, 7), K=f(B, N, 7, nx), cost=f(B),
                iters=torch.full((B,), -77, dtype=torch.int32, device="cuda"),
                ok=torch.full((B,), 77, dtype=torch.uint8, device="cuda"), fn_pred=f(B, 2),
                stats=torch.full((B, _abi.NSTATS), -77, dtype=torch.int32, device="cuda"))


def _solve_args(t, B, maxiter=MAXITER):
    p = lambda k: t[k].data_ptr()  # noqa: E731
    return (B, p("x0"), p("node_ref"), p("inst_ref"), p("surface"), p("xs_init"), p("us_init"), maxiter, 0, p("xs"),
            p("us"), p("K"), p("cost"), p("iters"), p("ok"), p("fn_pred"), p("stats"))


def _host(t):
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in OUT}


def _same_bits(a, b):
    """array_equal on the bytes: a free-space instance's fn_pred is NaN, which no value comparison equals."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# -- 1. the solve's narrow entry points ------------------------------------------------------
@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_solve_entry_points_write_the_same_bits(variant):
    B = 3
    cfg = product_cfg(variant, N)
    batch = make_batch(variant, B, N, seed=21, surface=np.array([1, 0, 1]))
    assert batch.surface.tolist() == [1, 0, 1]  # contact and free space
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    lib = solver._lib
    calls = {
        "ffddp_solve_batch_dev": lambda a: lib.ffddp_solve_batch_dev(solver._h, *a, None),
        "ffddp_solve_batch_sel_dev": lambda a: lib.ffddp_solve_batch_sel_dev(solver._h, *a, None, None),
        "ffddp_solve_batch_fref_dev": lambda a: lib.ffddp_solve_batch_fref_dev(solver._h, *a, None, None, None),
        "ffddp_solve_batch_wts_dev": lambda a: lib.ffddp_solve_batch_wts_dev(solver._h, *a, None, None, None, None),
    }
    t = _inputs(batch)
    t.update(_fresh_outputs(B, cfg.nx))
    solver.solve_dev(t, maxiter=MAXITER)
    ref = _host(t)
    assert np.all(np.isfinite(ref["xs"])) and np.all(ref["iters"] >= 0) and np.all(ref["ok"] <= 1)
    for name, call in calls.items():
        t = _inputs(batch)
        t.update(_fresh_outputs(B, cfg.nx))
        assert call(_solve_args(t, B)) == 0, (name, lib.ffddp_last_error(solver._h))
        got = _host(t)
        for k in OUT:
            assert _same_bits(got[k], ref[k]), (name, k)
    solver.close()


# -- 2. calc_diff's narrow entry points ------------------------------------------------------
@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_calc_diff_entry_points_write_the_same_bits(variant):
    B = 2
    cfg = product_cfg(variant, N)
    nx = cfg.nx
    batch = make_batch(variant, B, N, seed=22, surface=np.array([1, 0]))
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    lib, d = solver._lib, _abi.dptr
    f = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))  # noqa: E731
    rng = np.random.default_rng(5)
    xs = f(batch.xs_init, (B, N + 1, nx)) + 0.01 * rng.standard_normal((B, N + 1, nx))
    us = f(batch.us_init, (B, N, 7)) + 0.1 * rng.standard_normal((B, N, 7))
    head = (solver._h, B, d(f(batch.x0, (B, nx))), d(f(batch.node_ref, (B, N + 1, 6))), d(f(batch.inst_ref, (B, 21))),
            _abi.uptr(np.ascontiguousarray(batch.surface, dtype=np.uint8)), d(xs), d(us))
    shapes = dict(Fx=(B, N, nx, nx), Fu=(B, N, nx, 7), Lx=(B, N + 1, nx), Lu=(B, N, 7), Lxx=(B, N + 1, nx, nx),
                  Lxu=(B, N, nx, 7), Luu=(B, N, 7, 7), cost=(B, N + 1), xnext=(B, N, nx), lam=(B, N + 1, 3))

    def run(fn, *extra):
        out = {k: np.full(s, np.nan) for k, s in shapes.items()}
        assert fn(*head, *extra, *(d(out[k]) for k in shapes)) == 0, lib.ffddp_last_error(solver._h)
        return out

    ref = solver.calc_diff(batch, xs, us)
    assert set(ref) == set(shapes) and all(np.all(np.isfinite(v)) for v in ref.values())
    for name, out in (("ffddp_calc_diff", run(lib.ffddp_calc_diff)),
                      ("ffddp_calc_diff_fref", run(lib.ffddp_calc_diff_fref, None)),
                      ("ffddp_calc_diff_wts", run(lib.ffddp_calc_diff_wts, None, None))):
        for k in shapes:
            assert _same_bits(out[k], ref[k]), (name, k)
    solver.close()


# -- 3. error texts --------------------------------------------------------------------------
def _err(solver):
    return solver._lib.ffddp_last_error(solver._h).decode()


def test_fleet_entry_points_name_themselves():
    """B = 0 and a null required pointer: -1 and the called function's own name; B above max_batch: -4."""
    solver = BatchedBoxFDDP(product_cfg("classical", N), max_batch=2, device=0)
    lib, h = solver._lib, solver._h
    keep = torch.ones(6, dtype=torch.float64, device="cuda")
    rows = _abi.FleetInjectRows()
    rows.sigma = keep.data_ptr()  # a row array: the rows entry points do not forward to the plain ones
    sched, tasks = _abi.FleetSched(), _abi.FleetTasks()
    pre = (None,) * 5 + (7, 1, None, 7, None)          # q .. ee_z, ld_qv, ld_scalar, tau_hat, ld_tau_hat, q_nom
    post = (None,) * 11 + (7,) + (None,) * 5 + (0.0, None, 0, None)
    obs = (None, None, None, 7, None, None, None, None)  # z, q, v, ld_qv, tau_filt, qv_ctrl, tau_hat, tau_ctrl
    # name -> (call(B) with every pointer null, the text after the name for B = 0)
    tick = " B must be positive"
    inj = " B must be positive and k >= 0"
    calls = {
        "ffddp_fleet_pre_dev": (lambda B: lib.ffddp_fleet_pre_dev(h, B, None, None, *pre, None, 0, *(None,) * 6, None), tick),
        "ffddp_fleet_pre_sched_dev": (
            lambda B: lib.ffddp_fleet_pre_sched_dev(h, B, None, None, *pre, None, 0, *(None,) * 6, sched, None), tick),
        "ffddp_fleet_pre_task_dev": (
            lambda B: lib.ffddp_fleet_pre_task_dev(h, B, None, None, *pre, tasks, *(None,) * 6, None, None), tick),
        "ffddp_fleet_post_dev": (lambda B: lib.ffddp_fleet_post_dev(h, B, None, None, *post, None), tick),
        "ffddp_fleet_post_sched_dev": (lambda B: lib.ffddp_fleet_post_sched_dev(h, B, None, None, *post, sched, None), tick),
        "ffddp_fleet_inject_obs_dev": (lambda B: lib.ffddp_fleet_inject_obs_dev(h, B, None, 0, *obs, None), inj),
        "ffddp_fleet_inject_cmd_dev": (lambda B: lib.ffddp_fleet_inject_cmd_dev(h, B, None, 0, None, None, None), inj),
        "ffddp_fleet_inject_obs_rows_dev": (
            lambda B: lib.ffddp_fleet_inject_obs_rows_dev(h, B, None, 0, *obs, C.byref(rows), None), inj),
        "ffddp_fleet_inject_cmd_rows_dev": (
            lambda B: lib.ffddp_fleet_inject_cmd_rows_dev(h, B, None, 0, None, None, C.byref(rows), None), inj),
    }
    for name, (call, text) in calls.items():
        assert call(0) == -1, name
        assert _err(solver) == name + ":" + text, name
        assert call(2) == -1, name  # params / the injector struct (and everything else) null
        assert _err(solver) == name + ": null pointer", name
        assert call(3) == -4, name
        assert _err(solver) == "B exceeds max_batch", name
    # without a row array the rows entry points are the plain ones, and say so
    assert lib.ffddp_fleet_inject_obs_rows_dev(h, 0, None, 0, *obs, None, None) == -1
    assert _err(solver) == "ffddp_fleet_inject_obs_dev:" + inj
    assert lib.ffddp_fleet_inject_cmd_rows_dev(h, 0, None, 0, None, None, C.byref(_abi.FleetInjectRows()), None) == -1
    assert _err(solver) == "ffddp_fleet_inject_cmd_dev:" + inj
    # a null handle, before anything else
    assert lib.ffddp_fleet_pre_dev(None, 0, None, None, *pre, None, 0, *(None,) * 6, None) == -1
    assert lib.ffddp_fleet_post_sched_dev(None, 0, None, None, *post, sched, None) == -1
    assert lib.ffddp_fleet_inject_cmd_rows_dev(None, 0, None, 0, None, None, C.byref(rows), None) == -1
    solver.close()


def test_solve_argument_check_order_and_texts():
    B = 2
    cfg = product_cfg("classical", N)
    batch = make_batch("classical", B, N, seed=23)
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    cfg0 = product_cfg("classical", N)
    cfg0.w_fn = 0.0
    s0 = BatchedBoxFDDP(cfg0, max_batch=B, device=0)
    lib = solver._lib
    t = _inputs(batch)
    t.update(_fresh_outputs(B, cfg.nx))
    fref = torch.full((B, N + 1), 22.0, dtype=torch.float64, device="cuda")
    a = _solve_args(t, B)
    wts = lambda s, args, fr=None: lib.ffddp_solve_batch_wts_dev(s._h, *args, None, fr, None, None)  # noqa: E731
    # a null handle before anything else
    assert lib.ffddp_solve_batch_wts_dev(None, -1, *a[1:], None, fref.data_ptr(), None, None) == -1
    # force_ref on a handle without the fn_track cost: rejected before the B checks
    w_fn = "force_ref given but the handle has no fn_track cost (w_fn <= 0)"
    for Bx in (-1, 0, B, B + 1):
        assert wts(s0, (Bx,) + a[1:], fref.data_ptr()) == -1
        assert _err(s0) == w_fn
    # then B and maxiter, the capacity, the empty batch, the pointers
    assert wts(solver, (-1,) + a[1:]) == -1 and _err(solver) == "negative B or maxiter"
    assert wts(solver, a[:7] + (-1,) + a[8:]) == -1 and _err(solver) == "negative B or maxiter"
    assert wts(solver, (B + 1,) + a[1:]) == -4 and _err(solver) == "B exceeds max_batch"
    nulls = (None,) * 6 + (MAXITER, 0) + (None,) * 8
    assert wts(solver, (0,) + nulls) == 0
    assert wts(solver, (B,) + nulls) == -1 and _err(solver) == "null pointer"
    assert wts(solver, a[:1] + (None,) + a[2:]) == -1 and _err(solver) == "null pointer"
    # the host entry point: the same check
    hz = (None,) * 6 + (MAXITER, 0) + (None,) * 8
    assert lib.ffddp_solve_batch(None, B, *hz) == -1
    assert lib.ffddp_solve_batch(solver._h, -1, *hz) == -1 and _err(solver) == "negative B or maxiter"
    assert lib.ffddp_solve_batch(solver._h, B + 1, *hz) == -4 and _err(solver) == "B exceeds max_batch"
    assert lib.ffddp_solve_batch(solver._h, 0, *hz) == 0
    assert lib.ffddp_solve_batch(solver._h, B, *hz) == -1 and _err(solver) == "null pointer"
    # the plan keeps its own stricter check
    ph, io = C.c_void_p(), _abi.PlanIO()
    assert lib.ffddp_plan_create(solver._h, 0, MAXITER, 0, C.byref(ph), C.byref(io)) == -1
    assert _err(solver) == "plan needs B >= 1 and maxiter >= 0"
    # nothing above left the outputs touched or the handle unusable
    assert wts(solver, a) == 0
    got = _host(t)
    assert np.all(np.isfinite(got["xs"])) and np.all(got["iters"] >= 0)
    s0.close()
    solver.close()
