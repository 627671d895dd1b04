"""GPU: the per-instance, per-node contact-force reference (force_ref) of the
device solve, its sampler and metrics kernels, and the device fleet loop.

The oracle is oracle.fddp.SolverBoxFDDP over ForceRefOCP below: oracle.ocp's
RobotOCP with node k evaluated under dataclasses.replace(cfg, fn_des=f[k]).
The oracle's calcDiff hands running() a slice and the point3d branch of
cost_stack takes a scalar fn_des, so a slice is evaluated node by node and
stacked.  Oracle solves run in spawned workers (as tests/oracle_pool.py); a
worker imports this module, so nothing at module level touches the device or
imports the product.

Tolerances are tests/test_gpu_parity.py's for the same case (TOL_NODE,
TOL_SOLVE, TOL_K, TOL_K_ELEM and its case tables for point3d with the cone);
everything else is np.array_equal."""
from __future__ import annotations

import dataclasses
from concurrent.futures import ProcessPoolExecutor
from multiprocessing import get_context
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import fddp, ocp

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
ISENT = -77
OUT = ("xs", "us", "K", "cost", "iters", "ok", "fn_pred", "stats")
MAXITER = 10


# -- the oracle ------------------------------------------------------------------------------
class ForceRefOCP(ocp.RobotOCP):
    """RobotOCP whose fn_track reference at node k is f[k] (f: N + 1 values)."""

    def __init__(self, cfg, prob, f):
        super().__init__(cfg, prob)
        self.f = np.asarray(f, float).reshape(cfg.horizon + 1)

    def _cfg(self, k):
        return dataclasses.replace(self.cfg, fn_des=float(self.f[k]))

    def running(self, idx, x, u, diff):
        if isinstance(idx, slice):
            ks = range(*idx.indices(self.N))
            outs = [ocp.running_eval(self._cfg(k), self.prob, k, x[j], u[j], diff) for j, k in enumerate(ks)]
            return {key: np.stack([np.asarray(o[key]) for o in outs]) for key in outs[0]}
        return ocp.running_eval(self._cfg(int(idx)), self.prob, idx, x, u, diff)

    def terminal(self, x, diff):
        return ocp.terminal_eval(self._cfg(self.N), self.prob, x, diff)


def _solve_one(args):
    ocfg, prob, f, xs_init, us_init, consts = args
    if np.ndim(f) == 0:  # a constant: the plain oracle with fn_des replaced
        s = fddp.SolverBoxFDDP(dataclasses.replace(ocfg, fn_des=float(f)), prob, box=True, consts=consts)
    else:
        s = fddp.SolverBoxFDDP(ForceRefOCP(ocfg, prob, f), box=True, consts=consts)
    ok = s.solve(xs_init, us_init, MAXITER, False)
    st = s.stats
    return dict(ok=bool(ok), iter=int(s.iter), xs=s.xs, us=s.us, K=s.K, cost=float(s.cost), iters_run=st.iters_run,
                trials=st.trials, reg_retries=st.reg_retries, forward_errors=st.forward_errors,
                neg_branch=st.neg_branch, neg_accepted=st.neg_accepted, clamped=st.clamped)


def _oracle_solves(cfg, batch, fs, consts_list):
    """One oracle solve per (consts, instance): fs[i] a scalar or (N+1,).  Returns {consts index: [dict per instance]}."""
    from helpers import oracle_cfg, oracle_problem
    from oracle_pool import _workers

    ocfg = oracle_cfg(cfg)
    jobs = [(ocfg, oracle_problem(batch, i, cfg.horizon), fs[i], np.array(batch.xs_init[i]), np.array(batch.us_init[i]), c)
            for c in consts_list for i in range(len(fs))]
    n = _workers(len(jobs))
    if n == 1:
        res = [_solve_one(j) for j in jobs]
    else:
        with ProcessPoolExecutor(max_workers=n, mp_context=get_context("spawn")) as ex:
            res = list(ex.map(_solve_one, jobs))
    return {c: res[c * len(fs):(c + 1) * len(fs)] for c in range(len(consts_list))}


# -- device helpers --------------------------------------------------------------------------
def _torch():
    return pytest.importorskip("torch")


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _cfg(variant, N, contact, cone=0):
    from helpers import product_cfg

    c = product_cfg(variant, N, contact)
    if cone:
        c.w_friction_cone, c.mu = 2.0e2, 0.6
    return c


def _inputs(batch):
    t = {k: _dev(getattr(batch, k)) for k in ("x0", "node_ref", "inst_ref", "xs_init", "us_init")}
    t["surface"] = _dev(np.ascontiguousarray(batch.surface, dtype=np.uint8))
    return t


def _fresh_outputs(B, N, nx):
    torch = _torch()
    f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float64, device="cuda")  # noqa: E731
    return dict(xs=f(B, N + 1, nx), us=f(B, N, 7), K=f(B, N, 7, nx), cost=f(B),
                iters=torch.full((B,), ISENT, dtype=torch.int32, device="cuda"),
                ok=torch.full((B,), 77, dtype=torch.uint8, device="cuda"), fn_pred=f(B, 2),
                stats=torch.full((B, 10), ISENT, dtype=torch.int32, device="cuda"))


def _host(t):
    _torch().cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in OUT}


def _solve_dev(solver, batch, **kw):
    B = int(batch.x0.shape[0])
    t = _inputs(batch)
    t.update(_fresh_outputs(B, solver.N, solver.nx))
    solver.solve_dev(t, maxiter=MAXITER, **kw)
    return _host(t)


def _as_solver(o):
    """solve_dev's outputs under the attribute names test_gpu_parity._check_solves reads."""
    return SimpleNamespace(ok=o["ok"].astype(bool), iter=o["iters"], stats=o["stats"], xs=o["xs"], us=o["us"], K=o["K"],
                           cost=o["cost"])


def _check_against_oracle(name, variant, contact, surf, cone, cfg, batch, got, fs, table_shape=True):
    """test_gpu_parity.test_solve_matches_oracle's checks and tolerances for the case: the oracle as it is, and for
    the point3d cases of parity's tables first the oracle with gains by Cholesky solves at the tight table.

    table_shape=False: the case's shape is not the one the explicit-inverse table (CROCODDYL_FORM_TOL, the
    oracle's own rounding error at N = 12, B = 4) was measured at.  The explicit-inverse oracle is then allowed its
    own error at this shape where that is larger: its distance d from the solve-form oracle, measured here
    between the two oracle solves, without the code under test.  The bound is the triangle inequality's,
    1.001 x (the tight tolerance, asserted just before) + d, never below the table's; 1.001 covers the two
    normalisations (max |K| differs by d between the forms).  Measured at N = 4, B = 3, classical point3d with the
    cone, ramp 5 -> 40 N: d = 4.70e-7 (K), 3.66e-5 (K element-wise) against the table's 1.5e-7 / 3e-5, and the
    library 5e-9 from the solve form; with the scalar 22 N on that shape d is 1.7e-7 already."""
    import test_gpu_parity as TP
    from helpers import elem_err, rel_err

    key = (variant, contact, surf, cone)
    s = _as_solver(got)
    if key in TP.CROCODDYL_FORM_TOL:
        ref = _oracle_solves(cfg, batch, fs, [TP.SOLVE_FORM, None])
        tight, tight_k = TP.CASE_TOL.get(key, (TP.TOL_SOLVE, TP.TOL_K))
        tight_ke = TP.CASE_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        TP._check_solves(name + "/solve_form", cfg, batch, s, ref[0], tight, tight_k, tight_ke)
        tol, tol_k = TP.CROCODDYL_FORM_TOL[key]
        tol_ke = TP.CROCODDYL_FORM_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        if not table_shape:
            pairs = list(zip(ref[1], ref[0]))
            d = max(rel_err(c[k], e[k]) for e, c in pairs for k in ("xs", "us", "cost"))  # scaled by the explicit
            d_k = max(rel_err(c["K"], e["K"]) for e, c in pairs)                           # form, as the check is
            d_ke = max(elem_err(c["K"], e["K"]) for e, c in pairs)
            print(name, "explicit-inverse oracle against its solve form:", d, d_k, d_ke)
            tol, tol_k, tol_ke = max(tol, 1.001 * tight + d), max(tol_k, 1.001 * tight_k + d_k), max(tol_ke, 1.001 * tight_ke + d_ke)
        TP._check_solves(name + "/crocoddyl_form", cfg, batch, s, ref[1], tol, tol_k, tol_ke)
        return ref[1]
    ref = _oracle_solves(cfg, batch, fs, [None])[0]
    TP._check_solves(name, cfg, batch, s, ref, TP.TOL_SOLVE, TP.TOL_K, TP.TOL_K_ELEM)
    return ref


SOLVE_CASES = [("classical", "normal_1d", 0), ("ff", "normal_1d", 0), ("classical", "point3d", 1), ("ff", "point3d", 1)]


def _horizon(contact):
    return 30 if contact == "normal_1d" else 12


# -- 1. same bits ----------------------------------------------------------------------------
@pytest.mark.parametrize("surf", [1, 0])
@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_constant_array_reproduces_the_scalar_path(variant, contact, cone, surf):
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    torch = _torch()
    N, B = _horizon(contact), 4
    cfg = _cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=21 + surf, surface=surf)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    full = torch.full((B, N + 1), float(cfg.fn_des), dtype=torch.float64, device="cuda")
    plain = _solve_dev(solver, b)
    runs = {"array": _solve_dev(solver, b, force_ref=full),
            "array+mask": _solve_dev(solver, b, force_ref=full, active=torch.ones(B, dtype=torch.uint8, device="cuda"))}
    if not surf:  # free space has no fn_track cost: any finite reference changes nothing
        rng = np.random.default_rng(3)
        runs["arbitrary"] = _solve_dev(solver, b, force_ref=_dev(rng.uniform(-50.0, 90.0, (B, N + 1))))
    assert np.all(plain["iters"] > 0) and np.all(plain["xs"] != SENTINEL)
    for tag, r in runs.items():
        for k in OUT:
            assert np.array_equal(r[k], plain[k], equal_nan=True), (tag, k)
    solver.close()


# -- 2. per-instance constant ----------------------------------------------------------------
F_CONST = (5.0, 14.0, 22.0, 40.0)


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_per_instance_constant_matches_oracle(variant, contact, cone):
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    N, B = _horizon(contact), 4
    cfg = _cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=22, surface=1)
    for k in ("x0", "node_ref", "inst_ref", "xs_init", "us_init", "surface"):  # instance 3 is instance 0 again:
        a = np.array(getattr(b, k))                                           # f = 5 against f = 40 on one problem
        a[3] = a[0]
        setattr(b, k, a)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    f = np.repeat(np.array(F_CONST)[:, None], N + 1, 1)
    got = _solve_dev(solver, b, force_ref=_dev(f))
    ref = _check_against_oracle(f"fref/const/{variant}/{contact}/cone{cone}", variant, contact, 1, cone, cfg, b, got,
                                list(F_CONST))
    spread = float(np.max(np.abs(got["xs"][0] - got["xs"][3])))
    print("max |xs(f=5) - xs(f=40)| =", spread, "oracle:", float(np.max(np.abs(ref[0]["xs"] - ref[3]["xs"]))))
    assert spread > 1e-3
    # the predicted force follows the reference: at knot 0 where the torque is a control (classical; the
    # force-feedback knot-0 torque is part of x0, so its knot-0 force is given), at knot 1 in both
    print("fn_pred f=5:", got["fn_pred"][0], "f=40:", got["fn_pred"][3])
    assert got["fn_pred"][0, 1] != got["fn_pred"][3, 1]
    if variant == "classical":
        assert got["fn_pred"][0, 0] < got["fn_pred"][3, 0]
    solver.close()


# -- 3. per-node profile ---------------------------------------------------------------------
NODE_CASES = [(v, c, s, cone) for v in ("classical", "ff")
              for c, s, cone in (("normal_1d", 1, 0), ("normal_1d", 0, 0), ("point3d", 1, 1), ("point3d", 0, 0))]


def _profiles(N):
    ramp = np.linspace(5.0, 40.0, N + 1)
    step = np.where(np.arange(N + 1) < N // 2, 8.0, 35.0)
    return np.stack([ramp, step, ramp[::-1].copy()])


@pytest.mark.parametrize("variant,contact,surf,cone", NODE_CASES)
def test_per_node_profile_matches_oracle(variant, contact, surf, cone):
    import test_gpu_parity as TP
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, oracle_cfg, oracle_problem, rel_err

    N, B = 4, 3
    cfg = _cfg(variant, N, contact, cone)
    ocfg = oracle_cfg(cfg)
    b = make_batch(variant, B, N, seed=11 + surf, surface=surf)
    f = _profiles(N)
    rng = np.random.default_rng(7)
    xs = b.xs_init + 0.02 * rng.normal(size=b.xs_init.shape)
    us = b.us_init + 0.5 * rng.normal(size=b.us_init.shape)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    out = solver.calc_diff(b, xs, us, force_ref=f)
    worst = {}
    for i in range(B):
        model = ForceRefOCP(ocfg, oracle_problem(b, i, N), f[i])
        run = model.running(slice(0, N), xs[i, :N], us[i], True)
        term = model.terminal(xs[i, N], True)
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
    # the reference reaches the cost: against the scalar call every contact node's cost moves, a free one's does not
    plain = solver.calc_diff(b, xs, us)
    moved = out["cost"] != plain["cost"]
    if surf:
        running = moved[:, :N].all()
        assert running, moved
        # the classical terminal node (contact force 0) keeps its constant term, now with f[N]
        f2 = f.copy()
        f2[:, N] += 7.0
        out2 = solver.calc_diff(b, xs, us, force_ref=f2)
        assert np.array_equal(out2["cost"][:, :N], out["cost"][:, :N])
        if variant == "classical":
            assert moved[:, N].all() and np.all(out2["cost"][:, N] != out["cost"][:, N])
            w = 0.5 * cfg.w_fn * (f2[:, N] ** 2 - f[:, N] ** 2)  # lambda = 0: 0.5 w_fn (0 - f)^2, normal weight 1
            assert np.allclose(out2["cost"][:, N] - out["cost"][:, N], w, rtol=1e-9, atol=0.0)
    else:
        for k in out:
            assert np.array_equal(out[k], plain[k], equal_nan=True), k
    # the solve
    got = _solve_dev(solver, b, force_ref=_dev(f))
    _check_against_oracle(f"fref/node/{variant}/{contact}/surf{surf}/cone{cone}", variant, contact, surf, cone, cfg, b, got,
                          [f[i] for i in range(B)], table_shape=False)
    solver.close()


# -- 4. mask and batch independence ----------------------------------------------------------
@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_masked_rows_equal_their_own_batch(variant):
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, product_cfg

    torch = _torch()
    N, B = 8, 300  # two blocks of every per-instance kernel, the second partly filled; four slices of 75
    cfg = product_cfg(variant, N)
    b = make_batch(variant, B, N, seed=1234)
    assert 0 < int(np.sum(np.asarray(b.surface) != 0)) < B
    rng = np.random.default_rng(8)
    f = rng.uniform(5.0, 40.0, (B, 1)) + np.linspace(0.0, 1.0, N + 1)[None, :] * rng.uniform(-4.0, 4.0, (B, 1))
    mask = np.zeros(B, np.uint8)
    mask[::3] = 1
    on = mask != 0
    # the selected instances in a batch of their own
    sub = SimpleNamespace(**{k: np.ascontiguousarray(np.asarray(getattr(b, k))[on])
                             for k in ("x0", "node_ref", "inst_ref", "xs_init", "us_init", "surface")})
    small = BatchedBoxFDDP(cfg, max_batch=int(on.sum()))
    alone = _solve_dev(small, sub, force_ref=_dev(f[on]))
    small.close()
    # the whole batch under the mask: the unselected rows' warm starts and references are NaN
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    t = _inputs(b)
    off = torch.from_numpy(~on).cuda()
    t["xs_init"][off] = float("nan")
    t["us_init"][off] = float("nan")
    fp = f.copy()
    fp[~on] = np.nan
    t.update(_fresh_outputs(B, N, cfg.nx))
    sent = _host(t)
    solver.solve_dev(t, maxiter=MAXITER, active=_dev(mask), force_ref=_dev(fp))
    got = _host(t)
    cols = [0, 1, 2, 3, 4, 8, 9]  # stats [5..7] count line-search passes, which follow the slice's active count
    for k in OUT:
        a, r = (got[k][on], alone[k]) if k != "stats" else (got[k][on][:, cols], alone[k][:, cols])
        assert np.array_equal(a, r, equal_nan=True), k
        assert np.array_equal(got[k][~on], sent[k][~on], equal_nan=True), k
    assert np.all(np.isfinite(got["xs"][on])) and len(np.unique(got["iters"][on])) > 1
    # the reference matters on this batch: the scalar solve differs where there is contact
    plain = _solve_dev(solver, b)
    surf = np.asarray(b.surface) != 0
    assert np.any(plain["xs"][on & surf] != got["xs"][on & surf])
    assert np.array_equal(plain["xs"][on & ~surf], got["xs"][on & ~surf])
    solver.close()


# -- 5. errors -------------------------------------------------------------------------------
def test_errors():
    from ffddp import BatchedBoxFDDP, _abi
    from helpers import make_batch, product_cfg

    torch = _torch()
    N, B = 4, 3
    cfg = product_cfg("classical", N)
    b = make_batch("classical", B, N, seed=5, surface=1)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    t = _inputs(b)
    t.update(_fresh_outputs(B, N, cfg.nx))
    good = torch.full((B, N + 1), 22.0, dtype=torch.float64, device="cuda")
    for bad in (good[:, :N].contiguous(), good[: B - 1], good.to(torch.float32), good.cpu(), good.t().contiguous().t(),
                np.full((B, N + 1), 22.0)):
        with pytest.raises(ValueError, match="force_ref"):
            solver.solve_dev(t, maxiter=MAXITER, force_ref=bad)
    with pytest.raises(ValueError, match="force_ref"):
        solver.calc_diff(b, b.xs_init, b.us_init, force_ref=np.zeros((B, N)))
    # a handle without the fn_track cost refuses the argument instead of ignoring it
    cfg0 = product_cfg("classical", N)
    cfg0.w_fn = 0.0
    s0 = BatchedBoxFDDP(cfg0, max_batch=B)
    p = lambda k: t[k].data_ptr()  # noqa: E731
    args = (B, p("x0"), p("node_ref"), p("inst_ref"), p("surface"), p("xs_init"), p("us_init"), MAXITER, 0, p("xs"),
            p("us"), p("K"), p("cost"), p("iters"), p("ok"), p("fn_pred"), p("stats"))
    lib = solver._lib
    assert lib.ffddp_solve_batch_fref_dev(s0._h, *args, None, good.data_ptr(), None) == -1
    assert b"w_fn" in lib.ffddp_last_error(s0._h)
    assert lib.ffddp_solve_batch_fref_dev(s0._h, *args, None, None, None) == 0  # without it: the plain solve
    with pytest.raises(Exception, match="w_fn"):
        s0.solve_dev(t, maxiter=MAXITER, force_ref=good)
    with pytest.raises(Exception, match="w_fn"):
        s0.calc_diff(b, b.xs_init, b.us_init, force_ref=np.full((B, N + 1), 22.0))
    torch.cuda.synchronize()
    s0.close()
    # null handles, and the neighbours' codes for the new fleet calls
    assert lib.ffddp_solve_batch_fref_dev(None, *args, None, good.data_ptr(), None) == -1
    assert lib.ffddp_calc_diff_fref(None, B, *([None] * 17)) == -1
    k0, ptr = _abi.FleetTasks(), good.data_ptr()
    assert lib.ffddp_fleet_force_refs_dev(None, B, k0, ptr, B, 22.0, ptr, None) == -1
    h = solver._h
    assert lib.ffddp_fleet_force_refs_dev(h, B, k0, None, B, 22.0, ptr, None) == -1
    assert lib.ffddp_fleet_force_refs_dev(h, B, k0, ptr, B, 22.0, None, None) == -1
    assert lib.ffddp_fleet_force_refs_dev(h, B, k0, ptr, -1, 22.0, ptr, None) == -1
    assert lib.ffddp_fleet_force_refs_dev(h, 0, k0, ptr, B, 22.0, ptr, None) == -1
    assert lib.ffddp_fleet_force_refs_dev(h, B + 1, k0, ptr, B, 22.0, ptr, None) == -4
    m = lambda h_, B_=B, rf=B: lib.ffddp_fleet_metrics_fref_dev(  # noqa: E731
        h_, B_, B_, ptr, 69, k0, 0, 0.005, ptr, 0.0, ptr, 22.0, None, None, None, ptr, ptr, rf, None)
    assert m(None) == -1 and m(h, 0) == -1 and m(h, B + 1) == -4 and m(h, B, -1) == -1
    torch.cuda.synchronize()
    solver.close()


# -- 6. the sampler kernel -------------------------------------------------------------------
def _force_records(rng, B):
    from ffddp.trajectory import ForceProfile, force_records

    prof = []
    for b in range(B):
        f0, f1 = rng.uniform(0.0, 40.0, 2)
        t_on = rng.uniform(0.7, 1.1)
        t_ramp = 0.0 if b % 3 == 1 else rng.uniform(0.01, 0.6)
        prof.append(ForceProfile(f0, f1, t_on, t_ramp))
    prof[0] = ForceProfile(5.0, 30.0, 0.9, 0.25)  # breakpoints the tick times below hit exactly
    prof[1] = ForceProfile(8.0, 35.0, 0.9, 0.0)
    prof[2] = ForceProfile(22.0, 22.0)
    return force_records(prof)


def test_force_sampler_matches_sample_force():
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset
    from ffddp.trajectory import sample_force

    torch = _torch()
    B, N, rows, fn_default = 300, 30, 290, 17.25  # 9300 lanes: 37 blocks, the last partly filled
    solver = BatchedBoxFDDP(classical_preset(N), max_batch=B, device=0)
    dt_ocp = float(solver.cfg.dt)
    rng = np.random.default_rng(12)
    frec = _force_records(rng, B)
    frec_d = _dev(frec[:rows])  # its own allocation, rows records long: nothing may be read past it
    delay = (np.arange(B) % 7) * 0.0013
    delay[:3] = 0.0
    trec = np.zeros((B, _abi.FLEET_TASK_W))
    trec[:, 21] = delay
    trec_d = _dev(trec)
    buf = torch.full((B + 1, N + 1), SENTINEL, dtype=torch.float64, device="cuda")
    knots = np.arange(N + 1, dtype=float) * dt_ocp
    seen = set()
    for t in (0.2, 0.9 - 30 * dt_ocp, 0.9, 0.9 + 0.125, 1.15, 0.9 + 0.25, 1.7, 4.0):  # straddling t_on and t_on + t_ramp
        for with_tasks in (True, False):
            buf.fill_(SENTINEL)
            tasks = solver.fleet_tasks(trec_d, np.zeros(3), t) if with_tasks else None
            solver.fleet_force_refs_dev(frec_d, buf[:B], t=t, tasks=tasks, rows=rows, fn_default=fn_default)
            torch.cuda.synchronize()
            got = buf.cpu().numpy()
            tau = t - (delay if with_tasks else 0.0 * delay)
            tk = tau[:, None] + knots[None, :]
            want = sample_force(frec[:rows], tk[:rows])
            assert np.array_equal(got[:rows], want), (t, with_tasks, float(np.max(np.abs(got[:rows] - want))))
            assert np.all(got[rows:B] == fn_default) and np.all(got[B] == SENTINEL)
            s = (tk[:rows] - frec[:rows, 2:3]) / np.where(frec[:rows, 3:4] > 0, frec[:rows, 3:4], 1.0)
            seen |= {"below"} if np.any(s < 0) else set()
            seen |= {"inside"} if np.any((s > 0) & (s < 1) & (frec[:rows, 3:4] > 0)) else set()
            seen |= {"above"} if np.any(s > 1) else set()
    assert seen == {"below", "inside", "above"}
    # instance 0 at t = 0.9: knot 0 sits on t_on, instance 1 steps there, instance 2 is constant
    solver.fleet_force_refs_dev(frec_d, buf[:B], t=0.9, rows=rows, fn_default=fn_default)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[0, 0] == 5.0 and got[0, -1] > 5.0 and got[1, 0] == 35.0 and np.all(got[2] == 22.0)
    solver.close()


# -- 7. the metrics kernel -------------------------------------------------------------------
def test_metrics_kernel_with_force_records():
    import test_fleet_tasks_cpu as TC
    import test_gpu_fleet_metrics as MT
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset
    from ffddp.runlog import accumulate_metrics, metrics_accumulators
    from ffddp.trajectory import sample_force, task_records

    torch = _torch()
    B, ld, calls, dt, fn_des, rows_f = 300, 320, 24, 0.005, 1.5, 290
    base = TC.make_tasks()
    tasks = [dataclasses.replace(base[b % 6], delay=(b % 7) * 0.0013) for b in range(B)]
    rec = task_records(tasks)
    rec_d = _dev(rec)
    t_phase = np.array([float(k.t_contact_phase) for k in tasks])
    solver = BatchedBoxFDDP(classical_preset(8), max_batch=B, device=0)
    rng = np.random.default_rng(29)
    frec = _force_records(rng, B)
    frec[:, :2] *= 0.05  # forces of the synthetic records' size (0..2 N)
    frec_d = _dev(frec[:rows_f])
    acc = metrics_accumulators(B, ld)
    acc_d, plain_d, null_d = (_dev(metrics_accumulators(B, ld)) for _ in range(3))
    tp_d = _dev(t_phase)
    ktasks = solver.fleet_tasks(rec_d, np.zeros(3))
    F = {k: i for i, k in enumerate(_abi.FLEET_METRICS_FIELDS)}
    p = lambda a: a.data_ptr() if a is not None else None  # noqa: E731
    for k in range(calls):
        t = 0.3 + 0.06 * k
        obs_d, obs, info, need, fail = MT._kernel_inputs(rng, B)
        ts = (t - rec[:, -1]) + dt
        p_ref = MT._sampler_positions(solver, rec_d, ts)
        f_ref = np.concatenate([sample_force(frec[:rows_f], ts[:rows_f]), np.full(B - rows_f, fn_des)])
        accumulate_metrics(acc, obs, p_ref, ts, t_phase, f_ref, info, need, fail)
        ktasks.t = t
        dev = dict(info=_dev(info), need=_dev(need), plant_fail=_dev(fail))
        solver.fleet_metrics_dev(acc_d, obs_d, tp_d, fn_des, tasks=ktasks, dt=dt, force=frec_d, **dev)
        # without records: ffddp_fleet_metrics_dev, through either entry point
        solver.fleet_metrics_dev(plain_d, obs_d, tp_d, fn_des, tasks=ktasks, dt=dt, **dev)
        rc = solver._lib.ffddp_fleet_metrics_fref_dev(solver._h, B, ld, p(obs_d), int(obs_d.stride(0)), ktasks, B, dt, None,
                                                      0.0, p(tp_d), fn_des, p(dev["info"]), p(dev["need"]),
                                                      p(dev["plant_fail"]), p(null_d), None, 0, None)
        assert rc == 0
    torch.cuda.synchronize()
    got, plain, null = (a.cpu().numpy() for a in (acc_d, plain_d, null_d))
    assert np.array_equal(got, acc, equal_nan=True), [k for k, i in F.items() if not np.array_equal(got[i], acc[i], equal_nan=True)]
    assert np.array_equal(null, plain, equal_nan=True)
    i = F["sum_abs_fn_err"]
    others = [j for j in range(_abi.FLEET_METRICS_W) if j != i]
    assert np.array_equal(got[others], plain[others], equal_nan=True)
    assert np.all(got[i, :rows_f] != plain[i, :rows_f]) and np.array_equal(got[i, rows_f:B], plain[i, rows_f:B])
    # the table mode: one shared reference row, the scalar series time
    acc2, acc2_d = metrics_accumulators(B, ld), _dev(metrics_accumulators(B, ld))
    for k in range(3):
        obs_d, obs, info, need, fail = MT._kernel_inputs(rng, B)
        pr, ts1 = rng.normal(0.0, 0.3, 3), 0.85 + 0.1 * k
        f_ref = np.concatenate([sample_force(frec[:rows_f], np.full(rows_f, ts1)), np.full(B - rows_f, fn_des)])
        accumulate_metrics(acc2, obs, pr, ts1, t_phase, f_ref)
        solver.fleet_metrics_dev(acc2_d, obs_d, tp_d, fn_des, p_ref=_dev(pr), ts=ts1, force=frec_d)
    torch.cuda.synchronize()
    assert np.array_equal(acc2_d.cpu().numpy(), acc2, equal_nan=True)
    solver.close()


# -- 8. the device loop ----------------------------------------------------------------------
LB, LN, LT0, LTICKS = 5, 8, 0.7, 34
L_DELAY_TICKS = (0, 1, 2, 3, 0)  # instance 4 is instance 0 in everything but its force profile
LOOP_CASES = [("classical", None), ("ff", None), ("classical", 3)]


def _loop(variant, period, **kw):
    import test_gpu_fleet_tasks as TG
    from ffddp import controller as CT
    from ffddp import robot as R
    from ffddp.fleet_loop import DeviceFleetLoop
    from ffddp.trajectory import benchmark_task

    ee, cal, dt = TG._scene()
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (LB, 7))
    q0[4] = q0[0]
    radius, omega = np.array([0.10, 0.07, 0.12, 0.09, 0.10]), np.array([1.5, 1.1, 1.9, 1.3, 1.5])
    tasks = [benchmark_task(ee, radius=r, omega=w, delay=d * dt) for r, w, d in zip(radius, omega, L_DELAY_TICKS)]
    make = CT.ff_benchmark_config if variant == "ff" else CT.classical_benchmark_config
    cfg = make(dt, benchmark_task(ee).z_contact, horizon=LN, phase_source="trajectory")
    tilt = np.array([0.0, 5.0, 10.0, -5.0, 0.0])
    return DeviceFleetLoop(variant, LB, None, cfg, q0, tilt_deg=tilt, steps=LTICKS, calibration=cal, t0=LT0, tasks=tasks,
                           solve_period=period, **kw)


def _hand_tick(loop, frec_d, fref_d):
    """DeviceFleetLoop's tick through the entry points themselves, the force reference sampled and passed by hand."""
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
    s.fleet_force_refs_dev(frec_d, fref_d, tasks=loop.ktasks, fn_default=float(loop.cfg.fn_des), stream=loop._stream)
    s.solve_dev(T, maxiter=int(loop.cfg.max_iters), is_feasible=False, stream=loop._stream, force_ref=fref_d, **sel)
    s.fleet_post_dev(T, loop.params, lpf=LPF_ALPHA, stream=loop._stream, **kw)
    loop._stepped = False
    loop.k = k + 1


def _same_results(ra, rb, tag, skip=()):
    assert set(ra) - set(skip) == set(rb) - set(skip), tag
    for k in rb:
        if k in skip or k == "summary":
            continue
        a, b = ra[k], rb[k]
        assert np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f"), (tag, k)


@pytest.mark.parametrize("variant,period", LOOP_CASES)
def test_loop_constant_profiles_equal_the_plain_loop(variant, period):
    from ffddp.trajectory import ForceProfile

    plain = _loop(variant, period, metrics=True)
    fn = float(plain.cfg.fn_des)
    const = _loop(variant, period, metrics=True, force_profiles=[ForceProfile(fn, fn)] * 3 + [None, ForceProfile(fn, fn)])
    nones = _loop(variant, period, metrics=True, force_profiles=[None] * LB)
    assert plain.frec is None and nones.frec is None and const.frec is not None
    for loop in (plain, const, nones):
        loop.run(LTICKS)
    rp, rc, rn = plain.results(), const.results(), nones.results()
    contact_ticks = (rp["surface"] != 0).sum(0)
    print("ticks with surface = 1 per instance", contact_ticks)
    assert np.all(contact_ticks >= 10)
    _same_results(rc, rp, (variant, period, "const"), skip=("force_rec",))
    _same_results(rn, rp, (variant, period, "nones"))
    assert np.array_equal(rc["metrics"], rp["metrics"], equal_nan=True)
    assert np.array_equal(rc["force_rec"], np.tile([fn, fn, 0.0, 0.0], (LB, 1)))
    if period is not None:
        assert 0.0 < rp["solved"].mean() < 1.0
    for loop in (plain, const, nones):
        loop.close()


@pytest.mark.parametrize("variant,period", LOOP_CASES)
def test_loop_distinct_profiles_equal_the_hand_stepped_loop(variant, period):
    from ffddp.trajectory import ForceProfile, force_records, sample_force

    torch = _torch()
    profiles = [ForceProfile(5.0, 5.0), ForceProfile(8.0, 35.0, 0.8, 0.05), ForceProfile(30.0, 10.0, 0.82, 0.0), None,
                ForceProfile(5.0, 40.0, 0.8, 0.04)]
    a = _loop(variant, period, force_profiles=profiles)
    o = _loop(variant, period)
    fn = float(o.cfg.fn_des)
    frec = force_records([ForceProfile(fn, fn) if p is None else p for p in profiles])
    assert np.array_equal(a.force_rec, frec)
    frec_d, fref_d = _dev(frec), torch.zeros((LB, LN + 1), dtype=torch.float64, device="cuda")
    a.run(LTICKS)
    for _ in range(LTICKS):
        _hand_tick(o, frec_d, fref_d)
    ra, ro = a.results(), o.results()
    contact_ticks = (ra["surface"] != 0).sum(0)
    assert np.all(contact_ticks >= 10), contact_ticks
    _same_results(ra, ro, (variant, period), skip=("force_rec",))
    # the last tick's force_ref, and what it should be
    torch.cuda.synchronize()
    last = a.force_ref.cpu().numpy()
    assert np.array_equal(last, fref_d.cpu().numpy())
    tk = ra["t_task"][-1][:, None] + np.arange(LN + 1, dtype=float)[None, :] * a.dt_ocp
    assert np.array_equal(last, sample_force(frec, tk))
    # instances 0 and 4 share the task, the start and the plant: their setpoints (5 N; 5 -> 40 N) tell them apart
    both = (ra["surface"][:, 0] != 0) & (ra["surface"][:, 4] != 0)
    assert both.sum() >= 10
    assert np.array_equal(ra["info"][~both, 0], ra["info"][~both, 4], equal_nan=True)  # free space: the same instance
    assert not np.array_equal(ra["info"][both, 0], ra["info"][both, 4], equal_nan=True)
    # and the loop differs from the plain one
    plain = _loop(variant, period)
    plain.run(LTICKS)
    assert not np.array_equal(plain.results()["info"], ra["info"], equal_nan=True)
    for loop in (a, o, plain):
        loop.close()


# -- 9. the sweep ----------------------------------------------------------------------------
def test_sweep_scores_each_instance_against_its_own_reference():
    from ffddp import fleet as FL

    kw = dict(device_loop=True, seeds=2, total_time=0.2, scenarios=("flat", "tilted_10"), verbose=False)
    plain = FL.run_sweep(**kw)
    logs = FL.run_sweep(force_spread=(8.0, 36.0), force_ramp=0.5, **kw)
    dev = FL.run_sweep(force_spread=(8.0, 36.0), force_ramp=0.5, device_summary=True, **kw)
    rec = logs["force_rec"]
    assert rec.shape == (4, 4) and np.array_equal(rec, dev["force_rec"]) and "force_rec" not in plain
    assert np.all(rec[:, 0] == 8.0) and np.all((rec[:, 1] >= 8.0) & (rec[:, 1] <= 36.0)) and len(set(rec[:, 1])) == 4
    assert np.all(rec[:, 2] == 1.0) and np.all(rec[:, 3] == 0.5)
    const = FL.run_sweep(force_spread=(8.0, 36.0), **kw)["force_rec"]
    assert np.array_equal(const[:, 0], rec[:, 1]) and np.array_equal(const[:, 1], rec[:, 1]) and not const[:, 2:].any()
    # 0.2 s never reaches the contact: fn = 0, so the error is the reference itself (8 N before the ramp), where
    # the plain sweep has the configuration's 22 N; the device sums run in tick order, numpy's mean pairwise
    e_logs, e_dev = logs["per_instance"]["avg_abs_force_err"], dev["per_instance"]["avg_abs_force_err"]
    assert np.array_equal(e_logs, np.full(4, 8.0)) and np.array_equal(plain["per_instance"]["avg_abs_force_err"], np.full(4, 22.0))
    n = logs["ticks"]
    assert np.all(np.abs(e_dev - e_logs) <= (2 * n + 8) * 2.0 ** -53 * e_logs)
