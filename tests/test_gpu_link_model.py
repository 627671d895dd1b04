"""GPU: per-instance link inertial parameters (link_rows / link_model) of the
device solve, of calc_diff, of the gravity torque, of the fleet pre kernel and
of the device fleet loop.

Three references, none of them stored numbers:
- the same library without the argument (rows of the nominal model must give
  its bits);
- a second handle created with ``robot=`` one instance's model, solving that
  instance alone: the kernels without the feature, the model their constants;
- the numpy oracle (oracle.fddp.SolverBoxFDDP), solved in this process with
  oracle.panda's LINK_MASS / LINK_COM / LINK_INERTIA monkeypatched to that
  instance's model, at tests/test_gpu_parity.py's tolerances.

Solves run at test_gpu_torque_limits.py's shapes (N = 12, B = 6, maxiter 10,
test_gpu_force_ref.SOLVE_CASES): nodes of two instances share a k_node wave and
a k_forward_g8 wave, the row layout and the wide first pass run; the mask test
at B = 300 covers the four slices and the two-groups-per-row layout."""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle.panda as OP
from oracle import ocp

import test_gpu_cost_weights as CW
import test_gpu_force_ref as FR
from test_gpu_force_ref import MAXITER, OUT, SENTINEL, SOLVE_CASES, _dev, _fresh_outputs, _host, _inputs, _solve_dev, _torch

pytestmark = pytest.mark.gpu

N_SOLVE, B_SOLVE = CW.N_SOLVE, CW.B_SOLVE
STAT_COLS = CW.STAT_COLS
PAYLOAD_I = np.array([[4.0e-3, 3.0e-4, -2.0e-4], [3.0e-4, 5.0e-3, 1.0e-4], [-2.0e-4, 1.0e-4, 3.0e-3]])
LINK_FACTORS = (0.8, 0.9, 1.1, 1.2, 0.85, 1.15, 1.05)


def _models():
    """Instance 0 nominal; 1 a 0.5 kg point payload at the EE offset; 2 a 2 kg payload off the axis with a full
    inertia whose three off-diagonals are distinct (a swapped xy / xz entry shows); 3 another mass factor per link (a
    joint-index mix-up shows); 4 only link 3 changed (a lane reading its neighbour's joint shows); 5 the rated 3 kg."""
    from ffddp import robot as R

    base = R.LinkModel()
    mass, com = R.MASS.copy(), R.COM.copy()
    mass[2] *= 1.1
    com[2, 1] += 0.01
    return [base, base.with_payload(0.5, R.EE_P), base.with_payload(2.0, [0.03, -0.02, 0.15], PAYLOAD_I),
            base.scaled(LINK_FACTORS), R.LinkModel(mass, com, R.INERTIA), base.with_payload(3.0, R.EE_P)]


def _rows(models):
    from ffddp.config import link_model_rows

    return link_model_rows(models)


class _patched:
    """oracle.panda under `model`: the three inertial arrays replaced for the block, nothing under oracle/ edited."""

    def __init__(self, model):
        self.mp, self.model = pytest.MonkeyPatch(), model

    def __enter__(self):
        self.mp.setattr(OP, "LINK_MASS", np.array(self.model.mass))
        self.mp.setattr(OP, "LINK_COM", np.array(self.model.com))
        self.mp.setattr(OP, "LINK_INERTIA", np.array(self.model.inertia))

    def __exit__(self, *exc):
        self.mp.undo()


# -- 1. rows of the nominal model --------------------------------------------------------------
@pytest.mark.parametrize("surf", [1, 0])
@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_nominal_rows_reproduce_the_call_without(variant, contact, cone, surf):
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import cost_weight_row, torque_limit_rows
    from helpers import make_batch

    torch = _torch()
    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=41 + surf, surface=surf)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    assert hasattr(solver._lib, "ffddp_solve_batch_mdl_dev")
    md = _dev(_rows([None] * B))
    assert tuple(md.shape) == (B, _abi.LINK_W)
    w = _dev(np.tile(cost_weight_row(cfg), (B, 1)))
    ul = _dev(torque_limit_rows(cfg, np.tile(np.asarray(cfg.tau_limits, float), (B, 1))))
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    full = torch.full((B, N + 1), float(cfg.fn_des), dtype=torch.float64, device="cuda")
    plain = _solve_dev(solver, b)
    runs = {"rows": _solve_dev(solver, b, link_model=md),
            "rows+mask": _solve_dev(solver, b, link_model=md, active=ones),
            "rows+fref": _solve_dev(solver, b, link_model=md, force_ref=full),
            "rows+cw": _solve_dev(solver, b, link_model=md, cost_weights=w),
            "rows+ul": _solve_dev(solver, b, link_model=md, torque_limits=ul),
            "rows+all": _solve_dev(solver, b, link_model=md, active=ones, force_ref=full, cost_weights=w,
                                   torque_limits=ul)}
    assert np.all(plain["iters"] > 0) and np.all(plain["xs"] != SENTINEL)
    for tag, r in runs.items():
        for k in OUT:
            assert np.array_equal(r[k], plain[k], equal_nan=True), (tag, k)
    # the other surface: calc_diff
    d = solver.calc_diff(b, b.xs_init, b.us_init)
    dm = solver.calc_diff(b, b.xs_init, b.us_init, link_model=_rows([None] * B))
    for k in d:
        assert np.array_equal(dm[k], d[k], equal_nan=True), k
    solver.close()


# -- 2. / 3. distinct rows -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distinct(variant, contact, cone):
    """The case's batch solved once with the six models' rows, and every instance solved alone by a handle created
    with robot= its model (the kernels without the feature) and by the nominal handle.  Shared by tests 2 and 3."""
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=42, surface=1)
    models = _models()
    rows = _rows(models)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    got = _solve_dev(solver, b, link_model=_dev(rows))
    plain = _solve_dev(solver, b)
    solver.close()
    alone, nominal = [], []
    one = BatchedBoxFDDP(cfg, max_batch=1)
    for i in range(B):
        s = BatchedBoxFDDP(cfg, max_batch=1, robot=models[i])
        alone.append(_solve_dev(s, CW._sub(b, [i])))
        s.close()
        nominal.append(_solve_dev(one, CW._sub(b, [i])))
    one.close()
    return SimpleNamespace(cfg=cfg, batch=b, models=models, rows=rows, got=got, plain=plain, alone=alone, nominal=nominal)


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_equal_own_model_handles(variant, contact, cone):
    d = _distinct(variant, contact, cone)
    got = d.got
    assert len({r.tobytes() for r in d.rows}) == B_SOLVE
    for i, a in enumerate(d.alone):
        assert got["iters"][i] == a["iters"][0] and got["ok"][i] == a["ok"][0], i
        assert np.array_equal(got["stats"][i][STAT_COLS], a["stats"][0][STAT_COLS]), i
        for k in ("xs", "us", "K", "cost", "fn_pred"):
            assert np.array_equal(got[k][i], a[k][0], equal_nan=True), (i, k)
    # the test cannot pass on ignored rows: every changed model moves its own handle's controls
    moved = [float(np.max(np.abs(d.alone[i]["us"][0] - d.nominal[i]["us"][0]))) for i in range(B_SOLVE)]
    print("max |us(own model) - us(nominal)| per instance", moved)
    assert moved[0] == 0.0 and all(m > 1.0e-6 for m in moved[1:]), moved
    assert np.all(np.isfinite(got["cost"]))
    # instance 0 (the nominal model) is the plain solve's
    assert all(np.array_equal(got[k][0], d.plain[k][0], equal_nan=True) for k in ("xs", "us", "K", "cost", "iters"))


# Which three instances (= models: instance i plans with model i) each case holds to the oracle; together every model
# of the set.  The choice follows the kernels without the feature: on this batch (seed 42) the own-model handles of
# the classical cases miss test_gpu_parity's table on instance 2 under every model tried (normal_1d: xs 3.95e-10
# against 1e-10 under model 2, 7.3e-10 under model 3, 6.1e-10 under model 5; point3d + cone: xs 8.4e-8 against the
# tight table's 1e-8 under model 2) and, point3d + cone, on instance 5 under its 3 kg payload (K 3.0e-8 against
# 5e-9): the instance's conditioning, which test_gpu_torque_limits.py met on the same batch.  Those pairs are left to
# the force-feedback cases, whose handles are inside the table on every instance; nothing is widened.
ORACLE_INSTANCES = {SOLVE_CASES[0]: (0, 1, 3), SOLVE_CASES[1]: (2, 4, 5), SOLVE_CASES[2]: (1, 3, 4),
                    SOLVE_CASES[3]: (0, 2, 5)}


def _oracle_solves(d, idx, consts):
    from helpers import oracle_cfg, oracle_problem

    out = []
    for i in idx:
        with _patched(d.models[i]):
            out.append(CW._solve_one((oracle_cfg(d.cfg), oracle_problem(d.batch, i, N_SOLVE), np.array(d.batch.xs_init[i]),
                                      np.array(d.batch.us_init[i]), consts)))
    return out


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_match_oracle(variant, contact, cone):
    """test_gpu_parity.test_solve_matches_oracle's checks and tolerance table, one in-process oracle solve per
    instance under that instance's model.  The own-model handles (the kernels without the feature) are held to the
    same table first, so an excess of the batch would be the feature's."""
    import test_gpu_parity as TP

    d = _distinct(variant, contact, cone)
    idx = list(ORACLE_INSTANCES[(variant, contact, cone)])
    assert set().union(*ORACLE_INSTANCES.values()) == set(range(B_SOLVE))
    key = (variant, contact, 1, cone)
    name = f"mdl/{variant}/{contact}/cone{cone}"
    sub = SimpleNamespace(**{k: np.asarray(getattr(d.batch, k))[idx] for k in CW.IN_KEYS})
    handles = {k: np.stack([d.alone[i][k][0] for i in idx]) for k in OUT}
    rows = {k: d.got[k][idx] for k in OUT}
    if key in TP.CROCODDYL_FORM_TOL:
        ref = [_oracle_solves(d, idx, TP.SOLVE_FORM), _oracle_solves(d, idx, None)]
        tight, tight_k = TP.CASE_TOL.get(key, (TP.TOL_SOLVE, TP.TOL_K))
        tight_ke = TP.CASE_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        tol, tol_k = TP.CROCODDYL_FORM_TOL[key]
        tol_ke = TP.CROCODDYL_FORM_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        for tag, o in (("handles", handles), ("rows", rows)):
            s = FR._as_solver(o)
            TP._check_solves(f"{name}/{tag}/solve_form", d.cfg, sub, s, ref[0], tight, tight_k, tight_ke)
            TP._check_solves(f"{name}/{tag}/crocoddyl_form", d.cfg, sub, s, ref[1], tol, tol_k, tol_ke)
        return
    ref = _oracle_solves(d, idx, None)
    for tag, o in (("handles", handles), ("rows", rows)):
        TP._check_solves(f"{name}/{tag}", d.cfg, sub, FR._as_solver(o), ref, TP.TOL_SOLVE, TP.TOL_K, TP.TOL_K_ELEM)


def test_payload_models_match_oracle_in_the_classical_case_on_other_instances():
    """The identity assignment leaves models 2 and 5 (the full-inertia payload and the rated 3 kg) to the
    force-feedback cases: in the classical normal_1d case their own instances are outside the table on the parent's
    kernels.  A second batch of rows, model i + 1 on instance i, holds them to the oracle there on instances 1 and 4,
    where the probe found the own-model handles inside the table; the handles first, then the rows, bit-identical."""
    import test_gpu_parity as TP
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    variant, contact, cone = SOLVE_CASES[0]
    assert (variant, contact) == ("classical", "normal_1d") and (variant, contact, 1, cone) not in TP.CROCODDYL_FORM_TOL
    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=42, surface=1)
    models = _models()
    shifted = [models[(i + 1) % B] for i in range(B)]
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    got = _solve_dev(solver, b, link_model=_dev(_rows(shifted)))
    solver.close()
    idx = [1, 4]
    assert [(i + 1) % B for i in idx] == [2, 5]
    alone = []
    for i in idx:
        s = BatchedBoxFDDP(cfg, max_batch=1, robot=shifted[i])
        alone.append(_solve_dev(s, CW._sub(b, [i])))
        s.close()
    for a, i in zip(alone, idx):
        for k in ("xs", "us", "K", "cost", "fn_pred", "iters", "ok"):
            assert np.array_equal(got[k][i], a[k][0], equal_nan=True), (i, k)
    d = SimpleNamespace(cfg=cfg, batch=b, models=shifted)
    ref = _oracle_solves(d, idx, None)
    sub = SimpleNamespace(**{k: np.asarray(getattr(b, k))[idx] for k in CW.IN_KEYS})
    handles = {k: np.stack([a[k][0] for a in alone]) for k in OUT}
    for tag, o in (("handles", handles), ("rows", {k: got[k][idx] for k in OUT})):
        TP._check_solves(f"mdl/shifted/{variant}/{contact}/{tag}", cfg, sub, FR._as_solver(o), ref, TP.TOL_SOLVE, TP.TOL_K,
                         TP.TOL_K_ELEM)


# -- 4. calc_diff ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,contact,surf,cone", FR.NODE_CASES)
def test_calc_diff_with_distinct_rows_matches_oracle(variant, contact, surf, cone):
    import test_gpu_parity as TP
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, oracle_cfg, oracle_problem, rel_err

    N, B = 4, 3
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=11 + surf, surface=surf)
    models = [_models()[i] for i in (0, 2, 3)]
    rows = _rows(models)
    rng = np.random.default_rng(7)
    xs = b.xs_init + 0.02 * rng.normal(size=b.xs_init.shape)
    us = b.us_init + 0.5 * rng.normal(size=b.us_init.shape)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    out = solver.calc_diff(b, xs, us, link_model=rows)
    worst = {}
    ocfg = oracle_cfg(cfg)
    for i in range(B):
        prob = oracle_problem(b, i, N)
        with _patched(models[i]):
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
    plain = solver.calc_diff(b, xs, us)
    for k in out:
        assert np.array_equal(out[k][0], plain[k][0], equal_nan=True), k
    assert np.all(out["xnext"][1:] != plain["xnext"][1:]) or np.any(out["Fx"][1:] != plain["Fx"][1:])
    solver.close()


# -- 5. mask, four slices, the two-groups-per-row layout -------------------------------------
@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_masked_rows_equal_their_own_batch(variant):
    from ffddp import BatchedBoxFDDP
    from ffddp import robot as R
    from helpers import make_batch, product_cfg

    torch = _torch()
    N, B = 8, 300
    cfg = product_cfg(variant, N)
    b = make_batch(variant, B, N, seed=1234)
    assert 0 < int(np.sum(np.asarray(b.surface) != 0)) < B
    rng = np.random.default_rng(36)
    base = R.LinkModel()
    models = [base.scaled(rng.choice([0.8, 0.9, 1.0, 1.1, 1.2], size=7)).with_payload(float(rng.uniform(0.0, 3.0)), R.EE_P)
              for _ in range(B)]
    rows = _rows(models)
    mask = np.zeros(B, np.uint8)
    mask[::3] = 1
    on = mask != 0
    small = BatchedBoxFDDP(cfg, max_batch=int(on.sum()))
    alone = _solve_dev(small, CW._sub(b, on), link_model=_dev(rows[on]))
    small.close()
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    t = _inputs(b)
    off = torch.from_numpy(~on).cuda()
    t["xs_init"][off] = float("nan")
    t["us_init"][off] = float("nan")
    rp = rows.copy()
    rp[~on] = np.nan
    pad = np.ones(rows.shape[1], bool)
    for j in range(7):
        pad[16 * j:16 * j + 13] = False
    rp[:, pad] = np.nan  # the padding of selected rows is never read
    t.update(_fresh_outputs(B, N, cfg.nx))
    sent = _host(t)
    solver.solve_dev(t, maxiter=MAXITER, active=_dev(mask), link_model=_dev(rp))
    got = _host(t)
    for k in OUT:
        a, r = (got[k][on], alone[k]) if k != "stats" else (got[k][on][:, STAT_COLS], alone[k][:, STAT_COLS])
        assert np.array_equal(a, r, equal_nan=True), k
        assert np.array_equal(got[k][~on], sent[k][~on], equal_nan=True), k
    assert np.all(np.isfinite(got["xs"][on])) and len(np.unique(got["iters"][on])) > 1
    plain = _solve_dev(solver, b)
    assert np.any(plain["xs"][on] != got["xs"][on])
    solver.close()


# -- 6. gravity torque -----------------------------------------------------------------------
def _postures(B):
    from ffddp import robot as R

    return R.Q_NEUTRAL + np.random.default_rng(5).uniform(-0.5, 0.5, (B, 7))


def _own_handle_gravity(cfg, models, q):
    """ffddp_gravity_torque_dev of a handle created with each model, on that instance's posture."""
    from ffddp import BatchedBoxFDDP

    torch = _torch()
    out = np.zeros_like(q)
    for i, m in enumerate(models):
        s = BatchedBoxFDDP(cfg, max_batch=1, robot=m)
        tau = torch.full((1, 7), SENTINEL, dtype=torch.float64, device="cuda")
        rc = s._lib.ffddp_gravity_torque_dev(s._h, 1, C.c_void_p(_dev(q[i:i + 1]).data_ptr()), C.c_void_p(tau.data_ptr()), None)
        assert rc == 0
        torch.cuda.synchronize()
        out[i] = tau.cpu().numpy()[0]
        s.close()
    return out


def test_gravity_torque_under_each_instances_model():
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset

    torch = _torch()
    models = _models()
    B = len(models)
    cfg = classical_preset(4)
    q = _postures(B)
    own = _own_handle_gravity(cfg, models, q)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    tau = torch.full((B, 7), SENTINEL, dtype=torch.float64, device="cuda")
    solver.gravity_torque_dev(_dev(q), tau, link_model=_dev(_rows(models)))
    torch.cuda.synchronize()
    got = tau.cpu().numpy()
    assert np.array_equal(got, own)
    host = np.stack([_abi.gravity_torque(q[i], _abi.make_robot(m))[0] for i, m in enumerate(models)])
    assert np.max(np.abs(got - host)) < 1e-12
    # without rows: the handle's model, ffddp_gravity_torque_dev's bits
    tau2 = torch.full((B, 7), SENTINEL, dtype=torch.float64, device="cuda")
    solver.gravity_torque_dev(_dev(q), tau2)
    torch.cuda.synchronize()
    assert np.max(np.abs(tau2.cpu().numpy() - _abi.gravity_torque(q))) < 1e-12
    assert np.array_equal(tau2.cpu().numpy()[0], got[0])
    assert np.all(np.max(np.abs(got[1:] - tau2.cpu().numpy()[1:]), 1) > 0.05)  # the load the solve tests rely on
    solver.close()


# -- 7. the pre kernel, called directly ------------------------------------------------------
@pytest.mark.parametrize("variant,sched", [("classical", False), ("ff", True)])
def test_pre_computes_the_torque_reference_under_each_model(variant, sched):
    import dataclasses

    import test_fleet_tasks_cpu as TC
    import test_gpu_fleet_loop_kernels as KT
    import test_gpu_fleet_tasks as TG
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset, ff_preset
    from ffddp.trajectory import task_records

    torch = _torch()
    models = _models()
    B, N = TG.B, TG.HORIZON
    assert B == len(models)
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rec_d = _dev(task_records([dataclasses.replace(k, delay=d) for k, d in zip(TC.make_tasks(), TG.PRE_DELAYS)]))
    md = _dev(_rows(models))
    Q = None
    if sched:
        Q = _abi.FleetSched()
        Q.period, Q.apply_filter, Q.dt = 3, 0, 0.005
    keys = TG.PRE_OUT + (("need",) if sched else ()) + KT.STATE_KEYS
    rng = np.random.default_rng(12)
    for mode in (0, 1, 2):
        P = KT._params(phase_source=mode & 1, posture_mode=mode & 1, torque_mode=mode)
        st, od, q_nom = TG._pre_inputs(rng, variant, N, nx)
        tasks = lambda: solver.fleet_tasks(rec_d, TG.P_OFF, 0.8)  # noqa: E731

        def run(how):
            t = TG._pre_tensors(st, od, q_nom, variant, N, nx, sched)
            if how == "rows":
                solver.fleet_pre_dev(t, P, stream=stream, sched=Q, tasks=tasks(), link_model=md)
            elif how == "plain":
                solver.fleet_pre_dev(t, P, stream=stream, sched=Q, tasks=tasks())
            else:  # the new entry point with NULL rows
                p = lambda k: C.c_void_p(int(t[k].data_ptr()) if t.get(k) is not None else 0)  # noqa: E731
                s_ = solver._fleet_state(t)
                th = t.get("tau_hat")
                sp = C.byref(solver._fleet_sched(t, Q)) if Q is not None else None
                rc = solver._lib.ffddp_fleet_pre_mdl_dev(
                    solver._h, B, C.byref(P), C.byref(s_), p("q"), p("v"), p("fn_meas"), p("contact"), p("ee_z"),
                    int(t["q"].stride(0)), int(t["fn_meas"].stride(0)), p("tau_hat"),
                    int(th.stride(0)) if th is not None else 0, p("q_nom"), tasks(), None, 0, p("x0"), p("surface"),
                    p("inst_ref"), p("node_ref"), p("xs_init"), p("us_init"), sp, None, C.c_void_p(stream))
                assert rc == 0, solver._lib.ffddp_last_error(solver._h)
            return KT._down(t, keys), (t["q"].cpu().numpy() if mode == 0 else q_nom)

        (got, qq), (plain, _), (null, _) = run("rows"), run("plain"), run("null")
        for k in keys:
            assert np.array_equal(null[k], plain[k], equal_nan=True), (mode, k)
            if k != "inst_ref":
                assert np.array_equal(got[k], plain[k], equal_nan=True), (mode, k)
        assert np.array_equal(got["inst_ref"][:, :14], plain["inst_ref"][:, :14])
        if mode == 2:
            assert not got["inst_ref"][:, 14:].any()
            continue
        tau = torch.full((B, 7), SENTINEL, dtype=torch.float64, device="cuda")
        solver.gravity_torque_dev(_dev(np.ascontiguousarray(qq)), tau, link_model=md)
        torch.cuda.synchronize()
        assert np.array_equal(got["inst_ref"][:, 14:], tau.cpu().numpy()), mode
        assert np.array_equal(got["inst_ref"][0], plain["inst_ref"][0])
        assert np.all(np.max(np.abs(got["inst_ref"][1:, 14:] - plain["inst_ref"][1:, 14:]), 1) > 1e-3)
        # table mode (no task records: node_ref1 / contact_hint) with rows: ffddp_fleet_pre_dev's / _pre_sched_dev's
        # outputs, and the same torques
        node1 = _dev(rng.normal(size=(N + 1, 6)))

        def table(rows):
            t = TG._pre_tensors(st, od, q_nom, variant, N, nx, sched)
            t["node_ref1"] = node1
            solver.fleet_pre_dev(t, P, True, stream=stream, sched=Q, link_model=rows)
            return KT._down(t, keys)

        tg, tp = table(md), table(None)
        for k in keys:
            if k != "inst_ref":
                assert np.array_equal(tg[k], tp[k], equal_nan=True), (mode, "table", k)
        assert np.array_equal(tg["node_ref"], np.broadcast_to(node1.cpu().numpy(), tg["node_ref"].shape))
        assert np.array_equal(tg["inst_ref"][:, :14], tp["inst_ref"][:, :14])
        assert np.array_equal(tg["inst_ref"][:, 14:], tau.cpu().numpy()), (mode, "table")
        assert np.array_equal(tg["inst_ref"][0], tp["inst_ref"][0])
    solver.close()


def test_entry_point_errors():
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset
    from helpers import make_batch

    torch = _torch()
    cfg = classical_preset(4)
    solver = BatchedBoxFDDP(cfg, max_batch=2, device=0)
    b = make_batch("classical", 2, 4, seed=3)
    with pytest.raises(ValueError, match="LINK_W"):
        _solve_dev(solver, b, link_model=_dev(np.zeros((2, 64))))
    with pytest.raises(ValueError, match="LINK_W"):
        solver.calc_diff(b, b.xs_init, b.us_init, link_model=np.zeros((2, 64)))
    lib, h = solver._lib, solver._h
    assert lib.ffddp_gravity_torque_mdl_dev(None, 1, None, C.c_void_p(8), None, None) == -1
    assert lib.ffddp_fleet_pre_mdl_dev(h, 0, *([None] * 7), 7, 1, None, 7, None, _abi.FleetTasks(), None, 0,
                                       *([None] * 6), None, None, None) == -1
    assert b"ffddp_fleet_pre_mdl_dev" in lib.ffddp_last_error(h)
    torch.cuda.synchronize()
    solver.close()


# -- 8. the device loop ----------------------------------------------------------------------
LB, LTICKS = 6, CW.LTICKS
L_DELAY_TICKS = (0, 1, 2, 3, 0, 1)
LOOP_CASES = FR.LOOP_CASES


def _loop(variant, period, steps=LTICKS, t0=0.78, tilt=(0.0, 5.0, 10.0, -5.0, 0.0, 2.5), **kw):
    """test_gpu_cost_weights._loop with six instances.  Instance 4 is instance 0 in everything but what **kw gives."""
    from ffddp import robot as R
    from ffddp.fleet_loop import DeviceFleetLoop
    from ffddp.trajectory import benchmark_task

    cfg, ee, cal, dt = CW._ctrl_cfg(variant)
    rng = np.random.default_rng(4)
    q0 = R.Q_NEUTRAL + rng.normal(0.0, 0.02, (LB, 7))
    q0[4] = q0[0]
    radius, omega = np.array([0.10, 0.07, 0.12, 0.09, 0.10, 0.08]), np.array([1.5, 1.1, 1.9, 1.3, 1.5, 1.7])
    tasks = [benchmark_task(ee, radius=r, omega=w, delay=d * dt) for r, w, d in zip(radius, omega, L_DELAY_TICKS)]
    return DeviceFleetLoop(variant, LB, None, cfg, q0, tilt_deg=np.asarray(tilt, float), steps=steps, calibration=cal,
                           t0=t0, tasks=tasks, solve_period=period, **kw)


def _hand_tick(loop, md_d):
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
    s.fleet_pre_dev(T, loop.params, False, stream=loop._stream, tasks=loop.ktasks, link_model=md_d, **kw)
    s.solve_dev(T, maxiter=int(loop.cfg.max_iters), is_feasible=False, stream=loop._stream, link_model=md_d, **sel)
    s.fleet_post_dev(T, loop.params, lpf=LPF_ALPHA, stream=loop._stream, **kw)
    loop._stepped = False
    loop.k = k + 1


@pytest.mark.parametrize("variant,period", LOOP_CASES)
def test_loop_nominal_models_equal_the_plain_loop(variant, period):
    from ffddp import robot as R

    plain = _loop(variant, period, metrics=True)
    nom = _loop(variant, period, metrics=True, link_models=[R.LinkModel()] * LB)
    non = _loop(variant, period, metrics=True, link_models=[None] * LB)
    assert plain.md is None and nom.md is not None and np.array_equal(nom.link_rows, non.link_rows)
    for loop in (plain, nom, non):
        loop.run(LTICKS)
    rp, ra, rl = plain.results(), nom.results(), non.results()
    print("ticks with surface = 1 per instance", (rp["surface"] != 0).sum(0))
    FR._same_results(ra, rp, (variant, period, "models"))
    FR._same_results(rl, rp, (variant, period, "none"))
    assert np.array_equal(ra["metrics"], rp["metrics"], equal_nan=True)
    assert np.array_equal(rl["metrics"], rp["metrics"], equal_nan=True)
    assert set(nom.state()) == set(plain.state())
    for loop in (plain, nom, non):
        loop.close()


@pytest.mark.parametrize("variant,period", LOOP_CASES)
def test_loop_distinct_models_equal_the_hand_stepped_loop(variant, period):
    models = _models()
    o = _loop(variant, period)
    a = _loop(variant, period, link_models=models)
    rows = _rows(models)
    assert np.array_equal(a.link_rows, rows)
    md_d = _dev(rows)
    a.run(LTICKS)
    for _ in range(LTICKS):
        _hand_tick(o, md_d)
    ra, ro = a.results(), o.results()
    FR._same_results(ra, ro, (variant, period))
    # instances 0 and 4 share the task, the start and the plant: their models tell them apart; and the loop differs
    # from the plain one, whose instance 0 (the nominal model) it keeps
    assert not np.array_equal(ra["info"][:, 0], ra["info"][:, 4], equal_nan=True)
    plain = _loop(variant, period)
    plain.run(LTICKS)
    rp = plain.results()
    assert not np.array_equal(rp["info"], ra["info"], equal_nan=True)
    assert np.array_equal(rp["info"][:, 0], ra["info"][:, 0], equal_nan=True)
    for loop in (a, o, plain):
        loop.close()


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_distinct_models_forty_ticks_flat(variant):
    ticks = 40
    loop = _loop(variant, None, steps=ticks, t0=0.7, tilt=(0.0,) * LB, metrics=True, link_models=_models())
    loop.run(ticks)
    r = loop.results()
    print("ticks with surface = 1 per instance", (r["surface"] != 0).sum(0), "| max tau_cmd_inf", r["tau_cmd_inf"].max(0))
    assert not np.any(r["plant_fail"])
    for k, v in r["summary"].items():
        assert np.all(np.isfinite(np.asarray(v, float))), (k, v)
    loop.close()


# -- 9. the sweep ----------------------------------------------------------------------------
def test_sweep_with_a_payload_spread():
    """run_sweep(device_loop=True, payload_spread=...): the drawn masses come back beside the summary, every
    whole-run summary is finite (from the logs and from the device accumulators) and the controllers' models matter."""
    from ffddp import fleet as FL

    kw = dict(scenarios=("flat", "tilted_10"), seeds=2, total_time=0.1, verbose=False, device_loop=True)
    plain = FL.run_sweep(**kw)
    out = FL.run_sweep(payload_spread=(0.5, 3.0), **kw)
    dev = FL.run_sweep(payload_spread=(0.5, 3.0), device_summary=True, **kw)
    assert "payload_mass" not in plain and out["instances"] == 4 and out["ticks"] == 20
    want = FL.sweep_payload_masses(out["seed"], (0.5, 3.0))
    assert np.array_equal(out["payload_mass"], want) and np.array_equal(dev["payload_mass"], want)
    assert np.all((want >= 0.5) & (want <= 3.0))
    whole_run = ("rms_tangential_error", "rms_3d_error", "avg_abs_force_err", "max_fn", "unstable_ticks",
                 "neg_accepted_ticks", "solve_not_ok_ticks")  # 0.1 s has no contact phase: those keys are NaN
    for k in whole_run:
        assert np.all(np.isfinite(out["per_instance"][k])) and np.all(np.isfinite(dev["per_instance"][k])), k
    assert np.any(out["per_instance"]["rms_3d_error"] != plain["per_instance"]["rms_3d_error"])
