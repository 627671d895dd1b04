"""GPU: per-instance base mount and gravity (mount_rows / mount) of the device
solve, of calc_diff, of the gravity torque, of the fleet pre kernel, the plant
record re-framing kernel and the device fleet loop.

Three references, none of them stored numbers:
- the same library without the argument (rows of the nominal mount must give
  its bits);
- a second handle created with ``mount=`` one instance's mount, solving that
  instance alone: the kernels without the feature, the mount their constants;
- the numpy oracle (oracle.fddp.SolverBoxFDDP), solved in this process with
  oracle.panda's JOINT_PLACEMENT_R / JOINT_PLACEMENT_P / GRAVITY monkeypatched
  to that instance's mount, at tests/test_gpu_parity.py's tolerances.

Solves run at test_gpu_link_model.py's shapes (N = 12, B = 6, maxiter 10,
test_gpu_force_ref.SOLVE_CASES); the mask test at B = 300 covers the four
slices and the two-groups-per-row layout; the record kernel runs two blocks,
the second with a tail."""
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
TRANSLATED = 5  # the instance whose mount is a pure translation


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]),
            "y": np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]),
            "z": np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])}[axis]


def _mounts():
    """Instance 0 nominal; 1 and 2 the table's frame at 5 and 15 degrees (a rotation about y through a pivot off the
    base: all twelve placement entries and two gravity entries move); 3 a frame rotated about x (the third gravity
    entry and the other off-diagonals: a transposed base_R shows) with a translation; 4 a physically re-mounted arm,
    gravity kept (placement and gravity no longer move together); 5 a pure translation (base_p alone)."""
    from ffddp import robot as R

    return [R.Mount(), R.Mount.table_tilt(5.0), R.Mount.table_tilt(15.0),
            R.Mount.in_frame(_rot("x", -8.0), [0.03, 0.0, 0.0]), R.Mount.remounted(_rot("x", 20.0), np.zeros(3)),
            R.Mount.remounted(np.eye(3), [0.05, -0.03, 0.02])]


def _rows(mounts):
    from ffddp.config import mount_rows

    return mount_rows(mounts)


def _is_nominal(m):
    from ffddp import robot as R

    return (np.array_equal(m.base_R, R.JOINT_R[0]) and np.array_equal(m.base_p, R.JOINT_P[0])
            and np.array_equal(m.gravity, R.GRAVITY))


def _ref_map(m):
    """(A, c): a point x of the nominal planning world is A x + c in the mount's, a free vector A v.  A frame's mount
    re-expresses the world; a re-mounted arm carries its references along."""
    from ffddp import robot as R

    if m.frame is not None:
        Rf, pf = m.frame
        return Rf.T, -Rf.T @ pf
    Rb = m.base_R @ R.JOINT_R[0].T
    return Rb, m.base_p - Rb @ R.JOINT_P[0]


def _mounted(b, mounts, tau):
    """The batch with every instance's references in its own planning world (positions and velocities), its torque
    reference tau[i] (the gravity torque under its mount) and the initial guess moved with it.  An instance under
    the nominal mount keeps its inputs bit for bit."""
    out = SimpleNamespace(**{k: np.array(getattr(b, k)) for k in CW.IN_KEYS})
    ff = out.x0.shape[1] == 21
    for i, m in enumerate(mounts):
        if _is_nominal(m):
            continue
        A, c = _ref_map(m)
        out.node_ref[i, :, :3] = b.node_ref[i, :, :3] @ A.T + c
        out.node_ref[i, :, 3:] = b.node_ref[i, :, 3:] @ A.T
        delta = tau[i] - b.inst_ref[i, 14:]
        out.inst_ref[i, 14:] = tau[i]
        out.us_init[i] = b.us_init[i] + delta
        if ff:
            out.x0[i, 14:] = b.x0[i, 14:] + delta
            out.xs_init[i, :, 14:] = b.xs_init[i, :, 14:] + delta
    return out


class _patched:
    """oracle.panda under `mount`: the three constants replaced for the block, nothing under oracle/ edited."""

    def __init__(self, mount):
        self.mp, self.mount = pytest.MonkeyPatch(), mount

    def __enter__(self):
        JR, JP = np.array(OP.JOINT_PLACEMENT_R), np.array(OP.JOINT_PLACEMENT_P)
        JR[0], JP[0] = self.mount.base_R, self.mount.base_p
        self.mp.setattr(OP, "JOINT_PLACEMENT_R", JR)
        self.mp.setattr(OP, "JOINT_PLACEMENT_P", JP)
        self.mp.setattr(OP, "GRAVITY", np.array(self.mount.gravity))

    def __exit__(self, *exc):
        self.mp.undo()


def _gravity_dev(solver, q, rows_d=None, link_d=None):
    torch = _torch()
    tau = torch.full((q.shape[0], 7), SENTINEL, dtype=torch.float64, device="cuda")
    solver.gravity_torque_dev(_dev(np.ascontiguousarray(q)), tau, link_model=link_d, mount=rows_d)
    torch.cuda.synchronize()
    return tau.cpu().numpy()


# -- 1. rows of the nominal mount --------------------------------------------------------------
@pytest.mark.parametrize("surf", [1, 0])
@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_nominal_rows_reproduce_the_call_without(variant, contact, cone, surf):
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import cost_weight_row, link_model_rows, torque_limit_rows
    from helpers import make_batch

    torch = _torch()
    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=41 + surf, surface=surf)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    assert hasattr(solver._lib, "ffddp_solve_batch_mnt_dev")
    mt = _dev(_rows([None] * B))
    assert tuple(mt.shape) == (B, _abi.MOUNT_W)
    w = _dev(np.tile(cost_weight_row(cfg), (B, 1)))
    ul = _dev(torque_limit_rows(cfg, np.tile(np.asarray(cfg.tau_limits, float), (B, 1))))
    md = _dev(link_model_rows([None] * B))
    ones = torch.ones(B, dtype=torch.uint8, device="cuda")
    full = torch.full((B, N + 1), float(cfg.fn_des), dtype=torch.float64, device="cuda")
    plain = _solve_dev(solver, b)
    runs = {"rows": _solve_dev(solver, b, mount=mt),
            "rows+mask": _solve_dev(solver, b, mount=mt, active=ones),
            "rows+fref": _solve_dev(solver, b, mount=mt, force_ref=full),
            "rows+cw": _solve_dev(solver, b, mount=mt, cost_weights=w),
            "rows+ul": _solve_dev(solver, b, mount=mt, torque_limits=ul),
            "rows+md": _solve_dev(solver, b, mount=mt, link_model=md),
            "rows+all": _solve_dev(solver, b, mount=mt, active=ones, force_ref=full, cost_weights=w, torque_limits=ul,
                                   link_model=md)}
    assert np.all(plain["iters"] > 0) and np.all(plain["xs"] != SENTINEL)
    for tag, r in runs.items():
        for k in OUT:
            assert np.array_equal(r[k], plain[k], equal_nan=True), (tag, k)
    # the other surface: calc_diff
    d = solver.calc_diff(b, b.xs_init, b.us_init)
    dm = solver.calc_diff(b, b.xs_init, b.us_init, mount=_rows([None] * B))
    da = solver.calc_diff(b, b.xs_init, b.us_init, mount=_rows([None] * B), link_model=link_model_rows([None] * B))
    for k in d:
        assert np.array_equal(dm[k], d[k], equal_nan=True), k
        assert np.array_equal(da[k], d[k], equal_nan=True), k
    solver.close()


# -- 2. / 3. distinct rows -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distinct(variant, contact, cone):
    """The case's batch, every instance's references in its own planning world, solved once with the six mounts'
    rows, and every instance solved alone by a handle created with mount= its mount (the kernels without the
    feature) and by the nominal handle.  The translated instance also on the references as they were: a translation
    moves the problem only through them.  Shared by tests 2 and 3."""
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch

    N, B = N_SOLVE, B_SOLVE
    cfg = FR._cfg(variant, N, contact, cone)
    b0 = make_batch(variant, B, N, seed=42, surface=1)
    mounts = _mounts()
    rows = _rows(mounts)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    tau = _gravity_dev(solver, b0.x0[:, :7], _dev(rows))
    b = _mounted(b0, mounts, tau)
    got = _solve_dev(solver, b, mount=_dev(rows))
    solver.close()
    alone, nominal = [], []
    one = BatchedBoxFDDP(cfg, max_batch=1)
    raw = None
    for i in range(B):
        s = BatchedBoxFDDP(cfg, max_batch=1, mount=mounts[i])
        alone.append(_solve_dev(s, CW._sub(b, [i])))
        if i == TRANSLATED:
            raw = (_solve_dev(s, CW._sub(b0, [i])), _solve_dev(one, CW._sub(b0, [i])))
        s.close()
        nominal.append(_solve_dev(one, CW._sub(b, [i])))
    one.close()
    return SimpleNamespace(cfg=cfg, batch0=b0, batch=b, mounts=mounts, rows=rows, got=got, alone=alone, nominal=nominal,
                           raw=raw, tau=tau)


# What the rows must move, computed with the numpy oracle before any device run: over the four cases
# the smallest max |us(own mount) - us(nominal mount)| on the same inputs is 1.34 N m (the 5 degree table frame, ff
# normal_1d; the largest 105), and for the translated instance on the references as they were the smallest max |xs|
# difference is 0.61 and the smallest |fn_pred| difference 9.7e-4 N (classical normal_1d, where both solves track
# the 22 N setpoint; 0.2 to 9.4 N in the other cases).  The bounds are two orders below the smallest of each.
US_MOVED, XS_MOVED, FN_MOVED = 1.0e-2, 5.0e-3, 1.0e-5


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_equal_own_mount_handles(variant, contact, cone):
    d = _distinct(variant, contact, cone)
    got = d.got
    assert len({r.tobytes() for r in d.rows}) == B_SOLVE
    for i, a in enumerate(d.alone):
        assert got["iters"][i] == a["iters"][0] and got["ok"][i] == a["ok"][0], i
        assert np.array_equal(got["stats"][i][STAT_COLS], a["stats"][0][STAT_COLS]), i
        for k in ("xs", "us", "K", "cost", "fn_pred"):
            assert np.array_equal(got[k][i], a[k][0], equal_nan=True), (i, k)
    # the test cannot pass on ignored rows: every mount moves its own handle's controls on the same inputs
    moved = [float(np.max(np.abs(d.alone[i]["us"][0] - d.nominal[i]["us"][0]))) for i in range(B_SOLVE)]
    print("max |us(own mount) - us(nominal)| per instance", moved)
    assert moved[0] == 0.0 and all(m > US_MOVED for m in moved[1:]), moved
    own, nom = d.raw
    dx = float(np.max(np.abs(own["xs"][0] - nom["xs"][0])))
    df = float(np.max(np.abs(own["fn_pred"][0] - nom["fn_pred"][0])))
    print("translated instance on the references as they were: max |xs| diff", dx, "max |fn_pred| diff", df)
    assert dx > XS_MOVED and df > FN_MOVED, (dx, df)
    assert np.all(np.isfinite(got["cost"]))
    # the gravity torque references the batch was built with are the host model's within rounding
    from ffddp import _abi
    host = np.stack([_abi.gravity_torque(d.batch0.x0[i, :7], _abi.make_robot(mount=m))[0] for i, m in enumerate(d.mounts)])
    assert np.max(np.abs(d.tau - host)) < 1e-12


# Which instances (= mounts: instance i plans under mount i) each case holds to the oracle; together every mount of
# the set in one classical and one force-feedback case.  The choice follows the kernels without the feature: the
# own-mount handles were probed against test_gpu_parity's table first.  Of the 24 (case, instance)
# pairs 23 are inside it; the translated instance 5 of the classical point3d + cone case misses the tight table on
# the own-mount handle (xs 1.68e-8 against 1e-8: the instance's conditioning, which test_gpu_link_model.py met on the
# same batch) and, bit-identical, on the rows.  That mount is held in the classical normal_1d case instead; nothing is
# widened.  Three or four instances per case keep the oracle solves to a few seconds.
ORACLE_INSTANCES = {SOLVE_CASES[0]: (0, 1, 3, 5), SOLVE_CASES[1]: (1, 3, 5), SOLVE_CASES[2]: (1, 2, 4),
                    SOLVE_CASES[3]: (0, 2, 4)}


def _oracle_solves(d, idx, consts):
    from helpers import oracle_cfg, oracle_problem

    out = []
    for i in idx:
        with _patched(d.mounts[i]):
            out.append(CW._solve_one((oracle_cfg(d.cfg), oracle_problem(d.batch, i, N_SOLVE), np.array(d.batch.xs_init[i]),
                                      np.array(d.batch.us_init[i]), consts)))
    return out


def _oracle_check(d, idx, key, name, tags=("handles", "rows")):
    """test_gpu_parity.test_solve_matches_oracle's checks and tolerance table on the instances idx."""
    import test_gpu_parity as TP

    variant, contact, _, cone = key
    sub = SimpleNamespace(**{k: np.asarray(getattr(d.batch, k))[idx] for k in CW.IN_KEYS})
    outs = {"handles": {k: np.stack([d.alone[i][k][0] for i in idx]) for k in OUT}, "rows": {k: d.got[k][idx] for k in OUT}}
    if key in TP.CROCODDYL_FORM_TOL:
        ref = [_oracle_solves(d, idx, TP.SOLVE_FORM), _oracle_solves(d, idx, None)]
        tight, tight_k = TP.CASE_TOL.get(key, (TP.TOL_SOLVE, TP.TOL_K))
        tight_ke = TP.CASE_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        tol, tol_k = TP.CROCODDYL_FORM_TOL[key]
        tol_ke = TP.CROCODDYL_FORM_TOL_K_ELEM.get(key, TP.TOL_K_ELEM)
        for tag in tags:
            s = FR._as_solver(outs[tag])
            TP._check_solves(f"{name}/{tag}/solve_form", d.cfg, sub, s, ref[0], tight, tight_k, tight_ke)
            TP._check_solves(f"{name}/{tag}/crocoddyl_form", d.cfg, sub, s, ref[1], tol, tol_k, tol_ke)
        return
    ref = _oracle_solves(d, idx, None)
    for tag in tags:
        TP._check_solves(f"{name}/{tag}", d.cfg, sub, FR._as_solver(outs[tag]), ref, TP.TOL_SOLVE, TP.TOL_K, TP.TOL_K_ELEM)


@pytest.mark.parametrize("variant,contact,cone", SOLVE_CASES)
def test_distinct_rows_match_oracle(variant, contact, cone):
    """One in-process oracle solve per instance under that instance's mount.  The own-mount handles (the kernels
    without the feature) are held to the same table first, so an excess of the batch would be the feature's."""
    d = _distinct(variant, contact, cone)
    idx = list(ORACLE_INSTANCES[(variant, contact, cone)])
    assert len(idx) >= 3
    for v in ("classical", "ff"):  # every mount in one classical and one force-feedback case
        assert set().union(*[set(i) for c, i in ORACLE_INSTANCES.items() if c[0] == v]) == set(range(B_SOLVE)), v
    _oracle_check(d, idx, (variant, contact, 1, cone), f"mnt/{variant}/{contact}/cone{cone}")


# -- 4. calc_diff ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,contact,surf,cone", FR.NODE_CASES)
def test_calc_diff_with_distinct_rows_matches_oracle(variant, contact, surf, cone):
    import test_gpu_parity as TP
    from ffddp import BatchedBoxFDDP
    from helpers import make_batch, oracle_cfg, oracle_problem, rel_err

    N, B = 4, 3
    cfg = FR._cfg(variant, N, contact, cone)
    b = make_batch(variant, B, N, seed=11 + surf, surface=surf)
    mounts = [_mounts()[i] for i in (0, 2, 4)]
    rows = _rows(mounts)
    rng = np.random.default_rng(7)
    xs = b.xs_init + 0.02 * rng.normal(size=b.xs_init.shape)
    us = b.us_init + 0.5 * rng.normal(size=b.us_init.shape)
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    out = solver.calc_diff(b, xs, us, mount=rows)
    worst = {}
    ocfg = oracle_cfg(cfg)
    for i in range(B):
        prob = oracle_problem(b, i, N)
        with _patched(mounts[i]):
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
    assert np.all(np.any(out["Lx"][1:] != plain["Lx"][1:], axis=(1, 2)))
    solver.close()


# -- 5. mask, four slices, the two-groups-per-row layout, the padding -------------------------
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
    rng = np.random.default_rng(37)
    mounts = []
    for i in range(B):
        Rf = _rot("xyz"[i % 3], float(rng.uniform(-6.0, 6.0))) @ _rot("xyz"[(i + 1) % 3], float(rng.uniform(-6.0, 6.0)))
        p = rng.uniform(-0.02, 0.02, 3)
        mounts.append(R.Mount.in_frame(Rf, p) if i % 2 else R.Mount.remounted(Rf, p))
    rows = _rows(mounts)
    mask = np.zeros(B, np.uint8)
    mask[::3] = 1
    on = mask != 0
    small = BatchedBoxFDDP(cfg, max_batch=int(on.sum()))
    alone = _solve_dev(small, CW._sub(b, on), mount=_dev(rows[on]))
    small.close()
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    t = _inputs(b)
    off = torch.from_numpy(~on).cuda()
    t["xs_init"][off] = float("nan")
    t["us_init"][off] = float("nan")
    rp = rows.copy()
    rp[~on] = np.nan
    rp[:, 15] = np.nan  # the padding of selected rows is never read
    t.update(_fresh_outputs(B, N, cfg.nx))
    sent = _host(t)
    solver.solve_dev(t, maxiter=MAXITER, active=_dev(mask), mount=_dev(rp))
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


def test_gravity_torque_under_each_instances_mount():
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp import robot as R
    from ffddp.config import classical_preset, link_model_rows

    torch = _torch()
    mounts = _mounts()
    B = len(mounts)
    cfg = classical_preset(4)
    q = _postures(B)
    own = np.zeros_like(q)
    for i, m in enumerate(mounts):
        s = BatchedBoxFDDP(cfg, max_batch=1, mount=m)
        tau = torch.full((1, 7), SENTINEL, dtype=torch.float64, device="cuda")
        rc = s._lib.ffddp_gravity_torque_dev(s._h, 1, C.c_void_p(_dev(q[i:i + 1]).data_ptr()), C.c_void_p(tau.data_ptr()), None)
        assert rc == 0
        torch.cuda.synchronize()
        own[i] = tau.cpu().numpy()[0]
        s.close()
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    rows_d = _dev(_rows(mounts))
    got = _gravity_dev(solver, q, rows_d)
    assert np.array_equal(got, own)
    host = np.stack([_abi.gravity_torque(q[i], _abi.make_robot(mount=m))[0] for i, m in enumerate(mounts)])
    assert np.max(np.abs(got - host)) < 1e-12
    # without rows: the handle's mount, ffddp_gravity_torque_dev's bits; the nominal rows give them too
    plain = _gravity_dev(solver, q)
    assert np.max(np.abs(plain - _abi.gravity_torque(q))) < 1e-12
    assert np.array_equal(plain[0], got[0])
    assert np.array_equal(_gravity_dev(solver, q, _dev(_rows([None] * B))), plain)
    # a change of frame (1..3) and a translation (5) leave the load as it is; the re-mounted arm's (4) moves
    assert np.max(np.abs(got[[1, 2, 3, 5]] - plain[[1, 2, 3, 5]])) < 1e-12
    assert np.max(np.abs(got[4] - plain[4])) > 1.0
    # with link rows as well: the own handle has both
    models = [R.LinkModel().with_payload(0.5 * (i + 1), R.EE_P) for i in range(B)]
    md = _dev(link_model_rows(models))
    both = _gravity_dev(solver, q, rows_d, md)
    hostb = np.stack([_abi.gravity_torque(q[i], _abi.make_robot(models[i], m))[0] for i, m in enumerate(mounts)])
    assert np.max(np.abs(both - hostb)) < 1e-12 and np.all(np.max(np.abs(both - got), 1) > 0.05)
    solver.close()


# -- 7. the pre kernel, called directly ------------------------------------------------------
@pytest.mark.parametrize("variant,sched", [("classical", False), ("ff", True)])
def test_pre_computes_the_torque_reference_under_each_mount(variant, sched):
    import dataclasses

    import test_fleet_tasks_cpu as TC
    import test_gpu_fleet_loop_kernels as KT
    import test_gpu_fleet_tasks as TG
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp import robot as R
    from ffddp.config import classical_preset, ff_preset, link_model_rows
    from ffddp.trajectory import task_records

    torch = _torch()
    mounts = _mounts()
    B, N = TG.B, TG.HORIZON
    assert B == len(mounts)
    md = _dev(link_model_rows([R.LinkModel().with_payload(0.5 * (i + 1), R.EE_P) for i in range(B)]))
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rec_d = _dev(task_records([dataclasses.replace(k, delay=d) for k, d in zip(TC.make_tasks(), TG.PRE_DELAYS)]))
    mt = _dev(_rows(mounts))
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
                solver.fleet_pre_dev(t, P, stream=stream, sched=Q, tasks=tasks(), mount=mt)
            elif how == "plain":
                solver.fleet_pre_dev(t, P, stream=stream, sched=Q, tasks=tasks())
            elif how == "link":  # ffddp_fleet_pre_mdl_dev
                solver.fleet_pre_dev(t, P, stream=stream, sched=Q, tasks=tasks(), link_model=md)
            elif how == "rows+link":
                solver.fleet_pre_dev(t, P, stream=stream, sched=Q, tasks=tasks(), link_model=md, mount=mt)
            else:  # the new entry point with NULL rows
                p = lambda k: C.c_void_p(int(t[k].data_ptr()) if t.get(k) is not None else 0)  # noqa: E731
                s_ = solver._fleet_state(t)
                th = t.get("tau_hat")
                sp = C.byref(solver._fleet_sched(t, Q)) if Q is not None else None
                rc = solver._lib.ffddp_fleet_pre_mnt_dev(
                    solver._h, B, C.byref(P), C.byref(s_), p("q"), p("v"), p("fn_meas"), p("contact"), p("ee_z"),
                    int(t["q"].stride(0)), int(t["fn_meas"].stride(0)), p("tau_hat"),
                    int(th.stride(0)) if th is not None else 0, p("q_nom"), tasks(), None, 0, p("x0"), p("surface"),
                    p("inst_ref"), p("node_ref"), p("xs_init"), p("us_init"), sp, None, None, C.c_void_p(stream))
                assert rc == 0, solver._lib.ffddp_last_error(solver._h)
            return KT._down(t, keys), (t["q"].cpu().numpy() if mode == 0 else q_nom)

        (got, qq), (plain, _), (null, _) = run("rows"), run("plain"), run("null")
        for k in keys:
            assert np.array_equal(null[k], plain[k], equal_nan=True), (mode, k)
            if k != "inst_ref":
                assert np.array_equal(got[k], plain[k], equal_nan=True), (mode, k)
        assert np.array_equal(got["inst_ref"][:, :14], plain["inst_ref"][:, :14])
        # with link rows as well, against ffddp_fleet_pre_mdl_dev: every other output is its, the torques are the
        # ones under both rows
        (both, _), (link, _) = run("rows+link"), run("link")
        for k in keys:
            if k != "inst_ref":
                assert np.array_equal(both[k], link[k], equal_nan=True), (mode, "link", k)
        assert np.array_equal(both["inst_ref"][:, :14], link["inst_ref"][:, :14])
        if mode == 2:
            assert not got["inst_ref"][:, 14:].any() and not both["inst_ref"][:, 14:].any()
            continue
        tau = _gravity_dev(solver, np.ascontiguousarray(qq), mt)
        assert np.array_equal(got["inst_ref"][:, 14:], tau), mode
        tau_both = _gravity_dev(solver, np.ascontiguousarray(qq), mt, md)
        assert np.array_equal(both["inst_ref"][:, 14:], tau_both), mode
        assert np.all(np.max(np.abs(tau_both - tau), 1) > 0.05)  # the payloads' load
        assert np.max(np.abs(both["inst_ref"][4, 14:] - link["inst_ref"][4, 14:])) > 1.0
        assert np.array_equal(got["inst_ref"][0], plain["inst_ref"][0])
        assert np.max(np.abs(got["inst_ref"][4, 14:] - plain["inst_ref"][4, 14:])) > 1.0  # the re-mounted arm's load
        # table mode (no task records: node_ref1 / contact_hint) with rows: ffddp_fleet_pre_dev's / _pre_sched_dev's
        # outputs, and the same torques
        node1 = _dev(rng.normal(size=(N + 1, 6)))

        def table(rows):
            t = TG._pre_tensors(st, od, q_nom, variant, N, nx, sched)
            t["node_ref1"] = node1
            solver.fleet_pre_dev(t, P, True, stream=stream, sched=Q, mount=rows)
            return KT._down(t, keys)

        tg, tp = table(mt), table(None)
        for k in keys:
            if k != "inst_ref":
                assert np.array_equal(tg[k], tp[k], equal_nan=True), (mode, "table", k)
        assert np.array_equal(tg["inst_ref"][:, :14], tp["inst_ref"][:, :14])
        assert np.array_equal(tg["inst_ref"][:, 14:], tau), (mode, "table")
        assert np.array_equal(tg["inst_ref"][0], tp["inst_ref"][0])
    solver.close()


# -- 8. the record kernel --------------------------------------------------------------------
def _reframe_numpy(obs, frame, sel):
    """ffddp_fleet_obs_frame_dev restated: each entry (R[0][i] x0 + R[1][i] x1) + R[2][i] x2, in that order."""
    out = obs.copy()
    Rm, p = frame[:, :9].reshape(-1, 3, 3), frame[:, 9:]

    def rt(x0, x1, x2, i):
        return (Rm[:, 0, i] * x0 + Rm[:, 1, i] * x1) + Rm[:, 2, i] * x2

    d = [obs[:, 28 + k] - p[:, k] for k in range(3)]
    for i in range(3):
        out[:, 28 + i] = rt(d[0], d[1], d[2], i)
        out[:, 31 + i] = rt(obs[:, 31], obs[:, 32], obs[:, 33], i)
        out[:, 43 + i] = rt(obs[:, 43], obs[:, 44], obs[:, 45], i)
        for j in range(3):
            out[:, 34 + 3 * i + j] = rt(obs[:, 34 + j], obs[:, 37 + j], obs[:, 40 + j], i)
        for j in range(7):
            out[:, 48 + 7 * i + j] = rt(obs[:, 48 + j], obs[:, 55 + j], obs[:, 62 + j], i)
    keep = sel == 0
    out[keep] = obs[keep]
    return out


def test_record_kernel_equals_its_numpy_restatement():
    import test_gpu_fleet_mismatch as FM
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp import plant as PL
    from ffddp import robot as R
    from ffddp.config import classical_preset

    torch = _torch()
    B = FM.PLANT_B
    assert B == 70 and _abi.PLANT_OBS == 69
    q, v, tau, tilts, phys = FM._plant_inputs(3)
    plant = PL.BatchedPlant(B, timestep=0.001, n_substeps=5, physics=phys)
    plant.q, plant.v = q.copy(), v.copy()
    plant.set_tilt(tilts)
    obs = plant.step(tau, integrate=False).copy()
    plant.close()
    assert np.any(obs[:, 46] > 0.0) and np.any(obs[:, 46] == 0.0) and np.all(np.isfinite(obs))
    rng = np.random.default_rng(8)
    mounts = [R.Mount.table_tilt(float(t)) if b % 3 else R.Mount.in_frame(_rot("x", float(rng.uniform(-10, 10))) @
                                                                            _rot("z", float(rng.uniform(-10, 10))),
                                                                            rng.uniform(-0.05, 0.05, 3))
              for b, t in enumerate(tilts)]
    frame = np.stack([m.obs_frame() for m in mounts])
    sel = (np.arange(B) % 5 != 1).astype(np.uint8)
    frame_n = frame.copy()
    frame_n[sel == 0] = np.nan  # an unselected instance's frame row is not read
    solver = BatchedBoxFDDP(classical_preset(4), max_batch=B)
    LD = 72
    out = torch.full((B, LD), SENTINEL, dtype=torch.float64, device="cuda")
    solver.fleet_obs_frame_dev(_dev(obs), _dev(frame_n), out[:, :], sel=_dev(sel))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = _reframe_numpy(obs, frame, sel)
    assert np.array_equal(got[:, :69], want)
    assert np.all(got[:, 69:] == SENTINEL)  # the stride's padding is not written
    untouched = list(range(0, 28)) + [46, 47]
    assert np.array_equal(got[:, untouched], obs[:, untouched])
    assert np.array_equal(got[sel == 0, :69], obs[sel == 0])
    identity = np.all(frame == R.Mount().obs_frame(), axis=1)  # the table's frame at tilt 0
    on = (sel != 0) & ~identity
    assert identity.any() and np.all(np.any(got[on, 28:46] != obs[on, 28:46], axis=1))
    assert np.array_equal(got[identity, :69], obs[identity])
    # sel == NULL: all; a strided input
    wide = torch.full((B, 80), SENTINEL, dtype=torch.float64, device="cuda")
    wide[:, :69] = _dev(obs)
    out2 = torch.full((B, 69), SENTINEL, dtype=torch.float64, device="cuda")
    solver.fleet_obs_frame_dev(wide, _dev(frame), out2)
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), _reframe_numpy(obs, frame, np.ones(B, np.uint8)))
    # in the table's frame a touching tool's contact force points along +z: the tilt is gone
    t10 = [b for b in range(B) if b % 3 and tilts[b] == 10.0 and obs[b, 46] > 0.0]  # _plant_inputs: the touching ones
    assert t10
    fw = out2.cpu().numpy()[t10, 43:46]
    assert np.all(np.abs(fw[:, 0]) < 1e-9 * np.abs(fw[:, 2])) and np.all(np.abs(obs[t10, 43]) > 0.15 * np.abs(obs[t10, 45]))
    # refusals
    lib, h = solver._lib, solver._h
    o_, f_, u_ = C.c_void_p(_dev(obs).data_ptr()), C.c_void_p(_dev(frame).data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.ffddp_fleet_obs_frame_dev(None, B, o_, 69, f_, None, u_, LD, None) == -1
    for args in ((B, None, 69, f_, None, u_, LD), (B, o_, 69, None, None, u_, LD), (B, o_, 69, f_, None, None, LD),
                 (B, o_, 68, f_, None, u_, LD), (B, o_, 69, f_, None, u_, 68), (0, o_, 69, f_, None, u_, LD)):
        assert lib.ffddp_fleet_obs_frame_dev(h, *args, None) == -1, args
        assert b"ffddp_fleet_obs_frame_dev" in lib.ffddp_last_error(h)
    assert lib.ffddp_fleet_obs_frame_dev(h, B + 1, o_, 69, f_, None, u_, LD, None) == -4
    torch.cuda.synchronize()
    solver.close()


def test_entry_point_errors():
    from ffddp import BatchedBoxFDDP, _abi
    from ffddp.config import classical_preset
    from helpers import make_batch

    torch = _torch()
    cfg = classical_preset(4)
    solver = BatchedBoxFDDP(cfg, max_batch=2, device=0)
    b = make_batch("classical", 2, 4, seed=3)
    with pytest.raises(ValueError, match="MOUNT_W"):
        _solve_dev(solver, b, mount=_dev(np.zeros((2, 12))))
    with pytest.raises(ValueError, match="MOUNT_W"):
        solver.calc_diff(b, b.xs_init, b.us_init, mount=np.zeros((2, 12)))
    lib, h = solver._lib, solver._h
    assert lib.ffddp_gravity_torque_mnt_dev(None, 1, None, None, C.c_void_p(8), None, None) == -1
    q_d, tau_d = _dev(np.zeros((2, 7))), _dev(np.zeros((2, 7)))
    mt_d = _dev(_rows([None, None]))
    qp, tp, mp = (C.c_void_p(a.data_ptr()) for a in (q_d, tau_d, mt_d))
    for rows in (None, mp):  # a null q or tau is refused before any launch, with and without rows
        assert lib.ffddp_gravity_torque_mnt_dev(h, 2, None, None, rows, tp, None) == -1
        assert lib.ffddp_gravity_torque_mnt_dev(h, 2, qp, None, rows, None, None) == -1
        assert b"ffddp_gravity_torque_mnt_dev" in lib.ffddp_last_error(h)
        assert lib.ffddp_gravity_torque_mnt_dev(h, 2, qp, None, rows, tp, None) == 0
        assert lib.ffddp_gravity_torque_mnt_dev(h, 0, None, None, rows, None, None) == 0
    assert lib.ffddp_fleet_pre_mnt_dev(h, 0, *([None] * 7), 7, 1, None, 7, None, _abi.FleetTasks(), None, 0,
                                       *([None] * 6), None, None, None, None) == -1
    assert b"ffddp_fleet_pre_mnt_dev" in lib.ffddp_last_error(h)
    torch.cuda.synchronize()
    solver.close()


# -- 9. the device loop ----------------------------------------------------------------------
LB, TICKS = 6, 40
LOOP_TILTS = (0.0, 5.0, 10.0, 15.0, 5.0, 10.0)


def _loop(variant, tilt=LOOP_TILTS, **kw):
    """test_gpu_fleet_mismatch._loop_setup's loop (six instances, 40 ticks from 0.7 s across the references' contact
    switch, mixed injector profiles, per-instance plant physics) with the tilts and **kw as arguments."""
    import test_gpu_fleet_mismatch as FM
    from ffddp import controller as CT
    from ffddp import fleet as FL
    from ffddp import plant as PL
    from ffddp import robot as R
    from ffddp.fleet_loop import DeviceFleetLoop
    from ffddp.trajectory import benchmark_traj

    assert (FM.LB, FM.TICKS) == (LB, TICKS)
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
    scale = np.array([1.0, 0.9, 1.1, 0.95, 1.05, 1.0])[:, None] * np.linspace(0.95, 1.05, 7)
    ucfgs = [None] * LB
    for b, c in zip(FM.INJECTED, FM.CM.mixed_configs(FM.LOOP_DELAYS, seed0=100)):
        ucfgs[b] = c
    phys = [PL.PlantPhysics(armature=0.05 + 0.03 * b, damping=np.linspace(0.5, 1.5, 7) * (1.0 + 0.1 * b),
                            r_tool=0.03 + 0.0002 * b, margin=0.001 + 0.0001 * b, solref=(0.01 + 0.004 * b, 0.8 + 0.08 * b),
                            solimp=(0.85 + 0.01 * b, 0.95, 0.001 * (1 + b), 0.4 + 0.04 * b, float(1 + b % 3)))
            for b in range(LB)]
    if kw.get("metrics"):
        kw = dict(kw, t_contact_phase=float(meta["t_contact_phase"]))
    return DeviceFleetLoop(variant, LB, traj, cfg, q0, tilt_deg=np.asarray(tilt, float), torque_scale=scale, steps=TICKS,
                           calibration=cal, t0=FM.T0, uncertainty=ucfgs, noise="numpy", plant_physics=phys, **kw)


def _tilt_mounts(tilt=LOOP_TILTS):
    from ffddp import robot as R

    return [R.Mount.table_tilt(a) if a != 0.0 else None for a in tilt]


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_without_mounts_is_the_plain_loop(variant):
    plain = _loop(variant, metrics=True)
    non = _loop(variant, metrics=True, mounts=[None] * LB)
    assert plain.mt is None and non.mt is None and non.obs_frame is None
    for loop in (plain, non):
        loop.run(TICKS)
    rp, rn = plain.results(), non.results()
    FR._same_results(rn, rp, (variant, "none"))
    assert np.array_equal(rn["metrics"], rp["metrics"], equal_nan=True)
    assert set(non.state()) == set(plain.state())
    for loop in (plain, non):
        loop.close()


def _hand_run(o, mounts, ticks):
    """DeviceFleetLoop's ticks through the entry points themselves on a loop built without mounts: the rows, the
    frames and the re-framed records by hand."""
    from ffddp import robot as R
    from ffddp.fleet_loop import LPF_ALPHA

    torch = _torch()
    s, T = o.solver, o.T
    mt = _dev(_rows(mounts))
    frame = _dev(np.stack([(R.Mount() if m is None else m).obs_frame() for m in mounts]))
    sel = _dev(np.array([m is not None for m in mounts], np.uint8))
    fr = torch.zeros((o.B, 69), dtype=torch.float64, device="cuda")
    T.update(tau_bias=fr[:, 14:21], fn_meas=fr[:, 46], contact=fr[:, 47], ee_z=fr[:, 30], obs=fr)
    assert o.inject is not None  # q, v: the injector's outputs, fed from the plant's own record

    def reframe():
        s.fleet_obs_frame_dev(o.P["obs"], frame, fr, sel=sel, stream=o._stream)

    reframe()  # the start sequence's first observation
    for _ in range(ticks):
        k = o.k
        if not o._stepped:
            o._plant_step()
            reframe()
        r = o._row(k)
        T["info"], T["log_obs"] = o.log_info[r], o.log_obs[r]
        T["node_ref1"], hint = o.ref_table[k], bool(o.hints[k])
        s.fleet_inject_obs_dev(o.J, o.inject, k, z=o.z_table[k], stream=o._stream, rows=o.inject_rows)
        s.fleet_pre_dev(T, o.params, hint, stream=o._stream, mount=mt)
        s.solve_dev(T, maxiter=int(o.cfg.max_iters), is_feasible=False, stream=o._stream, mount=mt)
        s.fleet_post_dev(T, o.params, lpf=LPF_ALPHA, stream=o._stream)
        s.fleet_inject_cmd_dev(o.J, o.inject, k, stream=o._stream, rows=o.inject_rows)
        o._stepped = False
        o.k = k + 1
    o._plant_step()  # the closing record
    reframe()
    o._stepped = True


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_loop_with_table_mounts_equals_the_hand_stepped_loop(variant):
    mounts = _tilt_mounts()
    a = _loop(variant, mounts=mounts)
    m = _loop(variant, mounts=mounts, metrics=True)
    o = _loop(variant)
    hidden = _loop(variant)
    assert np.array_equal(a.mount_rows, _rows(mounts)) and a.frame_rows.shape == (LB, 12)
    assert not a.hints[0] and a.hints[TICKS - 1]  # the run crosses the references' contact switch
    a.run(TICKS)
    m.run(TICKS)
    hidden.run(TICKS)
    _hand_run(o, mounts, TICKS)
    ra, rm, ro, rh = a.results(), m.results(), o.results(), hidden.results()
    FR._same_results(ra, ro, (variant, "hand"))
    FR._same_results(rm, ra, (variant, "metrics"), skip=("metrics", "summary"))
    assert not np.any(ra["plant_fail"]) and not np.any(rm["plant_fail"])
    for k, v in rm["summary"].items():
        assert np.all(np.isfinite(np.asarray(v, float))), (k, v)
    # the level instance is the hidden-tilt loop's; every mounted instance's log differs from it
    assert np.array_equal(ra["obs"][:, 0], rh["obs"][:, 0]) and np.array_equal(ra["info"][:, 0], rh["info"][:, 0], equal_nan=True)
    for b in range(1, LB):
        assert not np.array_equal(ra["obs"][:, b], rh["obs"][:, b]), b
        assert not np.array_equal(ra["info"][:, b], rh["info"][:, b], equal_nan=True), b
    assert set(a.state()) == set(hidden.state())
    for loop in (a, m, o, hidden):
        loop.close()


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_mounted_loop_rewound_with_load_state_repeats_its_logs(variant):
    """state() at the start, a run, load_state(), the run again: the same logs and accumulators.  The saved state has
    `stepped` set, so the first tick after load_state reads the re-framed records before any plant step: they must
    be those of the uploaded plant records, not the last ones of the run before.  And a state saved mid-run."""
    K_SAVE = 17
    loop = _loop(variant, mounts=_tilt_mounts(), metrics=True)
    s0 = loop.state()
    assert s0["stepped"] and s0["k"] == 0
    logs, mid = [], None
    for how in ("run", "run", "resume"):
        loop.load_state(s0 if how != "resume" else mid)
        if how == "run":
            loop.log_info.fill_(float("nan"))
            loop.log_obs.fill_(float("nan"))
            loop.run(K_SAVE)
            mid = loop.state()
            loop.run(TICKS - K_SAVE)
        else:
            loop.log_info[K_SAVE:].fill_(float("nan"))
            loop.log_obs[K_SAVE:].fill_(float("nan"))
            loop.run(TICKS - K_SAVE)
        r = loop.results()
        r["obs_frame"] = loop.obs_frame.cpu().numpy()
        logs.append(r)
    # the re-framed start record differs from the run's last one, so a stale record would show
    assert not np.array_equal(logs[0]["obs"][0], logs[0]["obs"][TICKS])
    for how, other in zip(("run", "resume"), logs[1:]):
        FR._same_results(other, logs[0], (variant, how))
        assert np.array_equal(other["metrics"], logs[0]["metrics"], equal_nan=True), how
        assert np.array_equal(other["obs_frame"], logs[0]["obs_frame"]), how
    loop.close()


# -- 10. the sweep ---------------------------------------------------------------------------
def test_sweep_with_the_tilt_known():
    """run_sweep(device_loop=True, tilt_known=True): the flag comes back beside the summary, every whole-run summary
    is finite (from the logs and from the device accumulators) and telling the controllers the tilt matters."""
    from ffddp import fleet as FL

    kw = dict(scenarios=("flat", "tilted_10"), seeds=2, total_time=0.1, verbose=False, device_loop=True)
    plain = FL.run_sweep(**kw)
    out = FL.run_sweep(tilt_known=True, **kw)
    dev = FL.run_sweep(tilt_known=True, device_summary=True, **kw)
    both = FL.run_sweep(tilt_known=True, payload_spread=(0.5, 3.0), limit_spread=(0.5, 1.0), **kw)
    assert "tilt_known" not in plain and out["tilt_known"] is True and dev["tilt_known"] is True
    assert out["instances"] == 4 and out["ticks"] == 20 and both["tilt_known"] is True and "payload_mass" in both
    whole_run = ("rms_tangential_error", "rms_3d_error", "avg_abs_force_err", "max_fn", "unstable_ticks",
                 "neg_accepted_ticks", "solve_not_ok_ticks")  # 0.1 s has no contact phase: those keys are NaN
    for k in whole_run:
        assert np.all(np.isfinite(out["per_instance"][k])) and np.all(np.isfinite(dev["per_instance"][k])), k
        assert np.all(np.isfinite(both["per_instance"][k])), k
    e, p = out["per_instance"]["rms_3d_error"], plain["per_instance"]["rms_3d_error"]
    assert np.array_equal(e[:2], p[:2]) and np.all(e[2:] != p[2:])  # flat: unchanged; tilted_10: the mount matters
