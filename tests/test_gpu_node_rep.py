"""GPU: the first node stage of a uniform cold start (k_node_rep).

An instance whose running nodes start from one repeated (x, u) point -- the
reference's own cold start, xs_init = [x0] * (N + 1), us_init = [g(q0)] * N --
has its first calc + calcDiff evaluated at node 0 and the terminal node only;
nodes 1..N-1 are built from node 0's record and the terms the node references
enter.  The results must be those of the full evaluation, bit for bit:
FFDDP_NODE_REP=0 (read at handle creation) switches the replication off.

A batch here mixes, with both surface flags:
  0, 1  uniform cold starts (0: surface, its target point constant along the
        horizon in the constrained axes, so the contact dynamics repeat too);
  2     one state component of one interior node moved by one ulp: not uniform;
  3     only us_init[N-1] changed: not uniform;
  4     only xs_init[N] changed: the terminal node is not part of the test, so
        still uniform (a surface instance; its target point moves along the
        horizon as the workload made it);
  5     a surface instance whose target height changes at node 1: the contact
        dynamics of the nodes differ, so it takes the full evaluation.
"""
from __future__ import annotations

import numpy as np
import pytest

from ffddp import BatchedBoxFDDP

from helpers import make_batch, product_cfg

pytestmark = pytest.mark.gpu

OUT = ("xs", "us", "K", "cost", "iter", "ok", "fn_pred", "stats")
SWITCH = "FFDDP_NODE_REP"


def _cfg(contact, N):
    """contact "point3d_cone": point3d with the friction cone on (ClassicalMPCConfig's defaults, as test_gpu_parity)."""
    c = product_cfg("classical", N, contact.replace("_cone", ""))
    if contact.endswith("_cone"):
        c.w_friction_cone, c.mu = 2.0e2, 0.6
    return c


def _mixed_batch(contact, N, B=6, seed=41):
    b = make_batch("classical", B, N, seed=seed)
    b.surface[:] = np.array([1, 0, 1, 0, 1, 1], np.uint8)[:B]
    b.node_ref[0, :, :3] = b.node_ref[0, 0, :3]  # constant target point: the contact dynamics repeat
    t_in = N - 1 if N > 2 else 1                 # an interior node (1..N-1)
    b.xs_init[2, t_in, 9] = np.nextafter(b.xs_init[2, t_in, 9], np.inf)
    b.us_init[3, N - 1, 4] += 0.25
    b.xs_init[4, N, :7] += 0.01
    b.node_ref[5, :, :3] = b.node_ref[5, 0, :3]
    b.node_ref[5, 1, 2] += 1e-3
    return b


def _solver(cfg, B, monkeypatch, switch):
    with monkeypatch.context() as m:
        if switch is None:
            m.delenv(SWITCH, raising=False)
        else:
            m.setenv(SWITCH, switch)  # read by ffddp_create
        return BatchedBoxFDDP(cfg, max_batch=B)


def _outputs(s):
    return {k: np.array(getattr(s, k)) for k in OUT}


def _solve(cfg, b, monkeypatch, switch, maxiter):
    s = _solver(cfg, int(b.x0.shape[0]), monkeypatch, switch)
    s.solve(b, maxiter=maxiter, is_feasible=False)
    out = _outputs(s)
    s.close()
    return out


def _assert_same(a, c, tag):
    B = a["xs"].shape[0]
    for name in OUT:
        for i in range(B):  # each instance on its own
            assert np.array_equal(a[name][i], c[name][i], equal_nan=True), (tag, name, i)


@pytest.mark.parametrize("maxiter", [1, 4])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("contact", ["normal_1d", "point3d", "point3d_cone"])
def test_switch_on_equals_off(contact, N, maxiter, monkeypatch):
    """maxiter 1: the records of iteration 0 reach K directly."""
    cfg = _cfg(contact, N)
    b = _mixed_batch(contact, N)
    on = _solve(cfg, b, monkeypatch, None, maxiter)
    off = _solve(cfg, b, monkeypatch, "0", maxiter)
    assert np.all(np.isfinite(on["K"])) and np.any(on["K"] != 0.0)
    _assert_same(on, off, (contact, N, maxiter))


@pytest.mark.parametrize("contact", ["normal_1d", "point3d", "point3d_cone"])
def test_instances_do_not_depend_on_the_batch(contact, monkeypatch):
    """The same 6 instances solved alone (B = 1 each) give the bits they have in the batch."""
    N, B = 5, 6
    cfg = _cfg(contact, N)
    b = _mixed_batch(contact, N, B)
    whole = _solve(cfg, b, monkeypatch, None, 4)
    one = _solver(cfg, 1, monkeypatch, None)
    for i in range(B):
        sub = type(b)(*(np.ascontiguousarray(a[i:i + 1]) for a in (b.x0, b.node_ref, b.inst_ref, b.surface, b.xs_init,
                                                                  b.us_init, b.t0)))
        one.solve(sub, maxiter=4, is_feasible=False)
        alone = _outputs(one)
        for name in OUT:
            assert np.array_equal(alone[name][0], whole[name][i], equal_nan=True), (contact, name, i)
    one.close()


@pytest.mark.parametrize("contact,surf", [("normal_1d", 1), ("normal_1d", 0), ("point3d", 1), ("point3d", 0)])
def test_cold_start_matches_oracle(contact, surf):
    """test_gpu_parity's checks and tolerances (_check_solves: identical discrete path, xs / us / cost / K within
    its tables) at N = 5, B = 8, on cold starts whose target point is constant along the horizon (so the surface
    instances replicate as well).

    Through test_gpu_force_ref._check_against_oracle with table_shape=False: the point3d surface case is first held
    to parity's tight tolerances against the oracle with gains by Cholesky solves.  Parity's table for the
    explicit-inverse oracle is that oracle's own rounding error measured at N = 12, B = 4; at this shape it is larger
    (the library sat 7.2e-9 from it in xs against the table's 6e-9 while within 1e-10 of the solve form), so there
    the bound is the triangle inequality's: the tight tolerance plus the distance between the two oracle solves,
    measured in the test without the code under test, never below the table's."""
    import test_gpu_force_ref as FRT

    N, B = 5, 8
    cfg = product_cfg("classical", N, contact)
    b = make_batch("classical", B, N, seed=21 + surf, surface=surf)
    b.node_ref[::2, :, :3] = b.node_ref[::2, :1, :3]  # every other instance; the rest as the workload made them
    solver = BatchedBoxFDDP(cfg, max_batch=B)
    solver.solve(b, maxiter=10, is_feasible=False)
    got = dict(ok=np.array(solver.ok), iters=np.array(solver.iter), stats=np.array(solver.stats), xs=np.array(solver.xs),
               us=np.array(solver.us), K=np.array(solver.K), cost=np.array(solver.cost))
    FRT._check_against_oracle(f"node_rep/solve/{contact}/surf{surf}", "classical", contact, surf, 0, cfg, b, got,
                              [cfg.fn_des] * B, table_shape=False)
    solver.close()


def test_force_feedback_falls_back(monkeypatch):
    """The force-feedback kernels have no replication: the switch changes nothing."""
    N, B = 3, 4
    cfg = product_cfg("ff", N)
    b = make_batch("ff", B, N, seed=43)
    on = _solve(cfg, b, monkeypatch, None, 4)
    off = _solve(cfg, b, monkeypatch, "0", 4)
    _assert_same(on, off, "ff")


def test_force_reference_falls_back(monkeypatch):
    """Neither have the kernels of a solve with a per-node force reference."""
    import test_gpu_force_ref as FRT

    N, B = 3, 4
    cfg = product_cfg("classical", N)
    b = make_batch("classical", B, N, seed=44, surface=1)
    f = np.random.default_rng(5).uniform(5.0, 40.0, (B, N + 1))
    got = {}
    for switch in (None, "0"):
        s = _solver(cfg, B, monkeypatch, switch)
        t = FRT._inputs(b)
        t.update(FRT._fresh_outputs(B, s.N, s.nx))
        s.solve_dev(t, maxiter=4, force_ref=FRT._dev(f))
        got[switch] = FRT._host(t)
        s.close()
    for name, a in got[None].items():
        assert np.array_equal(a, got["0"][name], equal_nan=True), name


def test_plan_includes_the_replication(monkeypatch):
    """A captured solve plan replays the stream-launched solve, bit for bit, on uniform cold starts."""
    N, B = 3, 4
    cfg = product_cfg("classical", N)
    b = make_batch("classical", B, N, seed=45)
    b.surface[:] = np.array([1, 0, 1, 0], np.uint8)
    b.node_ref[:, :, :3] = b.node_ref[:, :1, :3]
    ref = _solver(cfg, B, monkeypatch, None)
    s = _solver(cfg, B, monkeypatch, None)
    plan = s.plan(B, maxiter=4)
    ref.solve(b, maxiter=4)
    plan.fill(b)
    plan.run()
    for name in OUT:
        assert np.array_equal(getattr(ref, name), getattr(plan, name), equal_nan=True), name
    off = _solve(cfg, b, monkeypatch, "0", 4)
    for name in OUT:
        assert np.array_equal(getattr(plan, name), off[name], equal_nan=True), name
    plan.close()
    s.close()
    ref.close()
