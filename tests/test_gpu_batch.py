"""GPU: batch-size independence and the solve's edge cases, through the C-ABI.

* At the BASELINE size (B = 4096, 4 slices on 4 streams, staggered) and at an
  uneven size (B = 517), every instance's solution equals, BIT FOR BIT, the
  solution of the same instance solved in a small batch on one stream: the
  per-instance arithmetic does not depend on batch composition, slicing or
  stream overlap (a size-independent property at full size).  A spread of
  those instances is also checked against the oracle.
* is_feasible = True with a feasible warm start (rollout of the cold controls),
  maxiter = 0, B = 0, and B above max_batch.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from ffddp import BatchedBoxFDDP, FfddpError, _abi

from helpers import elem_err, log_parity, make_batch, oracle_cfg, oracle_problem, oracle_solve, product_cfg, rel_err
from oracle_pool import solve_many

pytestmark = pytest.mark.gpu


def _sub(batch, idx):
    import copy

    b = copy.copy(batch)
    for f in ("x0", "node_ref", "inst_ref", "surface", "xs_init", "us_init", "t0"):
        setattr(b, f, np.ascontiguousarray(getattr(batch, f)[idx]))
    return b


# regime -> (xs/us/cost, K, K element-wise) tolerance of the oracle spread:
# tracking as the parity cases (observed <= 1.3e-11,
# profiles/r02_parity_errors.jsonl); random x0 (unconverged 10-iteration
# solves from far-off starts) at its error budget: against an x87
# extended-precision solve of the same 8 instances the numpy oracle itself
# is 1.7e-7 off in us, 1.4e-8 in K (9.9e-7 element-wise), the C++ baseline
# 2.2e-7 / 3.7e-8 / 3.1e-6 (tools/ext_budget.py, profiles/r04_ext_budget.jsonl)
SPREAD_TOL = {"tracking": (1e-10, 3e-10, 5e-8), "random": (2e-7, 2e-7, 3e-5)}  # K_elem observed 3.7e-9 / 2.7e-6


@pytest.mark.parametrize("variant,B,regime", [("classical", 4096, "tracking"), ("classical", 517, "tracking"),
                                              ("classical", 1024, "random"), ("ff", 1024, "tracking")])
def test_full_batch_equals_small_batches(variant, B, regime, monkeypatch):
    """classical B = 4096: the metric's batch; classical B = 1024 random x0:
    BASELINE configs[1] (crocoddyl_classical.py:367 solve semantics; the
    SURVEY-literal draw around the neutral keyframe, panda_robot.xml:233),
    where the device-side line-search widening, the BoxQP stall exit and the
    four-slice schedule all switch on; FF B = 1024: BASELINE configs[2]."""
    N = 30
    cfg = product_cfg(variant, N)
    batch = make_batch(variant, B, N, seed=77, regime=regime)
    big = BatchedBoxFDDP(cfg, max_batch=B)
    big.solve(batch, maxiter=10)
    # one-stream reference solver for small batches
    monkeypatch.setenv("FFDDP_STREAMS", "1")
    small = BatchedBoxFDDP(cfg, max_batch=8)
    rng = np.random.default_rng(1)
    picks = np.unique(np.concatenate([[0, 1, B // 4 - 1, B // 4, B // 2, B - 1], rng.integers(0, B, 10)]))
    for i0 in range(0, len(picks), 8):
        idx = picks[i0:i0 + 8]
        small.solve(_sub(batch, idx), maxiter=10)
        for j, i in enumerate(idx):
            for name in ("xs", "us", "K", "cost", "iter", "ok", "fn_pred"):
                a, b = getattr(big, name)[i], getattr(small, name)[j]
                assert np.array_equal(a, b, equal_nan=True), (name, int(i))
            # the counters, except [5..7] (which line-search pass evaluated a
            # trial depends on the slice's active count, not on the instance)
            sa, sb = big.stats[i], small.stats[j]
            assert np.array_equal(sa[[0, 1, 2, 3, 4, 8, 9]], sb[[0, 1, 2, 3, 4, 8, 9]]), int(i)
    # a spread of them against the oracle
    sel = picks[::2]
    ref = solve_many(cfg, batch, sel)
    e = dict(xs=0.0, us=0.0, cost=0.0, K=0.0, K_elem=0.0)
    for i, r in zip(sel, ref):
        assert bool(big.ok[i]) == r["ok"] and int(big.iter[i]) == r["iter"]
        assert int(big.stats[i, 1]) == r["trials"] and int(big.stats[i, 2]) == r["reg_retries"]
        assert int(big.stats[i, 8]) == r["neg_branch"] and int(big.stats[i, 9]) == r["neg_accepted"]
        e["xs"] = max(e["xs"], rel_err(big.xs[i], r["xs"]))
        e["us"] = max(e["us"], rel_err(big.us[i], r["us"]))
        e["cost"] = max(e["cost"], rel_err(big.cost[i], r["cost"]))
        e["K"] = max(e["K"], rel_err(big.K[i], r["K"]))
        e["K_elem"] = max(e["K_elem"], elem_err(big.K[i], r["K"]))
    log_parity(f"batch/{variant}/{regime}/B{B}", n=len(sel), **e)
    tol, tol_k, tol_ke = SPREAD_TOL[regime]
    assert max(e["xs"], e["us"], e["cost"]) < tol and e["K"] < tol_k and e["K_elem"] < tol_ke, e
    assert np.all(np.isfinite(big.cost))
    if variant == "classical" and regime == "tracking":
        assert np.mean(big.ok) > 0.9
    big.close()
    small.close()


@pytest.mark.parametrize("B,regime", [(4096, "tracking"), (1024, "random")])
def test_ff_full_batch_equals_small_batches_bits(B, regime, monkeypatch):
    """FF bit-for-bit across batch shapes where the one-wave passes run
    (B = 4096: the throughput and latency variants beside the two-wave tail)
    and where BoxQP clamps controls (random x0: the gains' clamped set, phase
    E after a clamp, the two-wave pass's flag word).  Bits only: the oracle
    spread of FF is test_full_batch_equals_small_batches' FF case."""
    N = 30
    cfg = product_cfg("ff", N)
    batch = make_batch("ff", B, N, seed=78, regime=regime)
    big = BatchedBoxFDDP(cfg, max_batch=B)
    big.solve(batch, maxiter=10)
    monkeypatch.setenv("FFDDP_STREAMS", "1")
    small = BatchedBoxFDDP(cfg, max_batch=8)
    rng = np.random.default_rng(2)
    picks = np.unique(np.concatenate([[0, B // 4, B // 2, B - 1], rng.integers(0, B, 12)]))
    for i0 in range(0, len(picks), 8):
        idx = picks[i0:i0 + 8]
        small.solve(_sub(batch, idx), maxiter=10)
        for j, i in enumerate(idx):
            for name in ("xs", "us", "K", "cost", "iter", "ok", "fn_pred"):
                assert np.array_equal(getattr(big, name)[i], getattr(small, name)[j], equal_nan=True), (name, int(i))
            assert np.array_equal(big.stats[i][[0, 1, 2, 3, 4, 8, 9]], small.stats[j][[0, 1, 2, 3, 4, 8, 9]]), int(i)
    assert np.all(np.isfinite(big.cost))
    big.close()
    small.close()


def test_pinned_outputs_bit_identical():
    """Host entry point with page-locked caller arrays (DMA per slice, no
    staging) vs pageable ones (staging buffer, first touch during the solve,
    host copies as slices finish) vs the default recycled page-locked outputs:
    same bits.  Recycled outputs are fresh per call while the caller holds
    the previous ones, and reused once they are gone."""
    N, B = 30, 1030
    cfg = product_cfg("classical", N)
    batch = make_batch("classical", B, N, seed=78)
    a = BatchedBoxFDDP(cfg, max_batch=B, outputs="fresh")
    a.solve(batch, maxiter=10)
    p = BatchedBoxFDDP(cfg, max_batch=B, pinned_outputs=True)
    p.solve(batch, maxiter=10)
    r = BatchedBoxFDDP(cfg, max_batch=B)
    assert r.outputs == "recycled"
    r.solve(batch, maxiter=10)
    for name in ("xs", "us", "K", "cost", "iter", "ok", "fn_pred", "stats"):
        assert np.array_equal(getattr(a, name), getattr(p, name), equal_nan=True), name
        assert np.array_equal(getattr(a, name), getattr(r, name), equal_nan=True), name
    first = p.xs
    p.solve(batch.slice(slice(0, B)), maxiter=10)  # same buffers, overwritten in place
    assert p.xs is first
    # recycled: the held result keeps its block; a second solve gets another
    held_xs, held_K = r.xs, r.K
    r.solve(batch, maxiter=10)
    assert not np.shares_memory(held_xs, r.xs) and not np.shares_memory(held_K, r.K)
    assert np.array_equal(held_xs, r.xs) and np.array_equal(held_K, r.K)
    addr = held_xs.ctypes.data
    del held_xs, held_K
    r.solve(batch, maxiter=10)  # the released block comes back
    assert r.xs.ctypes.data == addr
    # page-locked inputs as well (per-slice DMA of the inputs, no staging)
    pin = p.pinned_batch(batch)
    p.solve(pin, maxiter=10)
    for name in ("xs", "us", "K", "cost", "iter", "ok", "fn_pred", "stats"):
        assert np.array_equal(getattr(a, name), getattr(p, name), equal_nan=True), name
    a.close()
    p.close()
    r.close()


def test_host_output_modes_bit_identical():
    """The host entry point's output paths at a multi-slice and a one-slice
    batch: fresh pageable outputs (staging buffer) and recycled page-locked
    outputs give the same bits as the device entry point."""
    import torch

    for B in (300, 100):
        N = 30
        cfg = product_cfg("classical", N)
        batch = make_batch("classical", B, N, seed=79 + B)
        dev = torch.device("cuda", 0)
        f64 = dict(dtype=torch.float64, device=dev)
        t = dict(x0=torch.tensor(batch.x0, **f64), node_ref=torch.tensor(batch.node_ref, **f64),
                 inst_ref=torch.tensor(batch.inst_ref, **f64),
                 surface=torch.tensor(batch.surface, dtype=torch.uint8, device=dev),
                 xs_init=torch.tensor(batch.xs_init, **f64), us_init=torch.tensor(batch.us_init, **f64),
                 xs=torch.zeros((B, N + 1, 14), **f64), us=torch.zeros((B, N, 7), **f64),
                 K=torch.zeros((B, N, 7, 14), **f64), cost=torch.zeros(B, **f64),
                 iters=torch.zeros(B, dtype=torch.int32, device=dev), ok=torch.zeros(B, dtype=torch.uint8, device=dev),
                 fn_pred=torch.zeros((B, 2), **f64), stats=torch.zeros((B, _abi.NSTATS), dtype=torch.int32, device=dev))
        d = BatchedBoxFDDP(cfg, max_batch=B)
        d.solve_dev(t, maxiter=10)
        torch.cuda.synchronize(dev)
        ref = {k: t[k].cpu().numpy() for k in ("xs", "us", "K", "cost", "stats")}
        d.close()
        for outputs, env in (("fresh", None), ("recycled", None)):
            s = BatchedBoxFDDP(cfg, max_batch=B, outputs=outputs)
            s.solve(batch, maxiter=10)
            for k, v in ref.items():
                assert np.array_equal(getattr(s, k), v, equal_nan=True), (B, outputs, env, k)
            s.close()


def test_feasible_warm_start_matches_oracle():
    """is_feasible = True: xs_init is the rollout of us_init (gravity torques)
    through the dynamics, so the guess has no gaps (SolverFDDP feasible start)."""
    from oracle import fddp, ocp

    N, B = 20, 4
    cfg = product_cfg("classical", N)
    batch = make_batch("classical", B, N, seed=91, surface=1)
    ocfg = oracle_cfg(cfg)
    xs0 = np.zeros((B, N + 1, 14))
    for i in range(B):
        prob = oracle_problem(batch, i, N)
        x = batch.x0[i].copy()
        xs0[i, 0] = x
        for t in range(N):
            x = ocp.running_eval(ocfg, prob, t, x, batch.us_init[i, t], False)["xnext"]
            xs0[i, t + 1] = x
    us0 = batch.us_init.copy()
    s1 = BatchedBoxFDDP(cfg, max_batch=B)
    ok = s1.solve(batch, maxiter=4, is_feasible=True, xs_init=xs0, us_init=us0)
    for i in range(B):
        so = fddp.SolverBoxFDDP(ocfg, oracle_problem(batch, i, N))
        ok_o = so.solve(xs0[i], us0[i], 4, True)
        assert bool(ok[i]) == bool(ok_o) and int(s1.iter[i]) == int(so.iter)
        assert rel_err(s1.xs[i], so.xs) < 1e-6 and rel_err(s1.us[i], so.us) < 1e-6
        assert rel_err(s1.cost[i], so.cost) < 1e-6
    s1.close()


def test_maxiter_zero_and_sizes():
    from oracle import fddp

    N, B = 10, 3
    cfg = product_cfg("classical", N)
    batch = make_batch("classical", B, N, seed=5)
    s = BatchedBoxFDDP(cfg, max_batch=B)
    ok = s.solve(batch, maxiter=0)
    for i in range(B):
        so = fddp.SolverBoxFDDP(oracle_cfg(cfg), oracle_problem(batch, i, N))
        ok_o = so.solve(batch.xs_init[i], batch.us_init[i], 0, False)
        assert bool(ok[i]) == bool(ok_o)
        np.testing.assert_array_equal(s.xs[i], batch.xs_init[i])
        np.testing.assert_array_equal(s.us[i], batch.us_init[i])
    with pytest.raises(FfddpError):
        s.solve(make_batch("classical", B + 1, N, seed=6))
    empty = make_batch("classical", 1, N, seed=6)
    for f in ("x0", "node_ref", "inst_ref", "surface", "xs_init", "us_init", "t0"):
        setattr(empty, f, getattr(empty, f)[:0])
    assert s.solve(empty).shape == (0,)
    s.close()
