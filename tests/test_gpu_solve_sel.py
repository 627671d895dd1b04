"""GPU: the selected-instance device solve (ffddp_solve_batch_sel_dev,
BatchedBoxFDDP.solve_dev(active=...)).

A selected instance's outputs are the unmasked solve's bits; of an unselected
instance the solve reads no warm-start row (they are NaN here) and writes no
output row (they keep a sentinel).  Cases: a mixed mask at B = 12, a batch the
library splits into slices (one slice unselected, one selected, the rest
mixed, the last one shorter), the all-zero and all-ones masks, the in-place
warm start, and a repeated call.  The unmasked reference is solved once per
(variant, B) and shared."""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ffddp import BatchedBoxFDDP  # noqa: E402

from helpers import make_batch, product_cfg  # noqa: E402

N = 8
MAXITER = 10
SENTINEL = -777.25
ISENT = -77
OUT = ("xs", "us", "K", "cost", "iters", "ok", "fn_pred", "stats")
# the smallest batch the library splits into slices (4 streams x 64) plus 2, so the last slice is shorter
B_SLICED = 4 * 64 + 2


def _fresh_outputs(B, nx):
    f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float64, device="cuda")  # noqa: E731
    return dict(xs=f(B, N + 1, nx), us=f(B, N, 7), K=f(B, N, 7, nx), cost=f(B),
                iters=torch.full((B,), ISENT, dtype=torch.int32, device="cuda"),
                ok=torch.full((B,), 77, dtype=torch.uint8, device="cuda"), fn_pred=f(B, 2),
                stats=torch.full((B, 10), ISENT, dtype=torch.int32, device="cuda"))


def _inputs(batch):
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k))).cuda()
         for k in ("x0", "node_ref", "inst_ref", "xs_init", "us_init")}
    t["surface"] = torch.from_numpy(np.ascontiguousarray(batch.surface, dtype=np.uint8)).cuda()
    return t


def _host(t):
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in OUT}


@functools.lru_cache(maxsize=None)
def _case(variant, B):
    """(solver, batch, the unmasked solve's outputs): computed once, never changed."""
    cfg = product_cfg(variant, N)
    batch = make_batch(variant, B, N, seed=1234 + B)
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    t = _inputs(batch)
    t.update(_fresh_outputs(B, cfg.nx))
    solver.solve_dev(t, maxiter=MAXITER)
    full = _host(t)
    for v in full.values():
        v.setflags(write=False)
    # precondition: the active list shrinks during the solve, and not for all instances at once
    assert len(np.unique(full["iters"])) > 1, full["iters"]
    assert np.any(full["iters"] < MAXITER), full["iters"]
    return solver, batch, full


def _mask(B, kind):
    rng = np.random.default_rng(B)
    if kind == "mixed":
        m = (rng.random(B) < 0.5).astype(np.uint8)
        m[0], m[1], m[B - 1] = 0, 1, 1  # both values whatever the draw
    elif kind == "slices":
        Bs = (B + 3) // 4  # the library's slice length
        m = (rng.random(B) < 0.5).astype(np.uint8)
        m[:Bs] = 0            # slice 0: nothing selected
        m[Bs:2 * Bs] = 1      # slice 1: everything selected
        m[2 * Bs], m[2 * Bs + 1], m[B - 1], m[B - 2] = 1, 0, 1, 0
    else:
        raise ValueError(kind)
    return m


def _masked_inputs(batch, mask):
    """Device inputs with the unselected instances' warm-start rows NaN."""
    t = _inputs(batch)
    off = torch.from_numpy(mask == 0).cuda()
    t["xs_init"][off] = float("nan")
    t["us_init"][off] = float("nan")
    return t


def _check(got, full, mask, sent):
    on = mask != 0
    for k in OUT:
        assert np.array_equal(got[k][on], full[k][on], equal_nan=True), k
        assert np.array_equal(got[k][~on], sent[k][~on], equal_nan=True), k


@pytest.mark.parametrize("variant", ["classical", "ff"])
@pytest.mark.parametrize("B,kind", [(12, "mixed"), (B_SLICED, "slices")])
def test_selected_rows_match_and_unselected_rows_untouched(variant, B, kind):
    solver, batch, full = _case(variant, B)
    mask = _mask(B, kind)
    assert 0 < mask.sum() < B
    t = _masked_inputs(batch, mask)
    t.update(_fresh_outputs(B, solver.nx))
    sent = _host(t)
    active = torch.from_numpy(mask).cuda()
    solver.solve_dev(t, maxiter=MAXITER, active=active)
    got = _host(t)
    _check(got, full, mask, sent)
    # the same masked call again: identical bits
    t.update(_fresh_outputs(B, solver.nx))
    solver.solve_dev(t, maxiter=MAXITER, active=active)
    again = _host(t)
    for k in OUT:
        assert np.array_equal(again[k], got[k], equal_nan=True), k


@pytest.mark.parametrize("variant", ["classical", "ff"])
@pytest.mark.parametrize("B", [12, B_SLICED])
def test_all_zero_and_all_ones_masks(variant, B):
    solver, batch, full = _case(variant, B)
    t = _masked_inputs(batch, np.zeros(B, np.uint8))
    t.update(_fresh_outputs(B, solver.nx))
    sent = _host(t)
    solver.solve_dev(t, maxiter=MAXITER, active=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    got = _host(t)
    for k in OUT:
        assert np.array_equal(got[k], sent[k]), k
    t = _inputs(batch)
    t.update(_fresh_outputs(B, solver.nx))
    solver.solve_dev(t, maxiter=MAXITER, active=torch.ones(B, dtype=torch.uint8, device="cuda"))
    got = _host(t)
    for k in OUT:
        assert np.array_equal(got[k], full[k], equal_nan=True), k


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_in_place_warm_start(variant):
    """xs_init is xs, us_init is us: selected rows solve in place, unselected rows keep their content."""
    B = 12
    solver, batch, full = _case(variant, B)
    mask = _mask(B, "mixed")
    t = _inputs(batch)
    t.update(_fresh_outputs(B, solver.nx))
    xs, us = t["xs_init"].clone(), t["us_init"].clone()
    off = torch.from_numpy(mask == 0).cuda()
    xs[off] = SENTINEL
    us[off] = SENTINEL
    t["xs"] = t["xs_init"] = xs
    t["us"] = t["us_init"] = us
    sent = _host(t)
    solver.solve_dev(t, maxiter=MAXITER, active=torch.from_numpy(mask).cuda())
    _check(_host(t), full, mask, sent)


def test_active_argument_is_validated():
    solver, batch, _ = _case("classical", 12)
    t = _inputs(batch)
    t.update(_fresh_outputs(12, solver.nx))
    with pytest.raises(ValueError):
        solver.solve_dev(t, maxiter=MAXITER, active=torch.ones(12, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        solver.solve_dev(t, maxiter=MAXITER, active=torch.ones(11, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        solver.solve_dev(t, maxiter=MAXITER, active=torch.ones(12, dtype=torch.uint8))
