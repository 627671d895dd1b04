"""GPU: the fleet tick kernels (ffddp_fleet_warm_start_dev, ffddp_fleet_keep_dev)
against a numpy restatement of their rules (include/ffddp.h).  Both are pure
data movement plus a finiteness test, so every comparison is exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp.config import classical_preset, ff_preset  # noqa: E402

SENTINEL = -777.25

# (variant, N, B): N = 2 makes the min(k+1, N-1) clamp hit at once; B = 65
# crosses a wave of instances; ff has nx = 21 (odd strides, an instance's base
# only 8-byte aligned) and B = 130 is more than two waves of instances
SHAPES = [("classical", 2, 3), ("classical", 5, 65), ("ff", 3, 130)]


def _inputs(nx, N, B, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s)  # noqa: E731
    d = dict(x0=f(B, nx), u_cold=f(B, 7), valid=(rng.random(B) < 0.5).astype(np.uint8),
             xs=f(B, N + 1, nx), us=f(B, N, 7), K=f(B, N, 7, nx), cost=f(B),
             iters=rng.integers(0, 20, B).astype(np.int32), ok=(rng.random(B) < 0.7).astype(np.uint8),
             fn_pred=f(B, 2), stats=rng.integers(0, 50, (B, _abi.NSTATS)).astype(np.int32),
             keep_xs=f(B, N + 1, nx), keep_us=f(B, N, 7), keep_K=f(B, N, 7, nx))
    d["valid"][0], d["valid"][B - 1] = 1, 0  # both branches whatever the draw
    d["us"][0, 0, 3] = np.nan                # not kept
    d["us"][1, 0, 6] = np.inf                # not kept
    d["us"][2, 1, 2] = np.nan                # only knot 0 is tested: still kept
    d["cost"][B - 1] = np.nan
    d["fn_pred"][B // 2] = np.nan
    return d


def _warm_start_ref(d, N):
    """xs_init[b][0] = x0; k >= 1: valid ? keep_xs[b][k] : x0;
    us_init[b][k] = valid ? keep_us[b][min(k+1, N-1)] : u_cold."""
    B, nx = d["x0"].shape
    xs_init, us_init = np.zeros((B, N + 1, nx)), np.zeros((B, N, 7))
    for b in range(B):
        for k in range(N + 1):
            xs_init[b, k] = d["keep_xs"][b, k] if (d["valid"][b] and k >= 1) else d["x0"][b]
        for k in range(N):
            us_init[b, k] = d["keep_us"][b, min(k + 1, N - 1)] if d["valid"][b] else d["u_cold"][b]
    return xs_init, us_init


def _keep_ref(d, kx, ku, kK):
    """fin = us[b][0] all finite; kept arrays replaced iff fin; the record from the kept arrays."""
    B, nx = d["x0"].shape
    kx, ku, kK = kx.copy(), ku.copy(), kK.copy()
    fin = np.all(np.isfinite(d["us"][:, 0]), axis=1)
    for b in range(B):
        if fin[b]:
            kx[b], ku[b], kK[b] = d["xs"][b], d["us"][b], d["K"][b]
    fields = dict(fin=fin.astype(float)[:, None], us0=ku[:, 0], xs0=kx[:, 0], xs1=kx[:, 1],
                  K0=kK[:, 0].reshape(B, 7 * nx), cost=d["cost"][:, None], iters=d["iters"].astype(float)[:, None],
                  ok=d["ok"].astype(float)[:, None], stats9=d["stats"][:, 9].astype(float)[:, None],
                  fn0=d["fn_pred"][:, 0:1], fn1=d["fn_pred"][:, 1:2])
    return fin, kx, ku, kK, fields


@pytest.mark.parametrize("variant,N,B", SHAPES)
def test_fleet_tick_kernels_match_numpy(variant, N, B):
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    W = _abi.fleet_first_w(nx)
    assert W == 14 + 9 * nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    d = _inputs(nx, N, B, seed=N * 1000 + B)
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    t["xs_init"] = torch.full((B, N + 1, nx), SENTINEL, dtype=torch.float64, device="cuda")
    t["us_init"] = torch.full((B, N, 7), SENTINEL, dtype=torch.float64, device="cuda")
    t["first"] = torch.full((B, W), SENTINEL, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    solver.fleet_warm_start_dev(t, stream=stream)
    xs_ref, us_ref = _warm_start_ref(d, N)
    assert np.array_equal(t["xs_init"].cpu().numpy(), xs_ref, equal_nan=True)
    assert np.array_equal(t["us_init"].cpu().numpy(), us_ref, equal_nan=True)
    # inputs untouched
    assert np.array_equal(t["keep_xs"].cpu().numpy(), d["keep_xs"]) and np.array_equal(t["x0"].cpu().numpy(), d["x0"])

    # keep: the kept arrays start as a sentinel, so an instance that is not kept must still hold it
    for k in ("keep_xs", "keep_us", "keep_K"):
        t[k].fill_(SENTINEL)
    sent = {k: np.full(d[k].shape, SENTINEL) for k in ("keep_xs", "keep_us", "keep_K")}
    solver.fleet_keep_dev(t, stream=stream)
    fin, kx, ku, kK, fields = _keep_ref(d, sent["keep_xs"], sent["keep_us"], sent["keep_K"])
    assert not fin[0] and not fin[1] and fin[2] and fin.sum() == B - 2
    got = {k: t[k].cpu().numpy() for k in ("keep_xs", "keep_us", "keep_K")}
    assert np.array_equal(got["keep_xs"], kx, equal_nan=True)
    assert np.array_equal(got["keep_us"], ku, equal_nan=True)
    assert np.array_equal(got["keep_K"], kK, equal_nan=True)
    for b in (0, 1):
        assert all(np.all(got[k][b] == SENTINEL) for k in got), b
    first = t["first"].cpu().numpy()
    o = 0
    for name, ref in fields.items():  # the record's order (include/ffddp.h)
        w = ref.shape[1]
        assert np.array_equal(first[:, o:o + w], ref, equal_nan=True), name
        o += w
    assert o == W
    # the solution the kernel read is untouched
    assert np.array_equal(t["K"].cpu().numpy(), d["K"]) and np.array_equal(t["us"].cpu().numpy(), d["us"], equal_nan=True)
    solver.close()


def test_fleet_tick_error_codes():
    N, B = 2, 3
    solver = BatchedBoxFDDP(classical_preset(N), max_batch=B, device=0)
    lib, h = solver._lib, solver._h
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(int(buf.data_ptr()))
    ws = lambda B_, args: lib.ffddp_fleet_warm_start_dev(h, B_, *args, None)  # noqa: E731
    kp = lambda B_, args: lib.ffddp_fleet_keep_dev(h, B_, *args, None)  # noqa: E731
    assert ws(B + 1, [p] * 7) == -4 and kp(B + 1, [p] * 12) == -4  # FFDDP_E_CAPACITY
    assert ws(0, [p] * 7) == -1 and kp(-1, [p] * 12) == -1  # FFDDP_E_INVALID
    for i in range(7):
        assert ws(B, [p] * i + [None] + [p] * (6 - i)) == -1, i
    for i in range(12):
        assert kp(B, [p] * i + [None] + [p] * (11 - i)) == -1, i
    assert lib.ffddp_fleet_warm_start_dev(None, B, *([p] * 7), None) == -1
    assert lib.ffddp_fleet_keep_dev(None, B, *([p] * 12), None) == -1
    solver.close()
