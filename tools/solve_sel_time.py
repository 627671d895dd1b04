#!/usr/bin/env python3
"""What an unselected instance of ffddp_solve_batch_sel_dev still costs: the
masked solve of B instances with every second one selected, against the
unmasked solves of B and of B / 2 instances (device entry point, one stream,
events around `reps` back-to-back solves after a warm-up), and the per-kernel
profile (ffddp_profile_enable) of the three.  Prints one JSON line.

  python tools/solve_sel_time.py [--batch 1024] [--horizon 30] [--variant classical|ff]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
import ffddp_path  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--variant", choices=("classical", "ff"), default="classical")
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ffddp import BatchedBoxFDDP, _abi
    from helpers import make_batch, product_cfg

    B, N = a.batch, a.horizon
    cfg = product_cfg(a.variant, N)
    batch = make_batch(a.variant, B, N, seed=77)
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    nx = cfg.nx
    stream = torch.cuda.current_stream().cuda_stream

    def tensors(sl):
        t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)[sl])).cuda()
             for k in ("x0", "node_ref", "inst_ref", "xs_init", "us_init")}
        n = t["x0"].shape[0]
        t["surface"] = torch.from_numpy(np.ascontiguousarray(batch.surface[sl], dtype=np.uint8)).cuda()
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda")  # noqa: E731
        t.update(xs=z(n, N + 1, nx), us=z(n, N, 7), K=z(n, N, 7, nx), cost=z(n), iters=z(n, dtype=torch.int32),
                 ok=z(n, dtype=torch.uint8), fn_pred=z(n, 2), stats=z(n, _abi.NSTATS, dtype=torch.int32))
        return t

    mask = torch.zeros(B, dtype=torch.uint8, device="cuda")
    mask[::2] = 1
    full, half = tensors(slice(None)), tensors(slice(0, B, 2))
    sides = {"masked_half_of_B": (full, mask), "full_B": (full, None), "full_half_B": (half, None)}
    out = {"variant": a.variant, "B": B, "horizon": N, "maxiter": a.maxiter, "reps": a.reps, "ms_per_solve": {},
           "profile_ms_per_solve": {}}
    for _ in range(2):  # the second round is the recorded one
        for name, (t, m) in sides.items():
            for _ in range(a.warmup):
                solver.solve_dev(t, maxiter=a.maxiter, stream=stream, active=m)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                solver.solve_dev(t, maxiter=a.maxiter, stream=stream, active=m)
            e1.record()
            torch.cuda.synchronize()
            out["ms_per_solve"][name] = e0.elapsed_time(e1) / a.reps
    # selected instances of the masked solve equal the half batch solved alone (the solver is batch-independent)
    solver.solve_dev(full, maxiter=a.maxiter, stream=stream, active=mask)
    solver.solve_dev(half, maxiter=a.maxiter, stream=stream)
    torch.cuda.synchronize()
    out["masked_equals_half_batch_bits"] = bool(torch.equal(full["us"][::2], half["us"]) and torch.equal(full["K"][::2], half["K"]))
    solver.profile(True)
    for name, (t, m) in sides.items():
        solver.profile_read(reset=True)
        for _ in range(a.reps):
            solver.solve_dev(t, maxiter=a.maxiter, stream=stream, active=m)
        torch.cuda.synchronize()
        out["profile_ms_per_solve"][name] = {k: ms / a.reps for k, (ms, _) in solver.profile_read(reset=True).items()}
    solver.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
