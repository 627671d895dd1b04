"""CPU: bench.py's --dump-outputs writer.  Every output of the solve is
written as float64 <name>.npy; the files stay inside the byte budget, an
array too large for its share is cut to a sorted, seeded sample of instances
whose indices stand beside it, non-finite entries are written as 0 and
marked in a file of their own, and the same call writes the same files."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _outputs(B=37, N=5, nx=14, nu=7):
    g = torch.Generator().manual_seed(3)
    f = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)  # noqa: E731
    return dict(xs=f(B, N + 1, nx), us=f(B, N, nu), K=f(B, N, nu, nx), cost=f(B), fn_pred=f(B, 2),
                iters=torch.arange(B, dtype=torch.int32), ok=(torch.arange(B) % 2).to(torch.uint8),
                stats=torch.zeros((B, 10), dtype=torch.int32))


def test_dump_whole_when_it_fits(tmp_path):
    T = _outputs()
    n = bench.dump_outputs(T, tmp_path / "d")
    assert set(n) == set(bench.DUMP_NAMES) and all(v == 37 for v in n.values())
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == sorted(f"{k}.npy" for k in bench.DUMP_NAMES)
    for k in bench.DUMP_NAMES:
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == tuple(T[k].shape)
        assert np.array_equal(a, T[k].numpy().astype(np.float64))


def test_dump_marks_non_finite_entries(tmp_path):
    T = _outputs()
    want = T["fn_pred"].numpy().copy()
    T["fn_pred"][3, :] = float("nan")
    T["fn_pred"][5, 0] = float("inf")
    T["fn_pred"][5, 1] = float("-inf")
    bench.dump_outputs(T, tmp_path)
    a, m = np.load(tmp_path / "fn_pred.npy"), np.load(tmp_path / "fn_pred_nonfinite.npy")
    want[3, :] = want[5, :] = 0.0
    assert np.array_equal(a, want)
    mark = np.zeros_like(want)
    mark[3, :], mark[5, 0], mark[5, 1] = 1.0, 2.0, -2.0
    assert m.dtype == np.float64 and np.array_equal(m, mark)
    assert not (tmp_path / "xs_nonfinite.npy").exists()


def test_dump_samples_what_exceeds_the_budget(tmp_path):
    T = _outputs()
    # K alone is 37 * 5 * 7 * 14 * 8 = 145 040 bytes; xs (24 864) and us (10 360) fit their shares
    budget = 70_000
    n = bench.dump_outputs(T, tmp_path / "a", budget=budget)
    bench.dump_outputs(T, tmp_path / "b", budget=budget)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted([f"{k}.npy" for k in bench.DUMP_NAMES] + ["K_rows.npy"])
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= budget
    rows = np.load(tmp_path / "a" / "K_rows.npy")
    assert rows.dtype == np.float64 and 1 <= rows.size == n["K"] < 37
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 37
    assert np.array_equal(np.load(tmp_path / "a" / "K.npy"), T["K"].numpy()[rows.astype(int)])
    assert all(n[k] == 37 for k in bench.DUMP_NAMES if k != "K")
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= budget + 128 * len(files)  # .npy headers
    for f in files:  # same arguments, same files
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
