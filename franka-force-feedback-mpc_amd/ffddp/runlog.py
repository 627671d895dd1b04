"""Run log and closed-loop summary metrics.

Mirrors the reference's on-disk run format so its plotting/evaluation
scripts read our runs unchanged:

* ``RunLogger``  — reference ``src/utils/logging.py:33-151``: one row per
  control tick via ``log(**fields)``, ``set_meta(**fields)``, and ``save()``
  writing ``<results>/logs/<stamp>_<name>/{data.npz, data.csv, meta.json}``.
    - data.npz: every key (sorted) stacked over rows; ndarray rows are
      stacked along axis 0, anything else becomes a float array, and what
      cannot be a float array an object array of JSON-able values.
    - data.csv: one column per scalar key, ``k[i]`` columns for 1-D arrays of
      at most 10 entries, and a JSON-able cell for anything larger.
    - meta.json: run_name, timestamp, notes + set_meta fields, indent 2.
* ``summary_metrics`` — the end-of-run statistics of
  ``run_classical.py:513-535`` (and the identical block of
  ``run_force_feedback.py``), returned as the dict ``set_meta`` receives.
* ``accumulate_metrics`` / ``metrics_from_accumulators`` — the same
  statistics for a fleet from per-instance running sums, maxima and counts,
  one record per instance folded in per tick: the numpy restatement of the
  device kernel behind ``ffddp_fleet_metrics_dev``, which lets
  a sweep of any length report its summary without keeping the series.
"""
from __future__ import annotations

import csv
import dataclasses
import json
import time
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np

from ._abi import FLEET_METRICS_FIELDS, FLEET_METRICS_W

__all__ = ["RunLogger", "jsonable", "summary_metrics", "metrics_accumulators", "accumulate_metrics",
           "metrics_from_accumulators"]

_F = {k: i for i, k in enumerate(FLEET_METRICS_FIELDS)}  # accumulator field -> row


def jsonable(x: Any) -> Any:
    """JSON-friendly copy of ``x`` (reference ``_to_jsonable``, logging.py:13-30):
    dataclasses -> dict, Path -> str, containers recursively, ndarray -> list,
    JSON scalars unchanged, anything else -> ``str(x)``."""
    if x is None or isinstance(x, (str, bool, int, float)):
        return x
    if dataclasses.is_dataclass(x) and not isinstance(x, type):
        return dataclasses.asdict(x)
    if isinstance(x, Path):
        return str(x)
    if isinstance(x, dict):
        return {str(k): jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    return str(x)


def _csv_kind(v: Any) -> int:
    """0: one scalar cell, 1: flattened short vector, 2: one JSON-able cell."""
    if v is None or np.isscalar(v):
        return 0
    if isinstance(v, np.ndarray) and v.ndim == 1 and v.size <= 10:
        return 1
    return 2


class RunLogger:
    """Per-tick run log with the reference's directory layout and file formats.

    ``RunLogger(run_name, results_dir="results", notes=None, overwrite=False)``
    creates ``results_dir/logs/<YYYYmmdd_HHMMSS>_<run_name>/`` immediately and
    raises ``FileExistsError`` if it exists and ``overwrite`` is False
    (logging.py:40-61).
    """

    def __init__(self, run_name: str, results_dir: Path | str = "results", notes: Optional[Dict[str, Any]] = None,
                 overwrite: bool = False):
        self.results_dir = Path(results_dir)
        self.logs_dir = self.results_dir / "logs"
        self.logs_dir.mkdir(parents=True, exist_ok=True)
        stamp = time.strftime("%Y%m%d_%H%M%S")
        self.run_dir = self.logs_dir / f"{stamp}_{run_name}"
        if self.run_dir.exists() and not overwrite:
            raise FileExistsError(f"Run dir exists: {self.run_dir}")
        self.run_dir.mkdir(parents=True, exist_ok=True)
        self._rows: list = []
        self.meta: Dict[str, Any] = {"run_name": run_name, "timestamp": stamp, "notes": jsonable(notes or {})}

    @property
    def path_npz(self) -> Path:
        return self.run_dir / "data.npz"

    @property
    def path_csv(self) -> Path:
        return self.run_dir / "data.csv"

    @property
    def path_meta(self) -> Path:
        return self.run_dir / "meta.json"

    def __len__(self) -> int:
        return len(self._rows)

    def log(self, **fields: Any) -> None:
        """Append one control tick (arrays are kept as given)."""
        self._rows.append(fields)

    def set_meta(self, **fields: Any) -> None:
        self.meta.update(jsonable(fields))

    # -- file writers ---------------------------------------------------------
    def _column(self, key: str):
        vals = [row.get(key) for row in self._rows]
        if isinstance(vals[0], np.ndarray):
            try:
                return np.stack(vals, axis=0)
            except (ValueError, TypeError):
                pass
        try:
            return np.array(vals, dtype=float)
        except (ValueError, TypeError):
            return np.array([jsonable(v) for v in vals], dtype=object)

    def save(self) -> None:
        """Write data.npz, data.csv and meta.json (no-op for an empty log)."""
        if not self._rows:
            return
        keys = sorted(self._rows[0].keys())
        np.savez_compressed(self.path_npz, **{k: self._column(k) for k in keys})

        first = self._rows[0]
        kinds = [_csv_kind(first.get(k)) for k in keys]
        header = []
        for k, kind in zip(keys, kinds):
            header.extend([f"{k}[{i}]" for i in range(first[k].size)] if kind == 1 else [k])
        with open(self.path_csv, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(header)
            for row in self._rows:
                cells = []
                for k in keys:
                    v = row.get(k)
                    kind = _csv_kind(v)
                    if kind == 0:
                        cells.append(v)
                    elif kind == 1:
                        cells.extend(v.tolist())
                    else:
                        cells.append(jsonable(v))
                w.writerow(cells)

        with open(self.path_meta, "w") as fh:
            json.dump(self.meta, fh, indent=2)


def _rms(a: np.ndarray) -> float:
    return float(np.sqrt(np.mean(a ** 2))) if a.size else float("nan")


def _force_ref(fn_des):
    """fn_des as the force-error terms take it: the scalar as a float (the
    arithmetic it always had), an array (one reference per sample or per
    instance) as float64."""
    return float(fn_des) if np.ndim(fn_des) == 0 else np.asarray(fn_des, dtype=float)


def summary_metrics(t, err_tan, err_3d, fn_meas, contact, fn_des, t_contact_phase: float) -> Dict[str, float]:
    """End-of-run statistics of the closed loop (run_classical.py:513-535).

    Inputs are the per-tick series the runner collects (``summary`` dict,
    run_classical.py:452-457); ``contact`` is 1.0 where fn_meas > 0.5 N.
    The contact phase is t >= t_contact_phase.  fn_des: the desired normal
    force, a scalar or one value per sample (a setpoint that varies over the
    run, trajectory.sample_force).
    """
    t = np.asarray(t, dtype=float)
    err_tan = np.asarray(err_tan, dtype=float)
    err_3d = np.asarray(err_3d, dtype=float)
    fn_meas = np.asarray(fn_meas, dtype=float)
    contact = np.asarray(contact, dtype=float)
    phase = t >= float(t_contact_phase)
    nan = float("nan")
    c_phase, fn_phase, et_phase = contact[phase], fn_meas[phase], err_tan[phase]
    return {
        "avg_abs_position_err": float(np.mean(np.abs(err_tan))) if err_tan.size else nan,
        "avg_abs_force_err": float(np.mean(np.abs(fn_meas - _force_ref(fn_des)))) if fn_meas.size else nan,
        "rms_tangential_error": _rms(err_tan),
        "rms_tangential_error_contact_phase": _rms(et_phase),
        "rms_3d_error": _rms(err_3d),
        "max_fn": float(np.max(fn_meas)) if fn_meas.size else nan,
        "contact_loss_pct": float((1.0 - np.mean(contact)) * 100.0) if contact.size else nan,
        "contact_loss_contact_phase_pct": float((1.0 - np.mean(c_phase)) * 100.0) if c_phase.size else nan,
        "fn_mean_contact_phase": float(np.mean(fn_phase)) if fn_phase.size else nan,
        "contact_phase_start_s": float(t_contact_phase),
    }


# -- the same statistics from running sums (include/ffddp.h: ffddp_fleet_metrics_dev) --------
def metrics_accumulators(B: int, ld: Optional[int] = None) -> np.ndarray:
    """Fresh accumulators (FLEET_METRICS_W, ld >= B), field-major: zero, max_fn at -inf."""
    acc = np.zeros((FLEET_METRICS_W, int(B) if ld is None else int(ld)))
    acc[_F["max_fn"]] = -np.inf
    return acc


def accumulate_metrics(acc: np.ndarray, obs, p_ref, ts, t_phase, fn_des, info=None, need=None,
                       plant_fail=None) -> np.ndarray:
    """One ffddp_fleet_metrics_dev call in numpy, term for term in the kernel's
    (and so ``summary_metrics``' callers') order: fold one plant record per
    instance into acc (FLEET_METRICS_W, ld >= B), in place.

    obs (B, >= 48): the records after a tick's command ([28..30] site position,
    [46] normal force, [47] contact flag); p_ref (3,) or (B, 3): the reference
    position at the series time ts (scalar or (B,)); t_phase (B,): the start of
    each instance's contact phase; fn_des: the desired normal force, a scalar or
    (B,), each instance's own at ts; info (B, FLEET_INFO_W) or None (the four
    solver counters are left); need (B,) or None (every instance solved);
    plant_fail (B,) or None.  Called once per tick the sums are sequential in
    tick order, as the kernel's are."""
    obs = np.asarray(obs, dtype=float)
    B = obs.shape[0]
    p_ref = np.broadcast_to(np.asarray(p_ref, dtype=float), (B, 3))
    ts = np.broadcast_to(np.asarray(ts, dtype=float), (B,))
    a = acc[:, :B]
    with np.errstate(invalid="ignore"):
        ex, ey, ez = (obs[:, 28 + i] - p_ref[:, i] for i in range(3))
        s2 = ex * ex + ey * ey
        et, e3 = np.sqrt(s2), np.sqrt(s2 + ez * ez)
        fn = obs[:, 46] * (obs[:, 47] > 0.5)
        contact = (fn > 0.5).astype(float)
        phase = ts >= np.asarray(t_phase, dtype=float)
        et2 = et * et
        a[_F["n"]] += 1.0
        a[_F["sum_tan2"]] += et2
        a[_F["sum_3d2"]] += e3 * e3
        a[_F["sum_abs_tan"]] += np.abs(et)
        a[_F["sum_abs_fn_err"]] += np.abs(fn - _force_ref(fn_des))
        a[_F["max_fn"]] = np.maximum(a[_F["max_fn"]], fn)  # propagates NaN, as np.max
        a[_F["sum_contact"]] += contact
        a[_F["max_err_3d"]] = np.maximum(a[_F["max_err_3d"]], e3)
        a[_F["n_phase"], phase] += 1.0
        a[_F["sum_tan2_phase"], phase] += et2[phase]
        a[_F["sum_contact_phase"], phase] += contact[phase]
        a[_F["sum_fn_phase"], phase] += fn[phase]
    if info is not None:
        info = np.asarray(info, dtype=float)
        a[_F["unstable_ticks"]] += info[:, 4] != 0
        a[_F["neg_accepted_ticks"]] += info[:, 7] > 0
        a[_F["not_ok_ticks"]] += info[:, 0] == 0
        a[_F["solved_ticks"]] += 1.0 if need is None else (np.asarray(need) != 0)
    if plant_fail is not None:
        a[_F["plant_fail"]] += np.asarray(plant_fail, dtype=float)
    return acc


def metrics_from_accumulators(acc) -> Dict[str, np.ndarray]:
    """``summary_metrics``' statistics, per instance, from the accumulators
    (FLEET_METRICS_W, B): every key the running sums determine -- the
    tracking, force and contact figures by ``summary_metrics``' formulas
    (sqrt(sum / n), (1 - mean) * 100), NaN where it gives NaN (no sample, or
    none in the contact phase) -- plus ``max_err_3d`` and the sweep's counters
    ``unstable_ticks``, ``neg_accepted_ticks``, ``solve_not_ok_ticks``,
    ``solved_ticks`` as counted."""
    acc = np.asarray(acc, dtype=float)
    f = {k: acc[i] for k, i in _F.items()}
    nan = np.full(acc.shape[1], np.nan)
    has, has_p = f["n"] > 0, f["n_phase"] > 0
    n, n_p = np.where(has, f["n"], 1.0), np.where(has_p, f["n_phase"], 1.0)
    with np.errstate(invalid="ignore"):
        return {
            "avg_abs_position_err": np.where(has, f["sum_abs_tan"] / n, nan),
            "avg_abs_force_err": np.where(has, f["sum_abs_fn_err"] / n, nan),
            "rms_tangential_error": np.where(has, np.sqrt(f["sum_tan2"] / n), nan),
            "rms_tangential_error_contact_phase": np.where(has_p, np.sqrt(f["sum_tan2_phase"] / n_p), nan),
            "rms_3d_error": np.where(has, np.sqrt(f["sum_3d2"] / n), nan),
            "max_fn": np.where(has, f["max_fn"], nan),
            "contact_loss_pct": np.where(has, (1.0 - f["sum_contact"] / n) * 100.0, nan),
            "contact_loss_contact_phase_pct": np.where(has_p, (1.0 - f["sum_contact_phase"] / n_p) * 100.0, nan),
            "fn_mean_contact_phase": np.where(has_p, f["sum_fn_phase"] / n_p, nan),
            "max_err_3d": np.where(has, f["max_err_3d"], nan),
            "unstable_ticks": f["unstable_ticks"].copy(),
            "neg_accepted_ticks": f["neg_accepted_ticks"].copy(),
            "solve_not_ok_ticks": f["not_ok_ticks"].copy(),
            "solved_ticks": f["solved_ticks"].copy(),
        }
