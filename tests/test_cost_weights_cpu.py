"""Host side of the per-instance cost weights: the row builder, the index
constants against the header, run_sweep's draws and argument checks, and the
sweep tool's option.  No device."""
from __future__ import annotations

import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp.config import COST_WEIGHT_NAMES, classical_preset, cost_weight_row, ff_preset
from ffddp.fleet_loop import cost_weight_rows

ROOT = Path(__file__).resolve().parents[1]


def test_index_constants_equal_the_header():
    text = (ROOT / "include" / "ffddp.h").read_text()
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FFDDP_(COST_W|CW_\w+) (\d+)", text)}
    assert macros.pop("COST_W") == _abi.COST_W
    joint0 = macros.pop("CW_JOINT0")
    assert {"w_" + k[3:].lower(): v for k, v in macros.items()} == _abi.COST_INDEX
    # one entry per scalar cost weight of the configuration, in two blocks inside the row
    assert set(_abi.COST_INDEX) == set(COST_WEIGHT_NAMES) and len(COST_WEIGHT_NAMES) == 18
    assert len(set(_abi.COST_INDEX.values())) == 18 and max(_abi.COST_INDEX.values()) < _abi.COST_W
    fields = {n for n, _ in _abi.OcpConfig._fields_}
    assert set(COST_WEIGHT_NAMES) <= fields
    assert set(COST_WEIGHT_NAMES) == {n for n in fields if n.startswith("w_") and n != "w_wdamp_weights"}
    ee = [v for v in _abi.COST_INDEX.values() if v < joint0]
    jt = [v for v in _abi.COST_INDEX.values() if v >= joint0]
    assert sorted(ee) == list(range(10)) and sorted(jt) == list(range(joint0, joint0 + 8))


@pytest.mark.parametrize("variant", ["classical", "ff"])
@pytest.mark.parametrize("contact", ["normal_1d", "point3d"])
def test_row_repeats_the_configuration(variant, contact):
    cfg = (ff_preset if variant == "ff" else classical_preset)(12, contact)
    cfg.w_friction_cone = 2.0e2
    row = cost_weight_row(cfg)
    assert row.shape == (_abi.COST_W,) and row.dtype == np.float64
    c = cfg.to_struct()
    for name in COST_WEIGHT_NAMES:
        want = float(getattr(c, name))
        if name == "w_friction_cone" and contact != "point3d":
            want = 0.0  # built for point3d only
        if name in ("w_w", "w_w_soft_limits", "w_y") and variant != "ff":
            want = 0.0
        assert row[_abi.COST_INDEX[name]] == want, name
    used = sorted(_abi.COST_INDEX.values())
    assert not row[[i for i in range(_abi.COST_W) if i not in used]].any()  # the padding
    # the variant argument overrides the configuration's
    assert np.array_equal(cost_weight_row(cfg, variant), row)
    if variant == "ff":
        cl = cost_weight_row(cfg, "classical")
        assert cl[_abi.COST_INDEX["w_y"]] == 0.0 and cl[_abi.COST_INDEX["w_fn"]] == row[_abi.COST_INDEX["w_fn"]]
    # overrides
    over = cost_weight_row(cfg, w_fn=40.0, w_tau=0.0)
    assert over[_abi.COST_INDEX["w_fn"]] == 40.0 and over[_abi.COST_INDEX["w_tau"]] == 0.0
    rest = [i for i in range(_abi.COST_W) if i not in (_abi.COST_INDEX["w_fn"], _abi.COST_INDEX["w_tau"])]
    assert np.array_equal(over[rest], row[rest])


def test_row_builder_errors():
    cfg = classical_preset(12)
    with pytest.raises(ValueError, match="unknown cost weight"):
        cost_weight_row(cfg, w_nope=1.0)
    with pytest.raises(ValueError, match="unknown cost weight"):
        cost_weight_row(cfg, fn_des=10.0)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            cost_weight_row(cfg, w_fn=bad)
    cfg.w_vz = 0.0
    for absent in ("w_vz", "w_friction_cone", "w_y", "w_w", "w_w_soft_limits"):
        with pytest.raises(ValueError, match="does not build"):
            cost_weight_row(cfg, **{absent: 3.0})
        assert cost_weight_row(cfg, **{absent: 0.0})[_abi.COST_INDEX[absent]] == 0.0
    with pytest.raises(ValueError, match="variant"):
        cost_weight_row(cfg, "lqr")


def test_loop_rows_from_array_and_overrides():
    cfg = ff_preset(8)
    base = cost_weight_row(cfg)
    rows = cost_weight_rows(cfg, "ff", [None, {"w_fn": 7.5}, {}], 3)
    assert rows.shape == (3, _abi.COST_W) and np.array_equal(rows[0], base) and np.array_equal(rows[2], base)
    assert rows[1, _abi.COST_INDEX["w_fn"]] == 7.5
    arr = cost_weight_rows(cfg, "ff", rows, 3)
    assert np.array_equal(arr, rows) and arr is not rows
    for bad in (rows[:2], rows[:, :24], np.where(rows == 7.5, np.nan, rows), -rows):
        with pytest.raises(ValueError, match="cost_weights"):
            cost_weight_rows(cfg, "ff", bad, 3)
    with pytest.raises(ValueError, match="cost_weights"):
        cost_weight_rows(cfg, "ff", [None, None], 3)
    with pytest.raises(ValueError, match="cost_weights"):
        cost_weight_rows(cfg, "ff", [None, 5.0, None], 3)
    with pytest.raises(ValueError, match="unknown cost weight"):
        cost_weight_rows(cfg, "ff", [None, {"w_nope": 1.0}, None], 3)


def test_sweep_draws_are_reproducible_and_move_no_other_draw():
    names, tilt, scale, seed = FL._sweep_instances(("flat", "tilted_10"), 3)
    spread = {"w_tau": (2.0e-4, 3.2e-3), "w_fn": (7.0, 112.0)}
    w = FL.sweep_cost_weights(seed, spread)
    assert list(w) == ["w_fn", "w_tau"]  # the names' sorted order, whatever the dict's
    for b, s in enumerate(seed):
        u = np.random.default_rng([int(s), 5]).uniform(-1.0, 1.0, 2)
        assert w["w_fn"][b] == 7.0 * (112.0 / 7.0) ** (0.5 * (1.0 + u[0]))
        assert w["w_tau"][b] == 2.0e-4 * (3.2e-3 / 2.0e-4) ** (0.5 * (1.0 + u[1]))
    assert np.all((w["w_fn"] >= 7.0) & (w["w_fn"] <= 112.0)) and np.all((w["w_tau"] >= 2.0e-4) & (w["w_tau"] <= 3.2e-3))
    assert len(set(w["w_fn"][:3])) == 3
    again = FL.sweep_cost_weights(seed, dict(reversed(list(spread.items()))))
    assert all(np.array_equal(again[k], w[k]) for k in w)
    # one name alone takes the first uniform of the same generator
    assert np.array_equal(FL.sweep_cost_weights(seed, {"w_fn": (7.0, 112.0)})["w_fn"], w["w_fn"])
    # a generator of its own: the sweep's other per-instance draws are those of their own generators, as before
    phys = FL.sweep_plant_physics(seed, (0.5, 0.5))
    FL.sweep_cost_weights(seed, spread)
    assert FL.sweep_plant_physics(seed, (0.5, 0.5)) == phys
    for s in seed:
        for stream in (1, 2, 3, 4):
            a = np.random.default_rng([int(s), stream]).uniform(-1.0, 1.0, 2)
            assert not np.array_equal(a, np.random.default_rng([int(s), 5]).uniform(-1.0, 1.0, 2))
    # lo == hi is a constant
    assert np.all(FL.sweep_cost_weights(seed, {"w_fn": (28.0, 28.0)})["w_fn"] == 28.0)


def test_run_sweep_weight_arguments():
    kw = dict(seeds=1, scenarios=("flat",), verbose=False)
    with pytest.raises(NotImplementedError, match="device_loop"):
        FL.run_sweep(weight_spread={"w_fn": (7.0, 112.0)}, **kw)
    for bad in ({"w_nope": (1.0, 2.0)}, {"w_fn": (0.0, 2.0)}, {"w_fn": (3.0, 2.0)}, {"w_fn": (1.0,)}, {"w_fn": (1.0, np.inf)},
                {}, [("w_fn", 1.0, 2.0)]):
        with pytest.raises(ValueError, match="weight_spread"):
            FL.run_sweep(weight_spread=bad, device_loop=True, **kw)


def _sweep_tool():
    spec = importlib.util.spec_from_file_location("sweep_c4_tool", ROOT / "tools" / "sweep_c4.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sweep_tool_weight_spread_option(capsys):
    tool = _sweep_tool()
    ap = tool.build_parser()
    a = ap.parse_args(["--device-loop", "1", "--weight-spread", "w_fn", "7", "112", "--weight-spread", "w_tau", "2e-4", "3.2e-3"])
    assert tool.weight_spread_arg(a.weight_spread) == {"w_fn": (7.0, 112.0), "w_tau": (2.0e-4, 3.2e-3)}
    assert FL.check_weight_spread(tool.weight_spread_arg(a.weight_spread)) == {"w_fn": (7.0, 112.0), "w_tau": (2.0e-4, 3.2e-3)}
    none = ap.parse_args([])
    assert none.weight_spread is None and tool.weight_spread_arg(none.weight_spread) is None
    with pytest.raises(ValueError, match="twice"):
        tool.weight_spread_arg([["w_fn", "1", "2"], ["w_fn", "2", "3"]])
    with pytest.raises(ValueError):
        tool.weight_spread_arg([["w_fn", "lo", "2"]])
    with pytest.raises(SystemExit):
        ap.parse_args(["--weight-spread", "w_fn", "7"])
    capsys.readouterr()
