"""Host side of the plant's per-instance link inertial parameters: the header
symbol and its binding, the input handling of BatchedPlant.set_link_models
that needs no handle (plant.plant_link_rows), and run_sweep's
plant_payload_spread / payload_known argument checks and draw.  No device."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp import plant as PL
from ffddp import robot as R
from ffddp.config import link_model_rows

ROOT = Path(__file__).resolve().parents[1]
SYMBOL = "ffddp_plant_set_instance_links"
PADDING = np.array([16 * j + k for j in range(7) for k in (13, 14, 15)] + list(range(112, 128)))


def test_header_declares_the_symbol_and_abi_binds_it():
    text = (ROOT / "include" / "ffddp.h").read_text()
    assert re.search(r"\bint %s\(ffddp_plant\* h, int n, const double\* link_rows\);" % SYMBOL, text)
    assert SYMBOL in _abi.SYMBOLS
    fn = getattr(_abi.load(), SYMBOL)
    assert fn.argtypes is not None and len(fn.argtypes) == 3
    # a null handle is refused before anything touches a device
    assert fn(None, 1, _abi.dptr(link_model_rows([None]))) == -1
    assert fn(None, 0, None) == -1


def test_link_rows_of_models_and_arrays():
    models = [None, R.LinkModel().with_payload(1.5), R.LinkModel().scaled(1.1)]
    rows = PL.plant_link_rows(models)
    assert rows.shape == (3, _abi.LINK_W) and rows.dtype == np.float64
    assert np.array_equal(rows, link_model_rows(models))  # through config.link_model_rows
    assert np.array_equal(rows[0], link_model_rows([R.LinkModel()])[0])  # None: the nominal model
    assert np.array_equal(PL.plant_link_rows(rows), rows)  # the array form passes through
    # the padding entries are not looked at
    nan_pad = rows.copy()
    nan_pad[:, PADDING] = np.nan
    assert PADDING.size == 128 - 91
    assert np.array_equal(PL.plant_link_rows(nan_pad), nan_pad, equal_nan=True)


def test_link_rows_refusals_are_value_errors():
    for bad in (0.0, -1.0, np.nan, np.inf):
        mass = R.MASS.copy()
        mass[4] = bad
        with pytest.raises(ValueError, match="finite"):
            PL.plant_link_rows([None, R.LinkModel(mass=mass)])
        rows = link_model_rows([None, None])
        rows[1, 16 * 4] = bad
        with pytest.raises(ValueError, match="finite"):
            PL.plant_link_rows(rows)
    for bad in (np.nan, -np.inf):
        com, I = R.COM.copy(), R.INERTIA.copy()
        com[6, 2] = bad
        I[0, 1, 2] = bad
        for m in (R.LinkModel(com=com), R.LinkModel(inertia=I)):
            with pytest.raises(ValueError, match="finite"):
                PL.plant_link_rows([m])
        for e in (16 * 6 + 3, 16 * 0 + 4 + 5):
            rows = link_model_rows([None])
            rows[0, e] = bad
            with pytest.raises(ValueError, match="finite"):
                PL.plant_link_rows(rows)
    for shape in ((2, 127), (128,), (0, 128), (2, 7, 16)):
        with pytest.raises(ValueError, match="expected"):
            PL.plant_link_rows(np.ones(shape))
    for seq in ([], [R.LinkModel(), 3.0], ["nominal"]):
        with pytest.raises(ValueError, match="LinkModel"):
            PL.plant_link_rows(seq)


def test_run_sweep_argument_checks():
    for bad in ((-0.5, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0), (1.0,), (0.0, 1.0, 2.0), 3.0):
        with pytest.raises(ValueError, match="plant_payload_spread"):
            FL.run_sweep(plant_payload_spread=bad)
        with pytest.raises(ValueError, match="plant_payload_spread"):
            FL.run_sweep(plant_payload_spread=bad, device_loop=True)
    with pytest.raises(NotImplementedError, match="payload_known"):
        FL.run_sweep(plant_payload_spread=(0.0, 3.0), payload_known=True)
    with pytest.raises(ValueError, match="payload_spread"):
        FL.run_sweep(plant_payload_spread=(0.0, 3.0), payload_known=True, payload_spread=(0.0, 3.0), device_loop=True)
    with pytest.raises(ValueError, match="payload_spread"):
        FL.run_sweep(plant_payload_spread=(0.0, 3.0), payload_known=True, payload_spread=(0.0, 3.0))
    with pytest.raises(ValueError, match="plant_payload_spread"):
        FL.run_sweep(payload_known=True, device_loop=True)
    with pytest.raises(ValueError, match="flag"):
        FL.run_sweep(plant_payload_spread=(0.0, 3.0), payload_known=2, device_loop=True)


def test_the_draw_has_its_own_generator():
    seed = np.array([0, 1, 2, 7, 255, 2 ** 31 + 5])
    m = FL.sweep_plant_payload_masses(seed, (0.5, 3.0))
    want = np.array([0.5 + 2.5 * np.random.default_rng([int(s), 8]).uniform(0.0, 1.0) for s in seed])
    assert np.array_equal(m, want)
    assert np.all((m >= 0.5) & (m <= 3.0)) and len(set(m)) == len(seed)
    # another stream than payload_spread's ([seed, 7]): the two axes are drawn independently
    ctrl = FL.sweep_payload_masses(seed, (0.5, 3.0))
    assert not np.any(m == ctrl)
    assert abs(np.corrcoef(FL.sweep_plant_payload_masses(np.arange(400), (0.0, 1.0)),
                           FL.sweep_payload_masses(np.arange(400), (0.0, 1.0)))[0, 1]) < 0.2
    # a degenerate range is that mass for all; the models are the nominal arm with a point payload at the EE offset
    assert np.array_equal(FL.sweep_plant_payload_masses(seed, (2.0, 2.0)), np.full(len(seed), 2.0))
    models = FL.payload_models(m)
    for mod, mass in zip(models, m):
        ref = R.LinkModel().with_payload(float(mass), R.EE_P)
        assert np.array_equal(mod.mass, ref.mass) and np.array_equal(mod.com, ref.com)
        assert np.array_equal(mod.inertia, ref.inertia) and mod.mass[6] == R.MASS[6] + mass


def test_fleet_loop_refuses_a_wrong_plant_model_list_before_any_device_work():
    from ffddp.controller import classical_benchmark_config
    from ffddp.fleet_loop import DeviceFleetLoop
    from ffddp.trajectory import benchmark_traj

    traj, meta = benchmark_traj(np.array([-0.3, 0.0, 0.6]))
    cfg = classical_benchmark_config(0.005, meta["z_contact"], horizon=4)
    q0 = np.tile(R.Q_NEUTRAL, (3, 1))
    for bad in ([R.LinkModel()] * 2, [R.LinkModel(), None, 1.0]):
        with pytest.raises(ValueError, match="plant_link_models"):
            DeviceFleetLoop("classical", 3, traj, cfg, q0, plant_link_models=bad)
