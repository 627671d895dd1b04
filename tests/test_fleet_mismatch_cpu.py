"""Per-instance plant physics and uncertainty profiles, host side (no device
here): the mixed BatchedUncertaintyInjector against per-instance scalar
injectors and against a numpy restatement of the per-row kernels' slot rule,
homogeneous configs through the same path, the new structs and constants
against the header, the new entry points' null-handle codes, the physics rows'
validation and run_sweep's refusals."""
import ctypes
import dataclasses
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp import plant as PL
from ffddp import uncertainty as U
from test_fleet_ff_cpu import _obs

ROOT = Path(__file__).resolve().parents[1]
DT = 0.005  # the sweep's control period
MIXED_DELAYS = ((0, 0), (2, 1), (0, 3), (4, 0))  # (observation, command) in ticks of DT


def mixed_configs(delays=MIXED_DELAYS, seed0=40):
    """One config per delay pair: its delays written as 1 kHz cycles / seconds, its own sigmas and a / b ranges."""
    return [U.UncertaintyProfileConfig(
        a_min=0.9 + 0.01 * i, a_max=1.02 + 0.02 * i, b_min=-0.1 - 0.05 * i, b_max=0.1 + 0.03 * i,
        sigma_q=5.0e-4 * (1 + i), sigma_dq=2.0e-3 / (1 + i), sigma_tau=5.0e-2 * (1 + 0.5 * i),
        delta_obs_cycles=5 * do, delta_cmd_s=dc * DT, seed=seed0 + 7 * i) for i, (do, dc) in enumerate(delays)]


class RowsRestatement:
    """k_fleet_inject_obs / k_fleet_inject_cmd with per-row delays and sigmas
    (csrc/ffddp_inject.hpp, ffddp_fleet_inject_rows) in numpy: rings as deep
    as the largest delay; instance b with row r writes the observation ring
    at (k - 1) mod (d_obs[r] + 1) and reads it at k mod (d_obs[r] + 1) (at
    k = 0 slots 0..d_obs[r] take the first observation), writes the command
    ring at k mod (d_cmd[r] + 1) and reads it at (k + 1) mod (d_cmd[r] + 1).
    `touched` marks every ring slot written."""

    def __init__(self, row, a, b, d_obs, d_cmd, sigma, lpf):
        self.row, self.a, self.b = np.asarray(row), np.asarray(a, float), np.asarray(b, float)
        self.d_obs, self.d_cmd, self.sigma = np.asarray(d_obs), np.asarray(d_cmd), np.asarray(sigma, float)
        self.B, self.lpf = len(self.row), float(lpf)
        self.obs_ring = np.zeros((int(self.d_obs.max()) + 1, self.B, 14))
        self.cmd_ring = np.zeros((int(self.d_cmd.max()) + 1, self.B, 7))
        self.touched = (np.zeros(self.obs_ring.shape[:2], bool), np.zeros(self.cmd_ring.shape[:2], bool))
        self.tau_hat_filt = np.zeros((self.B, 7))
        self.z_cmd = np.zeros((self.B, 7))

    def obs(self, k, z, q, v, tau_filt=None):
        qv = np.concatenate([q, v], 1)
        qv_ctrl, tau_hat, tau_ctrl = qv.copy(), np.zeros((self.B, 7)), np.zeros((self.B, 7))
        if tau_filt is not None:
            tau_hat, tau_ctrl = tau_filt.copy(), tau_filt.copy()
        for b in np.flatnonzero(self.row >= 0):
            r = self.row[b]
            no, nc, sg = int(self.d_obs[r]) + 1, int(self.d_cmd[r]) + 1, self.sigma[r]
            slots = range(no) if k == 0 else [(k - 1) % no]
            for s in slots:
                self.obs_ring[s, b] = qv[b]
                self.touched[0][s, b] = True
            old = self.obs_ring[k % no, b]
            qv_ctrl[b, :7] = old[:7] + (0.0 + sg[0] * z[r, 0:7])
            qv_ctrl[b, 7:] = old[7:] + (0.0 + sg[1] * z[r, 7:14])
            th = self.a[r] * self.cmd_ring[k % nc, b] + self.b[r] + (0.0 + sg[2] * z[r, 14:21])
            self.tau_hat_filt[b] = (1.0 - self.lpf) * self.tau_hat_filt[b] + self.lpf * th
            self.z_cmd[b] = z[r, 21:28]
            tau_hat[b], tau_ctrl[b] = th, self.tau_hat_filt[b]
        return qv_ctrl, tau_hat, tau_ctrl

    def cmd(self, k, tau_cmd, tau_app):
        out = tau_app.copy()
        for b in np.flatnonzero(self.row >= 0):
            r = self.row[b]
            nc = int(self.d_cmd[r]) + 1
            self.cmd_ring[k % nc, b] = tau_cmd[b]
            self.touched[1][k % nc, b] = True
            out[b] = self.a[r] * self.cmd_ring[(k + 1) % nc, b] + self.b[r] + (0.0 + self.sigma[r, 2] * self.z_cmd[b])
        return out


def test_mixed_host_injector_equals_scalar_injectors_and_slot_rule():
    """300 ticks: across the host class's 256-tick chunk of normals."""
    cfgs, steps, B = mixed_configs(), 300, len(MIXED_DELAYS)
    assert [U.delay_steps(c, DT) for c in cfgs] == list(MIXED_DELAYS)
    bat = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs)
    scal = [U.ScenarioUncertaintyInjector(dt=DT, nu=7, config=c) for c in cfgs]
    assert np.array_equal(bat.delay, np.array(MIXED_DELAYS)) and bat.delay.dtype.kind == "i"
    assert np.array_equal(bat.sigma, np.array([(c.sigma_q, c.sigma_dq, c.sigma_tau) for c in cfgs]))
    assert (bat.obs_delay_steps, bat.cmd_delay_steps) == (4, 3) and bat.sig is None  # the ring depths; no one sigma
    assert [(s.obs_delay_steps, s.cmd_delay_steps) for s in scal] == list(MIXED_DELAYS)
    a, b, z = U.predraw(cfgs, steps)  # already per config: every row is its own Generator's stream and a / b range
    assert np.array_equal(a, bat.a) and np.array_equal(b, bat.b)
    assert np.array_equal(a, [s.a for s in scal]) and np.array_equal(b, [s.b for s in scal])
    ga, gb, _ = U.draw_gain_bias(cfgs)
    assert np.array_equal(ga, a) and np.array_equal(gb, b)
    ker = RowsRestatement(np.arange(B), a, b, bat.delay[:, 0], bat.delay[:, 1], bat.sigma, 0.2)
    rng = np.random.default_rng(3)
    for k in range(steps):
        q, dq, tau = rng.normal(size=(B, 7)), rng.normal(size=(B, 7)), rng.normal(size=(B, 7)) * 10
        qb, dqb = bat.observation_for_controller(q, dq)
        th, thf = bat.tau_hat.copy(), bat.tau_hat_filt.copy()
        app = bat.command_for_plant(tau)
        qv, kth, kthf = ker.obs(k, z[k], q, dq)
        assert np.array_equal(qv[:, :7], qb) and np.array_equal(qv[:, 7:], dqb), k
        assert np.array_equal(kth, th) and np.array_equal(kthf, thf), k
        assert np.array_equal(ker.cmd(k, tau, np.zeros((B, 7))), app), k
        for i, s in enumerate(scal):
            d = s.observation_for_controller(_obs(q[i], dq[i]))
            assert np.array_equal(qb[i], d.q) and np.array_equal(dqb[i], d.dq), (k, i)
            assert np.array_equal(th[i], d.tau_meas_act) and np.array_equal(thf[i], d.tau_meas_act_filt), (k, i)
            assert np.array_equal(app[i], s.command_for_plant(tau[i])), (k, i)
    # every instance used the slots 0..d of its ring column, and no other
    for t, d in zip(ker.touched, (bat.delay[:, 0], bat.delay[:, 1])):
        assert np.array_equal(t, np.arange(t.shape[0])[:, None] <= d[None, :])


@pytest.mark.parametrize("delays", [(2, 1), (0, 0)])
def test_homogeneous_configs_keep_scalar_attributes_and_bits(delays):
    seeds, steps = [15, 1500003, 7], 300
    kw = dict(delta_obs_cycles=10, delta_cmd_s=5.0e-3) if delays == (2, 1) else {}
    cfgs = [U.UncertaintyProfileConfig(seed=s, **kw) for s in seeds]
    bat = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs)
    c0 = cfgs[0]
    assert (bat.obs_delay_steps, bat.cmd_delay_steps) == delays == U.delay_steps(c0, DT)
    assert bat.sig == (c0.sigma_q, c0.sigma_dq, c0.sigma_tau) and isinstance(bat.sig, tuple)
    assert np.array_equal(bat.delay, np.tile(delays, (3, 1))) and np.array_equal(bat.sigma, np.tile(bat.sig, (3, 1)))
    # the same seeds with the per-instance arrays given explicitly (the configs' own values unused)
    other = [dataclasses.replace(c, sigma_q=1.0, sigma_dq=2.0, sigma_tau=3.0, delta_obs_cycles=55, delta_cmd_s=0.05)
             for c in cfgs]
    exp = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=other, delay=np.tile(delays, (3, 1)),
                                       sigma=np.tile(bat.sig, (3, 1)))
    assert (exp.obs_delay_steps, exp.cmd_delay_steps) == delays and exp.sig == bat.sig
    sc = U.ScenarioUncertaintyInjector(dt=DT, nu=7, config=cfgs[1])
    rng = np.random.default_rng(5)
    for k in range(steps):
        q, dq, tau = rng.normal(size=(3, 7)), rng.normal(size=(3, 7)), rng.normal(size=(3, 7)) * 10
        qa, dqa = bat.observation_for_controller(q, dq)
        qe, dqe = exp.observation_for_controller(q, dq)
        assert np.array_equal(qa, qe) and np.array_equal(dqa, dqe), k
        assert np.array_equal(bat.tau_hat, exp.tau_hat) and np.array_equal(bat.tau_hat_filt, exp.tau_hat_filt), k
        d = sc.observation_for_controller(_obs(q[1], dq[1]))
        assert np.array_equal(qa[1], d.q) and np.array_equal(bat.tau_hat_filt[1], d.tau_meas_act_filt), k
        app = bat.command_for_plant(tau)
        assert np.array_equal(app, exp.command_for_plant(tau)) and np.array_equal(app[1], sc.command_for_plant(tau[1])), k
    with pytest.raises(ValueError, match="delay"):
        U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs, delay=[(0, 0), (-1, 0), (0, 0)])


def test_structs_and_constants_match_header():
    fr = [n for n, _ in _abi.FleetInjectRows._fields_]
    names = ("W", "ARMATURE", "DAMPING", "R_TOOL", "MARGIN", "SOLREF", "SOLIMP")
    offs = "".join(f'  printf("%zu ", offsetof(ffddp_fleet_inject_rows, {n}));\n' for n in fr)
    rows = "".join(f'  printf("%d ", FFDDP_PLANT_ROW_{n});\n' for n in names)
    pp = "".join(f'  printf("%zu ", (offsetof(ffddp_plant_params, {n}) - offsetof(ffddp_plant_params, armature)) / 8);\n'
                 for n in ("armature", "damping", "r_tool", "margin", "solref", "solimp", "site_R"))
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ffddp.h"\nint main(void) {\n'
           '  printf("%zu ", sizeof(ffddp_fleet_inject_rows));\n' + offs + rows + pp + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(src)
        exe = Path(d) / "t"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(exe)], check=True)
        vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_abi.FleetInjectRows) and vals[1:4] == [getattr(_abi.FleetInjectRows, n).offset for n in fr]
    want = [_abi.PLANT_ROW_W, _abi.PLANT_ROW_ARMATURE, _abi.PLANT_ROW_DAMPING, _abi.PLANT_ROW_R_TOOL,
            _abi.PLANT_ROW_MARGIN, _abi.PLANT_ROW_SOLREF, _abi.PLANT_ROW_SOLIMP]
    assert vals[4:11] == want == [23, 0, 7, 14, 15, 16, 18]
    # a row is the struct's physics fields in the struct's order, packed: site_R starts where a row ends
    assert vals[11:] == want[1:] + [_abi.PLANT_ROW_W]
    hdr = (ROOT / "include" / "ffddp.h").read_text()
    body = hdr.split("typedef struct ffddp_fleet_inject_rows {")[1].split("} ffddp_fleet_inject_rows;")[0]
    decl = [ln.split(";")[0] for ln in body.strip().splitlines()[1:] if ";" in ln]
    assert [d.replace("*", " ").split()[-1] for d in decl] == fr
    new = {"ffddp_plant_set_instance_params", "ffddp_fleet_inject_obs_rows_dev", "ffddp_fleet_inject_cmd_rows_dev"}
    assert new <= set(_abi.SYMBOLS) and all(f"int {n}(" in hdr for n in new)
    # the defaults are the scene's constants, the handle's struct
    p = PL.plant_params(0.001, 5)
    row = PL.PlantPhysics().row()
    flat = list(p.armature) + list(p.damping) + [p.r_tool, p.margin] + list(p.solref) + list(p.solimp)
    assert row.shape == (_abi.PLANT_ROW_W,) and np.array_equal(row, flat)


def test_new_entry_points_null_handle_errors():
    lib = _abi.load()
    inj, rows = _abi.FleetInject(), _abi.FleetInjectRows()
    rows.sigma = 8  # any member set: the per-row path
    for r in (None, ctypes.byref(rows)):
        assert lib.ffddp_fleet_inject_obs_rows_dev(None, 1, ctypes.byref(inj), 0, None, None, None, 7, None, None, None,
                                                   None, r, None) == -1
        assert lib.ffddp_fleet_inject_cmd_rows_dev(None, 1, ctypes.byref(inj), 0, None, None, r, None) == -1
    good = PL.plant_rows([PL.PlantPhysics()])
    assert lib.ffddp_plant_set_instance_params(None, 1, _abi.dptr(good)) == -1
    assert lib.ffddp_plant_set_instance_params(None, 0, None) == -1  # FFDDP_E_INVALID


BAD_ROWS = (("armature", 3, -0.1), ("damping", 9, -1.0e-9), ("r_tool", 14, 0.0), ("r_tool", 14, -0.03),
            ("solref", 16, 0.0), ("solref", 17, -1.0), ("d0", 18, 0.0), ("d0", 18, 1.0), ("dmax", 19, 1.0),
            ("dmax < d0 = 0.8", 19, 0.75), ("mid", 21, 0.0), ("mid", 21, 1.0), ("power", 22, 0.5), ("non-finite", 15, np.nan),
            ("non-finite", 20, np.inf))


def test_plant_rows_validation():
    seq = [PL.PlantPhysics(), PL.PlantPhysics(armature=np.linspace(0.05, 0.2, 7), damping=2.0, r_tool=0.031,
                                              margin=0.0, solref=(0.01, 0.7), solimp=(0.8, 0.8, 0.0, 0.3, 1.0))]
    rows = PL.plant_rows(seq)
    assert rows.shape == (2, 23) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows[1, 0:7], np.linspace(0.05, 0.2, 7)) and np.all(rows[1, 7:14] == 2.0)
    assert list(rows[1, 14:]) == [0.031, 0.0, 0.01, 0.7, 0.8, 0.8, 0.0, 0.3, 1.0]
    assert np.array_equal(PL.check_plant_rows(rows), rows)
    for what, col, val in BAD_ROWS:
        bad = rows.copy()
        bad[1, col] = val
        with pytest.raises(ValueError, match="plant rows"):
            PL.check_plant_rows(bad)
        with pytest.raises(ValueError, match="plant rows"):
            PL.plant_rows([PL.PlantPhysics(), PL.PlantPhysics(
                armature=bad[1, 0:7], damping=bad[1, 7:14], r_tool=bad[1, 14], margin=bad[1, 15], solref=bad[1, 16:18],
                solimp=bad[1, 18:23])])
    for shape in ((23,), (2, 22), (0, 23)):
        with pytest.raises(ValueError, match="plant rows"):
            PL.check_plant_rows(np.ones(shape))
    with pytest.raises(ValueError, match="PlantPhysics"):
        PL.plant_rows([])
    with pytest.raises(ValueError, match="PlantPhysics"):
        PL.plant_rows([PL.PlantPhysics(), None])


def test_run_sweep_spread_refusals_and_draws():
    """All refused before any device object is made, so this runs without a device."""
    kw = dict(scenarios=("flat", "actuation_uncertainty"), seeds=1, total_time=0.1, verbose=False)
    for bad in ((0.5,), (0.5, 0.95), (-0.1, 0.5), (0.5, 0.5, 0.5)):
        with pytest.raises(ValueError, match="plant_spread"):
            FL.run_sweep(plant_spread=bad, **kw)
        with pytest.raises(ValueError, match="plant_spread"):
            FL.run_sweep(plant_spread=bad, device_loop=True, device_noise="numpy", **kw)
    for bad in ((0.5,), (1.0, 3), (-0.1, 3), (0.5, 17), (0.5, -1), (0.5, 2.5), (0.5, True), (0.5, 3, 1)):
        with pytest.raises(ValueError, match="uncertainty_spread"):
            FL.run_sweep(uncertainty_spread=bad, **kw)
    # the draws: generators of their own, the profile written so that delay_steps returns the drawn ticks
    seed = [17, 1500003]
    ph = FL.sweep_plant_physics(seed, (0.5, 0.9))
    for s, p in zip(seed, ph):
        u = np.random.default_rng([s, 2]).uniform(-1.0, 1.0, 2)
        assert p.solref == (0.02 * (1.0 + 0.5 * u[0]), 1.0) and p.damping == 1.0 * (1.0 + 0.9 * u[1])
        assert p.solref[0] >= 2.0 * 0.001 and p.armature == PL.JOINT_ARMATURE and p.solimp == PL.PlantPhysics().solimp
    assert FL.sweep_uncertainty_config("flat", 17, DT, (0.5, 3)) is None
    base = U.config_for_scenario("actuation_uncertainty", seed=17)
    assert FL.sweep_uncertainty_config("actuation_uncertainty", 17, DT, None) == base
    seen = set()
    for s in range(40):
        c = FL.sweep_uncertainty_config("actuation_uncertainty", s, DT, (0.5, 16))
        g = np.random.default_rng([s, 3])
        f = 1.0 + 0.5 * g.uniform(-1.0, 1.0)
        d = tuple(int(x) for x in g.integers(0, 17, 2))
        assert U.delay_steps(c, DT) == d and c.seed == s
        assert (c.sigma_q, c.sigma_dq, c.sigma_tau) == (5.0e-4 * f, 2.0e-3 * f, 5.0e-2 * f)
        assert (c.a_min, c.a_max, c.b_min, c.b_max) == (base.a_min, base.a_max, base.b_min, base.b_max)
        seen.update(d)
    assert seen == set(range(17))
