"""The device uncertainty injector's host side (no device here): the struct's
ctypes layout against the header, the entry points' null-handle codes,
uncertainty.predraw run through a numpy restatement of the two kernels against
the host injectors, uncertainty.philox_normals against numpy's Philox and its
moments, and the refusals."""
import ctypes
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from ffddp import _abi
from ffddp import fleet as FL
from ffddp import uncertainty as U
from test_fleet_ff_cpu import _obs

ROOT = Path(__file__).resolve().parents[1]
DT = 0.005  # the sweep's control period
DELAYED = dict(delta_obs_cycles=10, delta_cmd_s=5.0e-3)  # delays (2, 1) at DT; the default config gives (0, 0)
PHILOX_SEEDS = (0, 1, 2 ** 32 + 3, 2 ** 63 + 1)
PHILOX_TICKS = (0, 1, 799)


class KernelRestatement:
    """k_fleet_inject_obs / k_fleet_inject_cmd (csrc/ffddp_inject.hpp) in numpy
    for a fleet of B instances, `row` as the kernels' (-1: no injector): the
    ring slots from the tick number, the sums in the kernels' order."""

    def __init__(self, row, a, b, d_obs, d_cmd, sigma, lpf):
        self.row, self.a, self.b = np.asarray(row), np.asarray(a, float), np.asarray(b, float)
        self.B, self.d_obs, self.d_cmd, self.sig, self.lpf = len(self.row), int(d_obs), int(d_cmd), sigma, float(lpf)
        self.obs_ring = np.zeros((self.d_obs + 1, self.B, 14))
        self.cmd_ring = np.zeros((self.d_cmd + 1, self.B, 7))
        self.tau_hat_filt = np.zeros((self.B, 7))
        self.z_cmd = np.zeros((self.B, 7))

    def obs(self, k, z, q, v, tau_filt=None):
        """-> qv_ctrl (B, 14), tau_hat, tau_ctrl (B, 7); z (rows, 28)"""
        no, nc = self.d_obs + 1, self.d_cmd + 1
        qv = np.concatenate([q, v], 1)
        qv_ctrl, tau_hat, tau_ctrl = qv.copy(), np.zeros((self.B, 7)), np.zeros((self.B, 7))
        if tau_filt is not None:
            tau_hat, tau_ctrl = tau_filt.copy(), tau_filt.copy()
        on = self.row >= 0
        r = self.row[on]
        if k == 0:
            self.obs_ring[:, on] = qv[on]
        else:
            self.obs_ring[(k - 1) % no, on] = qv[on]
        old = self.obs_ring[k % no, on]
        zz = z[r]
        qv_ctrl[on, :7] = old[:, :7] + (0.0 + self.sig[0] * zz[:, 0:7])
        qv_ctrl[on, 7:] = old[:, 7:] + (0.0 + self.sig[1] * zz[:, 7:14])
        th = self.a[r, None] * self.cmd_ring[k % nc, on] + self.b[r, None] + (0.0 + self.sig[2] * zz[:, 14:21])
        self.tau_hat_filt[on] = (1.0 - self.lpf) * self.tau_hat_filt[on] + self.lpf * th
        self.z_cmd[on] = zz[:, 21:28]
        tau_hat[on], tau_ctrl[on] = th, self.tau_hat_filt[on]
        return qv_ctrl, tau_hat, tau_ctrl

    def cmd(self, k, tau_cmd, tau_app):
        """tau_app (B, 7) with the injected rows replaced"""
        nc = self.d_cmd + 1
        on = self.row >= 0
        r = self.row[on]
        self.cmd_ring[k % nc, on] = tau_cmd[on]
        out = tau_app.copy()
        out[on] = self.a[r, None] * self.cmd_ring[(k + 1) % nc, on] + self.b[r, None] + (0.0 + self.sig[2] * self.z_cmd[on])
        return out


def test_fleet_inject_struct_layout_matches_header():
    fi = [n for n, _ in _abi.FleetInject._fields_]
    offs = "".join(f'  printf("%zu ", offsetof(ffddp_fleet_inject, {n}));\n' for n in fi)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ffddp.h"\nint main(void) {\n'
           '  printf("%zu %d %d %d ", sizeof(ffddp_fleet_inject), FFDDP_INJECT_NOISE_TABLE, FFDDP_INJECT_NOISE_PHILOX,\n'
           '         FFDDP_INJECT_NZ);\n' + offs + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(src)
        exe = Path(d) / "t"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(exe)], check=True)
        vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[:4] == [ctypes.sizeof(_abi.FleetInject), _abi.INJECT_NOISE_TABLE, _abi.INJECT_NOISE_PHILOX, _abi.INJECT_NZ]
    assert vals[4:] == [getattr(_abi.FleetInject, n).offset for n in fi]
    assert _abi.INJECT_NZ == U.NZ and _abi.INJECT_NOISE_MODES == {"numpy": 0, "philox": 1}
    # the header's field order is the binding's, and the three entry points are bound
    hdr = (ROOT / "include" / "ffddp.h").read_text()
    body = hdr.split("typedef struct ffddp_fleet_inject {")[1].split("} ffddp_fleet_inject;")[0]
    decl = [ln.split(";")[0] for ln in body.strip().splitlines() if ";" in ln]
    assert [piece.replace("*", " ").split()[-1] for d in decl for piece in d.split(",")] == fi
    assert {"ffddp_fleet_inject_obs_dev", "ffddp_fleet_inject_cmd_dev", "ffddp_fleet_noise_dev"} <= set(_abi.SYMBOLS)
    # the Philox tag is defined once in the library and mirrored here
    consts = (ROOT / "franka-force-feedback-mpc_amd" / "csrc" / "ffddp_consts.hpp").read_text()
    assert f"INJECT_PHILOX_TAG = 0x{U.PHILOX_TAG:016x}ull" in consts


def test_fleet_inject_null_handle_errors():
    lib = _abi.load()
    inj = _abi.FleetInject()
    obs = lib.ffddp_fleet_inject_obs_dev(None, 1, ctypes.byref(inj), 0, None, None, None, 7, None, None, None, None, None)
    cmd = lib.ffddp_fleet_inject_cmd_dev(None, 1, ctypes.byref(inj), 0, None, None, None)
    noise = lib.ffddp_fleet_noise_dev(None, 1, None, 0, None, None, None)
    assert obs == -1 and cmd == -1 and noise == -1  # FFDDP_E_INVALID


@pytest.mark.parametrize("delays", [(2, 1), (0, 0)])
def test_predraw_through_the_kernels_restatement_equals_host_injectors(delays):
    """Three seeds, 300 ticks (across the host class's 256-tick chunk)."""
    seeds, steps = [15, 1500003, 7], 300
    kw = DELAYED if delays == (2, 1) else {}
    cfgs = [U.UncertaintyProfileConfig(seed=s, **kw) for s in seeds]
    assert U.delay_steps(cfgs[0], DT) == delays
    bat = U.BatchedUncertaintyInjector(dt=DT, nu=7, configs=cfgs)
    sc = U.ScenarioUncertaintyInjector(dt=DT, nu=7, config=cfgs[1])
    assert (bat.obs_delay_steps, bat.cmd_delay_steps) == delays == (sc.obs_delay_steps, sc.cmd_delay_steps)
    a, b, z = U.predraw(cfgs, steps)
    assert z.shape == (steps, 3, 28) and np.array_equal(a, bat.a) and np.array_equal(b, bat.b)
    assert (a[1], b[1]) == (sc.a, sc.b)
    ker = KernelRestatement(np.arange(3), a, b, *delays, bat.sig, 0.2)
    rng = np.random.default_rng(3)
    for k in range(steps):
        q, dq, tau = rng.normal(size=(3, 7)), rng.normal(size=(3, 7)), rng.normal(size=(3, 7)) * 10
        qv, th, thf = ker.obs(k, z[k], q, dq)
        qb, dqb = bat.observation_for_controller(q, dq)
        assert np.array_equal(qv[:, :7], qb) and np.array_equal(qv[:, 7:], dqb), k
        assert np.array_equal(th, bat.tau_hat) and np.array_equal(thf, bat.tau_hat_filt), k
        app = ker.cmd(k, tau, np.zeros((3, 7)))
        assert np.array_equal(app, bat.command_for_plant(tau)), k
        d = sc.observation_for_controller(_obs(q[1], dq[1]))
        assert np.array_equal(qv[1, :7], d.q) and np.array_equal(qv[1, 7:], d.dq), k
        assert np.array_equal(th[1], d.tau_meas_act) and np.array_equal(thf[1], d.tau_meas_act_filt), k
        assert np.array_equal(app[1], sc.command_for_plant(tau[1])), k


def test_philox_normals_raw_words_are_numpy_philox():
    for s in PHILOX_SEEDS:
        for k in PHILOX_TICKS:
            z, w = U.philox_normals([s], k, return_words=True)
            assert z.shape == (1, 28) and w.shape == (1, 7, 4) and w.dtype == np.uint64 and np.all(np.isfinite(z))
            for j in range(7):
                bg = np.random.Philox(key=np.array([s, U.PHILOX_TAG], dtype=np.uint64),
                                      counter=np.array([k, j, 0, 0], dtype=np.uint64))
                assert np.array_equal(w[0, j], bg.random_raw(4)), (s, k, j)
    # the table's order: q, dq, tau (observation), tau (command), 7 joints each, from (w0, w1) and (w2, w3)
    z, w = U.philox_normals([5], 3, return_words=True)
    u1 = (float(int(w[0, 2, 2]) >> 11) + 1.0) * 2.0 ** -53
    u2 = float(int(w[0, 2, 3]) >> 11) * 2.0 ** -53
    assert z[0, 14 + 2] == np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    assert z[0, 21 + 2] == np.sqrt(-2.0 * np.log(u1)) * np.sin(2.0 * np.pi * u2)


def test_philox_normals_moments():
    """A fixed set of n = 28 * 64 * 200 samples (seeds 0..63, ticks 0..199); 5 sigma limits."""
    zs = np.concatenate([U.philox_normals(np.arange(64), k).ravel() for k in range(200)])
    n = zs.size
    assert n == 28 * 64 * 200 and np.all(np.isfinite(zs))
    assert abs(zs.mean()) <= 5.0 / np.sqrt(n), zs.mean()
    assert abs(zs.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), zs.var()


def test_device_noise_refusals():
    """All refused before any device object is made, so this runs without a device."""
    kw = dict(scenarios=("flat", "actuation_uncertainty"), seeds=1, total_time=0.1, verbose=False)
    with pytest.raises(ValueError, match="device_loop"):
        FL.run_sweep(device_noise="numpy", **kw)
    with pytest.raises(ValueError, match="device_noise"):
        FL.run_sweep(device_loop=True, device_noise="bogus", **kw)
    with pytest.raises(ValueError, match="device_noise"):
        FL.run_sweep(device_noise="bogus", **kw)
    cfgs = [U.UncertaintyProfileConfig(seed=s) for s in range(4)]
    with pytest.raises(ValueError, match="philox"):
        U.predraw(cfgs, 100, max_table_bytes=224 * 100 * 4 - 1)
    assert U.predraw(cfgs, 100, max_table_bytes=224 * 100 * 4)[2].shape == (100, 4, 28)
