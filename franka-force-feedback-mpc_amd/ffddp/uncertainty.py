"""Benchmark uncertainty profile of the closed loop (src/run/uncertainty_profiles.py).

``actuation_uncertainty`` draws an actuation gain a and bias b once, delays
and perturbs the observations the controller sees (state noise, noisy torque
measurement with a first-order filter) and replaces the applied command by
a * (delayed command) + b + noise.  Same numpy Generator stream as the
reference (seeded PCG64, draws in the same order), so a run with the same
seed sees the same perturbations (tests/test_closed_loop.py pins it against
outputs the reference wrote).
"""
from __future__ import annotations

import dataclasses
from collections import deque
from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass
class UncertaintyProfileConfig:
    """uncertainty_profiles.py:12-30."""

    a_min: float = 0.95
    a_max: float = 1.05
    b_min: float = -0.1
    b_max: float = 0.1
    sigma_q: float = 5.0e-4
    sigma_dq: float = 2.0e-3
    sigma_tau: float = 5.0e-2
    delta_obs_cycles: int = 2
    delta_cmd_s: float = 1.0e-3
    seed: int = 0


def config_for_scenario(scenario: str, seed: int = 0) -> Optional[UncertaintyProfileConfig]:
    """Only actuation_uncertainty carries an injected profile (uncertainty_profiles.py:33-53)."""
    if str(scenario).strip().lower() != "actuation_uncertainty":
        return None
    return UncertaintyProfileConfig(seed=int(seed))


_ARRAY_FIELDS = ("q", "dq", "tau_meas", "tau_meas_filt", "tau_meas_act", "tau_meas_act_filt", "tau_cmd", "tau_act",
                 "tau_constraint", "tau_total", "tau_bias", "f_contact_world", "ee_pos", "ee_quat", "J_pos", "J_rot",
                 "ee_vel")


def copy_observation(obs):
    """Deep copy of the array fields of an Observation dataclass."""
    kw = {}
    for f in _ARRAY_FIELDS:
        if hasattr(obs, f):
            v = getattr(obs, f)
            kw[f] = None if v is None else np.asarray(v, dtype=float).copy()
    return dataclasses.replace(obs, **kw)


class ScenarioUncertaintyInjector:
    """uncertainty_profiles.py:84-161, draw for draw."""

    def __init__(self, dt: float, nu: int, config: UncertaintyProfileConfig, tau_lpf_alpha: float = 0.2):
        self.dt = float(max(dt, 1.0e-9))
        self.nu = int(nu)
        self.cfg = config
        self.rng = np.random.default_rng(int(config.seed))
        self.a = float(self.rng.uniform(float(config.a_min), float(config.a_max)))
        self.b = float(self.rng.uniform(float(config.b_min), float(config.b_max)))
        self.obs_delay_cycles_1khz = int(max(config.delta_obs_cycles, 0))
        # the observation delay is specified in 1 kHz cycles; convert to control steps
        self.obs_delay_steps = int(max(np.round(self.obs_delay_cycles_1khz * 1.0e-3 / self.dt), 0))
        self.cmd_delay_steps = int(max(np.round(float(config.delta_cmd_s) / self.dt), 0))
        self._obs_hist: deque = deque(maxlen=self.obs_delay_steps + 1)
        self._cmd_hist: deque = deque([np.zeros(self.nu) for _ in range(self.cmd_delay_steps + 1)],
                                      maxlen=self.cmd_delay_steps + 1)
        self._tau_hat_filt = np.zeros(self.nu)
        self._tau_lpf_alpha = float(np.clip(tau_lpf_alpha, 0.0, 1.0))

    def meta(self) -> dict:
        return {"a": float(self.a), "b": float(self.b), "sigma_q": float(self.cfg.sigma_q),
                "sigma_dq": float(self.cfg.sigma_dq), "sigma_tau": float(self.cfg.sigma_tau),
                "delta_obs_cycles_1khz": int(self.obs_delay_cycles_1khz), "delta_obs_steps": int(self.obs_delay_steps),
                "delta_cmd_steps": int(self.cmd_delay_steps), "delta_cmd_s": float(self.cfg.delta_cmd_s),
                "seed": int(self.cfg.seed)}

    def _tau_hat(self) -> np.ndarray:
        noise = self.rng.normal(0.0, float(self.cfg.sigma_tau), size=self.nu)
        return self.a * np.asarray(self._cmd_hist[0], dtype=float).reshape(self.nu) + self.b + noise

    def observation_for_controller(self, obs):
        cur = copy_observation(obs)
        if not self._obs_hist:
            self._obs_hist.extend(copy_observation(cur) for _ in range(self.obs_delay_steps + 1))
        else:
            self._obs_hist.append(cur)
        out = copy_observation(self._obs_hist[0])
        out.q = out.q + self.rng.normal(0.0, float(self.cfg.sigma_q), size=self.nu)
        out.dq = out.dq + self.rng.normal(0.0, float(self.cfg.sigma_dq), size=self.nu)
        th = self._tau_hat()
        a = self._tau_lpf_alpha
        self._tau_hat_filt = (1.0 - a) * self._tau_hat_filt + a * th
        out.tau_meas = th.copy()
        out.tau_meas_filt = self._tau_hat_filt.copy()
        out.tau_meas_act = th.copy()
        out.tau_meas_act_filt = self._tau_hat_filt.copy()
        return out

    def command_for_plant(self, tau_cmd_nominal) -> np.ndarray:
        self._cmd_hist.append(np.asarray(tau_cmd_nominal, dtype=float).reshape(self.nu).copy())
        return self._tau_hat()


class BatchedUncertaintyInjector:
    """ScenarioUncertaintyInjector for many instances at once (the closed-loop
    fleet's actuation_uncertainty scenario): each instance keeps its own
    seeded Generator and draws, in the scalar injector's order, the same
    numbers -- per tick 7 + 7 + 7 normals for the observation (q, dq, torque
    measurement) and 7 for the command -- pre-drawn a chunk of ticks at a time
    (a Generator's normals are one stream however many a call asks for), and
    the delay lines are ring buffers over the batch.  Only the fields the
    fleets read are produced: the delayed noisy (q, dq), the applied command
    and, as attributes refreshed by observation_for_controller, the torque
    measurement ``tau_hat`` (the scalar tau_meas_act) and its first-order
    filter ``tau_hat_filt`` (tau_meas_act_filt), both (B, nu).  Bit-identical
    to per-instance ScenarioUncertaintyInjector calls
    (tests/test_closed_loop.py, tests/test_fleet_ff_cpu.py).

    The configs may be any mix: instance i keeps its own delays
    (``delay[i]`` = delay_steps(cfg_i, dt), in ticks), its own sigma triple
    (``sigma[i]``) and its own a / b ranges.  The rings are as deep as the
    largest delay, [d_max + 1][B][.]; instance i uses slots 0..d_i of its
    column with its own modulus, so its slot sequence is the one a ring of its
    own depth would give.  ``delay`` (B, 2) and ``sigma`` (B, 3) may also be
    given explicitly, in place of the configs' values.  ``obs_delay_steps`` /
    ``cmd_delay_steps`` are the ring depths (the largest delays: every
    instance's when they agree) and ``sig`` the common sigma triple, or None
    when the instances' sigmas differ."""

    CHUNK = 256  # ticks of normals drawn per Generator call

    def __init__(self, dt: float, nu: int, configs, tau_lpf_alpha: float = 0.2, delay=None, sigma=None):
        self.nu = int(nu)
        self.dt = float(max(dt, 1.0e-9))
        self.cfgs = list(configs)
        self.B = len(self.cfgs)
        c0 = self.cfgs[0] if self.cfgs else UncertaintyProfileConfig()
        self.rngs = [np.random.default_rng(int(c.seed)) for c in self.cfgs]
        ab = [(float(r.uniform(float(c.a_min), float(c.a_max))), float(r.uniform(float(c.b_min), float(c.b_max))))
              for r, c in zip(self.rngs, self.cfgs)]
        self.a = np.array([x[0] for x in ab])
        self.b = np.array([x[1] for x in ab])
        if delay is None:
            delay = [delay_steps(c, self.dt) for c in self.cfgs]
        if sigma is None:
            sigma = [(float(c.sigma_q), float(c.sigma_dq), float(c.sigma_tau)) for c in self.cfgs]
        self.delay = np.array(delay, dtype=np.int64).reshape(self.B, 2)
        self.sigma = np.array(sigma, dtype=float).reshape(self.B, 3)
        if np.any(self.delay < 0):
            raise ValueError("BatchedUncertaintyInjector: a delay below 0")
        d0 = delay_steps(c0, self.dt)
        self.obs_delay_steps = int(self.delay[:, 0].max()) if self.B else d0[0]
        self.cmd_delay_steps = int(self.delay[:, 1].max()) if self.B else d0[1]
        self.sig = (float(c0.sigma_q), float(c0.sigma_dq), float(c0.sigma_tau))
        if self.B:
            self.sig = tuple(float(x) for x in self.sigma[0]) if np.all(self.sigma == self.sigma[0]) else None
        self._all = np.arange(self.B)
        self._no, self._nc = self.delay[:, 0] + 1, self.delay[:, 1] + 1  # each instance's ring moduli
        self._obs = None  # [D+1][B][14] ring of (q, dq); instance i's slot _oi[i] is its oldest
        self._oi = np.zeros(self.B, dtype=np.int64)
        self._cmd = np.zeros((self.cmd_delay_steps + 1, self.B, self.nu))
        self._ci = np.zeros(self.B, dtype=np.int64)
        self._z = np.zeros((self.B, 0, 4 * self.nu))
        self._zi = 0
        self._tau_lpf_alpha = float(np.clip(tau_lpf_alpha, 0.0, 1.0))
        self.tau_hat = np.zeros((self.B, self.nu))
        self.tau_hat_filt = np.zeros((self.B, self.nu))

    def _normals(self):
        """this tick's 28 normals per instance: q, dq, tau (observation), tau (command)"""
        if self._zi >= self._z.shape[1]:
            self._z = np.stack([r.standard_normal(self.CHUNK * 4 * self.nu).reshape(self.CHUNK, 4 * self.nu)
                                for r in self.rngs])
            self._zi = 0
        z = self._z[:, self._zi]
        self._zi += 1
        return z

    def _tau_hat(self, z7):
        return (self.a[:, None] * self._cmd[self._ci, self._all] + self.b[:, None]
                + (0.0 + self.sigma[:, 2:3] * z7))

    def observation_for_controller(self, q, dq):
        """(q, dq) [B][nu] -> the delayed, noisy (q, dq) the controllers see."""
        nu = self.nu
        cur = np.concatenate([np.asarray(q, float), np.asarray(dq, float)], 1)
        if self._obs is None:
            self._obs = np.repeat(cur[None], self.obs_delay_steps + 1, 0)
            self._oi[:] = 0
        else:  # deque(maxlen).append: the oldest slot takes the newest entry
            self._obs[self._oi, self._all] = cur
            self._oi = (self._oi + 1) % self._no
        old = self._obs[self._oi, self._all]
        self._z_tick = z = self._normals()
        qo = old[:, :nu] + (0.0 + self.sigma[:, 0:1] * z[:, :nu])
        dqo = old[:, nu:] + (0.0 + self.sigma[:, 1:2] * z[:, nu:2 * nu])
        # the torque measurement and its filter, as ScenarioUncertaintyInjector.observation_for_controller
        self.tau_hat = self._tau_hat(z[:, 2 * nu:3 * nu])
        a = self._tau_lpf_alpha
        self.tau_hat_filt = (1.0 - a) * self.tau_hat_filt + a * self.tau_hat
        return qo, dqo

    def command_for_plant(self, tau_cmd):
        """tau_cmd [B][nu] -> the applied torques a * (delayed command) + b + noise."""
        self._cmd[self._ci, self._all] = np.asarray(tau_cmd, float)
        self._ci = (self._ci + 1) % self._nc
        return self._tau_hat(self._z_tick[:, 3 * self.nu:])


# -- the injector on the device (fleet_loop.DeviceFleetLoop, csrc/ffddp_inject.hpp) --------------
NZ = 28  # normals per instance and tick: q, dq, tau (observation), tau (command), 7 each
PHILOX_TAG = 0x4646444450494E4A  # key word 1 of the device noise stream (ffddp_consts.hpp INJECT_PHILOX_TAG)


def delay_steps(config: UncertaintyProfileConfig, dt: float):
    """(observation, command) delay in control steps of period dt, as the injectors round them."""
    dt = float(max(dt, 1.0e-9))
    d_obs = int(max(np.round(int(max(config.delta_obs_cycles, 0)) * 1.0e-3 / dt), 0))
    d_cmd = int(max(np.round(float(config.delta_cmd_s) / dt), 0))
    return d_obs, d_cmd


def draw_gain_bias(configs):
    """Each instance's actuation gain a and bias b (B,): the first two uniforms
    of default_rng(seed), as the injectors draw them; also the Generators,
    advanced past them."""
    rngs = [np.random.default_rng(int(c.seed)) for c in configs]
    ab = [(float(r.uniform(float(c.a_min), float(c.a_max))), float(r.uniform(float(c.b_min), float(c.b_max))))
          for r, c in zip(rngs, configs)]
    return np.array([x[0] for x in ab]), np.array([x[1] for x in ab]), rngs


def predraw(configs, steps: int, max_table_bytes: int = 1 << 30):
    """The noise of ``steps`` ticks of BatchedUncertaintyInjector(configs),
    drawn ahead: a, b (B,) and z (steps, B, 28), row k of instance i being the
    28 standard normals its default_rng(seed) stream gives tick k, in the host
    class's order (q, dq, tau of the observation, tau of the command).  The
    device loop's ``noise="numpy"`` uploads z once.  It takes 224 * steps * B
    bytes (46 MB for the sweep's 256 instances x 800 ticks); above
    max_table_bytes this raises ValueError: use noise="philox", which needs
    no table."""
    configs = list(configs)
    steps = int(steps)
    nbytes = 8 * NZ * steps * len(configs)
    if nbytes > int(max_table_bytes):
        raise ValueError(f"predraw: the noise table of {len(configs)} instances x {steps} ticks takes {nbytes} bytes, "
                         f"above max_table_bytes = {int(max_table_bytes)}; use noise=\"philox\", which generates "
                         "the normals on the device and needs no table")
    a, b, rngs = draw_gain_bias(configs)
    z = np.zeros((steps, len(configs), NZ))
    for i, r in enumerate(rngs):  # a Generator's normals are one stream however many a call asks for
        z[:, i] = r.standard_normal(steps * NZ).reshape(steps, NZ)
    return a, b, z


_PHILOX_M = (0xD2E7470EE14C6C93, 0xCA5A826395121157)
_PHILOX_W = (0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B)
_M64 = (1 << 64) - 1


def philox4x64_10(counter, key):
    """One Philox4x64-10 block (Salmon et al. 2011) in Python integers: four 64-bit words."""
    c0, c1, c2, c3 = (int(x) & _M64 for x in counter)
    k0, k1 = (int(x) & _M64 for x in key)
    for _ in range(10):
        p0, p1 = _PHILOX_M[0] * c0, _PHILOX_M[1] * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & _M64, (p0 >> 64) ^ c3 ^ k1, p0 & _M64
        k0, k1 = (k0 + _PHILOX_W[0]) & _M64, (k1 + _PHILOX_W[1]) & _M64
    return c0, c1, c2, c3


def philox_normals(seeds, k: int, return_words: bool = False):
    """The device loop's ``noise="philox"`` normals of tick k, restated in
    numpy: z (B, 28) in the table's order.  Joint j of the instance seeded s
    takes the block philox4x64_10([k + 1, j, 0, 0], [s, PHILOX_TAG]) -- the
    first four words of numpy.random.Philox(key=[s, PHILOX_TAG], counter=[k, j,
    0, 0]).random_raw(4), which increments the counter before it generates --
    and Box-Muller on its pairs: u1 = ((w0 >> 11) + 1) 2^-53, u2 = (w1 >> 11)
    2^-53, z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2);
    (w0, w1) -> the joint's q and dq normals, (w2, w3) -> its two torque
    normals (observation, command).  return_words: also the raw words
    (B, 7, 4) uint64."""
    seeds = [int(s) for s in np.asarray(seeds, dtype=object).reshape(-1)]
    w = np.array([[philox4x64_10((int(k) + 1, j, 0, 0), (s, PHILOX_TAG)) for j in range(7)] for s in seeds],
                 dtype=np.uint64).reshape(len(seeds), 7, 4)
    u1 = ((w[..., 0::2] >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (w[..., 1::2] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    t = (2.0 * np.pi) * u2
    zn = np.stack([r[..., 0] * np.cos(t[..., 0]), r[..., 0] * np.sin(t[..., 0]),
                   r[..., 1] * np.cos(t[..., 1]), r[..., 1] * np.sin(t[..., 1])], 1)  # (B, 4, 7)
    z = zn.reshape(len(seeds), NZ)
    return (z, w) if return_words else z
