"""Fleet closed loop: B independent classical MPC controllers stepped together
(BASELINE.json configs[3]: "All 5 scenarios x 256 seeds = 1280-instance sweep
sharded over 8 MI355X, RCCL all-gather of costs").

``FleetClassicalMPC`` keeps, per instance, exactly the state and the per-tick
logic of ``ClassicalCrocoddylMPC.compute_control`` (crocoddyl_classical.py:
305-440, our B = 1 mirror in controller.py) in arrays, and runs ONE batched
device solve per control tick for all B instances (warm starts, problem
references and results stay in HBM; only x0, the shared node references and
the first knot of the solution cross PCIe).  With ``mpc_update_steps = P > 1``
an instance solves on every P-th tick, or at once when it has no plan (a mode
switch, an unstable tick or a non-finite solve dropped it), and runs the
feedback policy on the receding plan in between; the batched solve then takes
the tick's ``solved_now`` mask (``solve_dev(active=...)``).  The kept solution
is never moved between solves: ``age`` counts the controllers' _rollout_shift
calls since it was kept and every reader indexes through it (knot i of the
shifted lists is knot min(i + age, N - 1) of keep_us / keep_K, min(i + age, N)
of keep_xs), the convention of the device tick (include/ffddp.h,
ffddp_fleet_sched), so the state can be copied between the two.
``apply_command_filter`` is _safe_tau's filter, ``safe_tau_batch``.  At
period 1 without the filter a tick's launches and results are unchanged.

``FleetForceFeedbackMPC`` is the same for ``ForceFeedbackCrocoddylMPC``
(state y = (q, v, tau_hat), nx = 21; torque policy of Eq. 14-18 on the host).
Its tick's glue around the solve -- the warm-start shift, keeping the
solutions whose first control is finite, packing the first knot for the host
-- runs in two kernels of the library (include/ffddp.h:
ffddp_fleet_warm_start_dev, ffddp_fleet_keep_dev); the classical fleet uses
them with ``device_tick=True`` and torch operations by default.

``run_sweep`` closes B loops around ``BatchedPlant`` (one launch per tick for
all plants): per instance a scenario (table tilt / actuation mismatch /
uncertainty injector, run_classical.py:53-91 and uncertainty_profiles.py) and
a seed.  The seed perturbs the start posture (q0 = neutral + N(0, 0.02^2),
seeded) and seeds the actuation-uncertainty injector; the reference runs one
scenario from the keyframe with a fixed seed, so this is a sweep around its
configuration rather than a replay of it.  Ranks (torch.distributed) take
contiguous shards of the instances; the per-instance summary metrics are
all-gathered at the end (RCCL on the GPU box).  ``run_sweep(device_loop=True)``
runs the loop itself on the device (fleet_loop.DeviceFleetLoop); the injector
runs there too once ``device_noise`` names the source of its normals.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from . import robot as R
from .config import COST_WEIGHT_NAMES, OcpConfig
from .controller import (_OCP_FIELDS, _quat_wxyz_to_R, classical_benchmark_config, ff_benchmark_config,
                         ff_filter_alpha)
from .plant import JOINT_DAMPING, BatchedPlant, PandaTablePlant, PlantPhysics, plant_rows
from .runlog import summary_metrics
from .solver import BatchedBoxFDDP
from .trajectory import (TABLE_CENTER, TABLE_HALF_Z, TOOL_RADIUS, FleetTask, ForceProfile, make_approach_then_circle,
                         sample_force, sample_records, task_records, with_contact_hold)
from .uncertainty import BatchedUncertaintyInjector, config_for_scenario, delay_steps

Traj = Callable[[float], Tuple[np.ndarray, np.ndarray, bool]]


def node_ref(traj_fn: Traj, t0: float, N: int, dt_ocp: float, R_mj_from_pin, p_site_minus_frame_pin) -> np.ndarray:
    """A tick's node references (N+1, 6): the trajectory sampled at
    t0 + k dt_ocp, mapped to the Pinocchio frame (crocoddyl_classical.py:
    250-258, 526-546).  The fleets and the device loop's table share it."""
    out = np.zeros((N + 1, 6))
    sample = getattr(traj_fn, "sample", None)
    if sample is not None:  # same bits as the loop below (R_MJ_FROM_PIN is a signed permutation)
        P, V, _ = sample(np.array([t0 + k * dt_ocp for k in range(N + 1)]))
        out[:, :3] = P @ R_mj_from_pin - p_site_minus_frame_pin
        out[:, 3:] = V @ R_mj_from_pin
        return out
    for k in range(N + 1):
        p, v, _ = traj_fn(t0 + k * dt_ocp)
        out[k, :3] = R_mj_from_pin.T @ np.asarray(p, float) - p_site_minus_frame_pin
        out[k, 3:] = R_mj_from_pin.T @ np.asarray(v, float)
    return out


def fleet_ocp_config(cfg, variant: str, N: int, dt_ocp: float, R_des) -> OcpConfig:
    """The solver's OCP definition from a controller configuration
    (_MPCBase._ocp_config; variant "ff": ForceFeedbackCrocoddylMPC._ocp_config)."""
    ocp = OcpConfig(variant=variant, horizon=N, dt=dt_ocp, R_des=R_des)
    for f in _OCP_FIELDS:
        setattr(ocp, f, getattr(cfg, f))
    ocp.tau_limits = np.asarray(cfg.tau_limits, float).copy()
    if variant == "ff":
        ocp.ff_alpha = ff_filter_alpha(cfg, dt_ocp)
        ocp.w_w = float(cfg.w_w)
        ocp.w_w_soft_limits = float(cfg.w_w_soft_limits)
        ocp.w_y = float(cfg.w_y)
        ocp.y_weights = np.concatenate([cfg.y_q_weights, cfg.y_v_weights, cfg.y_tau_weights]).astype(float)
        ocp.use_inner_state_reg = bool(cfg.use_inner_state_reg)
        ocp.use_inner_tau_reg = bool(cfg.use_inner_tau_reg)
    return ocp


def safe_tau_batch(target, prev, cfg, dt: float) -> np.ndarray:
    """_safe_tau (crocoddyl_classical.py:260-284) for B rows at once, bit for
    bit the scalar controller's: a row with a non-finite entry becomes the
    previous command, the clip to tau_limits, and with apply_command_filter
    the trust region, the rate limit (tau_rate_limit * dt) and the smoothing,
    in its order and grouping.  target, prev (B, 7) -> the commands (B, 7),
    which are also the next ``prev``."""
    target = np.asarray(target, float)
    prev = np.asarray(prev, float)
    lim = np.asarray(cfg.tau_limits, float)
    bad = ~np.all(np.isfinite(target), 1)
    target = np.clip(np.where(bad[:, None], prev, target), -lim, lim)
    if not bool(cfg.apply_command_filter):
        return target
    d = np.clip(target - prev, -cfg.tau_trust_inf, cfg.tau_trust_inf)
    max_step = np.asarray(cfg.tau_rate_limit, float) * float(dt)
    d = np.clip(d, -max_step, max_step)
    a = float(np.clip(cfg.tau_smoothing_alpha, 0.0, 1.0))
    return np.clip((1.0 - a) * prev + a * (prev + d), -lim, lim)


class _FleetBase:
    """What the fleet controllers share: the solver and its device arrays, the
    kept solution and its ``valid`` mask, the surface latch, the problem
    references, and the device-side tick (``_tick_device``)."""

    variant = "classical"
    nx = 14

    def __init__(self, B: int, traj_fn: Traj, config, q_nom, tau0, R_site_from_pin_ee, p_site_minus_frame_pin,
                 device: int = 0):
        import torch

        cfg = config
        if int(cfg.mpc_update_steps) < 1:
            raise ValueError(f"{type(self).__name__}: mpc_update_steps must be at least 1")
        self.period = int(cfg.mpc_update_steps)
        # the scheduled tick (_tick_sched); period 1 without the filter keeps the plain one
        self.sched = self.period != 1 or bool(cfg.apply_command_filter)
        self.torch = torch
        self.B, self.cfg, self.traj_fn = int(B), cfg, traj_fn
        self.N = int(cfg.horizon)
        self.dev = torch.device("cuda", device)
        self.R_mj_from_pin = R.R_MJ_FROM_PIN.copy()
        self.R_site_from_pin_ee = np.asarray(R_site_from_pin_ee, float)
        self.p_site_minus_frame_pin = np.asarray(p_site_minus_frame_pin, float)
        self.R_des = self.R_mj_from_pin.T @ R.vertical_down_rotation_mj() @ self.R_site_from_pin_ee.T
        self.q_nom = np.asarray(q_nom, float).reshape(self.B, 7).copy()
        self.tau_prev = np.asarray(tau0, float).reshape(self.B, 7).copy()
        self.dt_ocp = float(cfg.dt_ocp) if cfg.dt_ocp is not None else float(cfg.dt)
        self.solver = BatchedBoxFDDP(self._ocp_config(), max_batch=self.B, device=device)
        self.solver.neg_step_rule = int(getattr(cfg, "neg_step_rule", 0))
        f64 = dict(dtype=torch.float64, device=self.dev)
        B, N, nx = self.B, self.N, self.nx
        self.T = dict(
            x0=torch.zeros((B, nx), **f64), node_ref=torch.zeros((B, N + 1, 6), **f64),
            inst_ref=torch.zeros((B, 21), **f64), surface=torch.zeros(B, dtype=torch.uint8, device=self.dev),
            xs_init=torch.zeros((B, N + 1, nx), **f64), us_init=torch.zeros((B, N, 7), **f64),
            xs=torch.zeros((B, N + 1, nx), **f64), us=torch.zeros((B, N, 7), **f64),
            K=torch.zeros((B, N, 7, nx), **f64), cost=torch.zeros(B, **f64),
            iters=torch.zeros(B, dtype=torch.int32, device=self.dev), ok=torch.zeros(B, dtype=torch.uint8, device=self.dev),
            fn_pred=torch.zeros((B, 2), **f64), stats=torch.zeros((B, _abi.NSTATS), dtype=torch.int32, device=self.dev),
        )
        # the kept solution (solver.xs/us/K of the last solve whose us[0] was finite)
        self.keep_xs = torch.zeros((B, N + 1, nx), **f64)
        self.keep_us = torch.zeros((B, N, 7), **f64)
        self.keep_K = torch.zeros((B, N, 7, nx), **f64)
        self.valid = np.zeros(B, bool)
        self.latched = np.zeros(B, bool)
        self.loss_count = np.zeros(B, np.int64)
        self.prev_mode = np.full(B, -1, np.int8)
        self.since = np.zeros(B, np.int32)  # ticks since the instance's last solve
        self.age = np.zeros(B, np.int32)    # _rollout_shift calls since the kept solution was kept
        self._stream = torch.cuda.current_stream(self.dev).cuda_stream
        self._tk = None  # the device tick's arrays, made on its first use
        self.last_info = {}

    def _ocp_config(self) -> OcpConfig:
        return fleet_ocp_config(self.cfg, self.variant, self.N, self.dt_ocp, self.R_des)

    def close(self):
        self.solver.close()

    def _phase(self, fn_meas, ee_z, t: float) -> np.ndarray:
        """_surface_mode + _track_mode: this tick's surface flags; a mode
        switch drops the instance's warm start."""
        _, _, hint = self.traj_fn(t)
        surface_now = self._surface(np.asarray(fn_meas, float), np.asarray(ee_z, float), hint)
        changed = (self.prev_mode >= 0) & (surface_now != (self.prev_mode == 1))
        self.valid &= ~changed
        self.prev_mode = surface_now.astype(np.int8)
        return surface_now

    def _tau_ref(self, q) -> np.ndarray:
        """_compute_tau_reference (crocoddyl_classical.py:453-460), vectorised."""
        tmode = str(self.cfg.torque_ref_mode).strip().lower()
        if tmode == "zero":
            return np.zeros((self.B, 7))
        if tmode == "gravity_qnom":
            return _abi.gravity_torque(self.q_nom)
        return _abi.gravity_torque(q)

    # -- the tick on the device (include/ffddp.h: ffddp_fleet_warm_start_dev / _keep_dev) ----
    def _tick_arrays(self):
        """One page of host memory laid out as the tick's inputs, its device
        twin, and views of both: float64 blocks x0, inst_ref, u_cold, the
        shared node references, then the uint8 flags surface and valid (each
        block on a 256-byte boundary)."""
        torch = self.torch
        B, N, nx = self.B, self.N, self.nx
        specs = (("x0", (B, nx), np.float64), ("inst_ref", (B, 21), np.float64), ("u_cold", (B, 7), np.float64),
                 ("node1", (1, N + 1, 6), np.float64), ("surface", (B,), np.uint8), ("valid", (B,), np.uint8))
        offs, tot = {}, 0
        for k, shape, dt in specs:
            offs[k] = tot
            tot += (int(np.prod(shape)) * np.dtype(dt).itemsize + 255) // 256 * 256
        host = np.zeros(tot, np.uint8)
        dev = torch.zeros(tot, dtype=torch.uint8, device=self.dev)
        hv, t = {}, dict(self.T)
        for k, shape, dt in specs:
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            hv[k] = host[offs[k]: offs[k] + n].view(dt).reshape(shape)
            d = dev[offs[k]: offs[k] + n]
            t[k] = (d.view(torch.float64) if dt is np.float64 else d).view(shape)
        t.update(keep_xs=self.keep_xs, keep_us=self.keep_us, keep_K=self.keep_K,
                 first=torch.zeros((B, _abi.fleet_first_w(nx)), dtype=torch.float64, device=self.dev))
        return dict(host=host, dev=dev, hv=hv, t=t)

    def _tick_device(self, x0, inst_ref, u_cold, surface_now, t: float) -> dict:
        """One tick through the library's glue kernels: one packed copy up,
        warm start, solve, keep, one copy of the packed first-knot records
        down.  Updates ``valid`` with the solves kept; returns the records'
        fields (of the kept solutions: us0, xs0, xs1, K0; of this solve: fin,
        cost, iters, ok, neg_acc, fn0, fn1)."""
        if self._tk is None:
            self._tk = self._tick_arrays()
        torch, B, N, nx = self.torch, self.B, self.N, self.nx
        hv, T = self._tk["hv"], self._tk["t"]
        hv["x0"][:], hv["inst_ref"][:], hv["u_cold"][:] = x0, inst_ref, u_cold
        hv["node1"][0] = self._node_ref(t)
        hv["surface"][:], hv["valid"][:] = surface_now, self.valid
        self._tk["dev"].copy_(torch.from_numpy(self._tk["host"]))
        T["node_ref"].copy_(T["node1"].expand(B, N + 1, 6))
        self.solver.fleet_warm_start_dev(T, stream=self._stream)
        self.solver.solve_dev(T, maxiter=int(self.cfg.max_iters), is_feasible=False, stream=self._stream)
        self.solver.fleet_keep_dev(T, stream=self._stream)
        down = T["first"].cpu().numpy()
        o = 8 + 9 * nx
        r = dict(fin=down[:, 0] != 0, us0=down[:, 1:8], xs0=down[:, 8:8 + nx], xs1=down[:, 8 + nx:8 + 2 * nx],
                 K0=down[:, 8 + 2 * nx:o].reshape(B, 7, nx), cost=down[:, o].copy(),
                 iters=down[:, o + 1].astype(np.int32), ok=down[:, o + 2] != 0, neg_acc=down[:, o + 3].astype(np.int32),
                 fn0=down[:, o + 4], fn1=down[:, o + 5])
        self.valid |= r["fin"]
        return r

    # -- the scheduled tick (mpc_update_steps > 1 or the command filter) ---------------
    def _tick_sched(self, x0, inst_ref, u_cold, surface_now, t: float) -> dict:
        """One tick in which only the instances that need it solve
        (_need_solve: no kept solution, or the period has run out), as torch
        indexing around solve_dev(active=need).  Returns _tick_device's record
        -- the kept first knot read through ``age`` -- plus ``need``.  The
        counters are advanced by _sched_advance once the command is out."""
        torch, B, N, nx, T, dev = self.torch, self.B, self.N, self.nx, self.T, self.dev
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        need = (~self.valid) | (self.since.astype(np.int64) + 1 >= self.period)
        T["x0"].copy_(up(x0))
        T["inst_ref"].copy_(up(inst_ref))
        T["surface"].copy_(up(np.asarray(surface_now).astype(np.uint8)))
        T["node_ref"].copy_(up(self._node_ref(t))[None].expand(B, N + 1, 6))
        # _shift_guess of the lists shifted `age` times; rows of instances that do not solve stay as they are
        a_d = up(np.minimum(self.age, N).astype(np.int64))
        valid_d, need_d = up(self.valid)[:, None, None], up(need.astype(np.uint8))
        ix = torch.clamp(torch.arange(N + 1, device=dev)[None, :] + a_d[:, None], max=N)
        xs_sh = torch.gather(self.keep_xs, 1, ix[:, :, None].expand(B, N + 1, nx))
        xs_i = T["x0"][:, None, :].expand(B, N + 1, nx).clone()
        xs_i[:, 1:] = torch.where(valid_d, xs_sh[:, 1:], xs_i[:, 1:])
        iu = torch.clamp(torch.arange(N, device=dev)[None, :] + 1 + a_d[:, None], max=N - 1)
        us_sh = torch.gather(self.keep_us, 1, iu[:, :, None].expand(B, N, 7))
        us_i = torch.where(valid_d, us_sh, up(u_cold)[:, None, :].expand(B, N, 7))
        nm = need_d.bool()
        T["xs_init"].copy_(torch.where(nm[:, None, None], xs_i, T["xs_init"]))
        T["us_init"].copy_(torch.where(nm[:, None, None], us_i, T["us_init"]))
        self._need_d = need_d  # alive until the solve has run
        self.solver.solve_dev(T, maxiter=int(self.cfg.max_iters), is_feasible=False, stream=self._stream,
                              active=need_d)
        fin = nm & torch.isfinite(T["us"][:, 0]).all(1)
        f3 = fin[:, None, None]
        self.keep_xs.copy_(torch.where(f3, T["xs"], self.keep_xs))
        self.keep_us.copy_(torch.where(f3, T["us"], self.keep_us))
        self.keep_K.copy_(torch.where(fin[:, None, None, None], T["K"], self.keep_K))
        fin_h = fin.cpu().numpy()
        self.age = np.where(fin_h, 0, self.age).astype(np.int32)
        self.valid |= fin_h
        # knot 0 of the shifted lists
        a = np.minimum(self.age, N).astype(np.int64)
        ar = torch.arange(B, device=dev)
        ku, kx, kx1 = up(np.minimum(a, N - 1)), up(a), up(np.minimum(a + 1, N))
        h = lambda x: x.cpu().numpy()  # noqa: E731
        stats9 = h(T["stats"][:, 9]).astype(np.int32)
        return dict(need=need, fin=fin_h, us0=h(self.keep_us[ar, ku]), xs0=h(self.keep_xs[ar, kx]),
                    xs1=h(self.keep_xs[ar, kx1]), K0=h(self.keep_K[ar, ku]), cost=h(T["cost"]).copy(),
                    iters=h(T["iters"]).astype(np.int32), ok=h(T["ok"]) != 0, neg_acc=np.where(need, stats9, 0),
                    fn0=h(T["fn_pred"][:, 0]), fn1=h(T["fn_pred"][:, 1]))

    def _sched_advance(self, need):
        """The end of a scheduled tick: ``since`` restarts for the instances
        that solved; the others' plan recedes by one knot (_rollout_shift)."""
        self.since = np.where(need, 0, self.since + 1).astype(np.int32)
        self.age = np.where(need, self.age, self.age + 1).astype(np.int32)

    # -- per-tick pieces (crocoddyl_classical.py line refs as in controller.py) -------
    def _surface(self, fn_meas, ee_z, hint: bool) -> np.ndarray:
        """_surface_mode / _detect_surface (:286-303), vectorised."""
        if str(self.cfg.phase_source).strip().lower() != "force_latch":
            return np.full(self.B, bool(hint))
        near = np.isfinite(ee_z) & (ee_z <= float(self.cfg.z_contact) + float(self.cfg.z_contact_band))
        lost = fn_meas < self.cfg.fn_contact_off
        cnt = np.where(self.latched, np.where(lost, self.loss_count + 1, 0), 0)
        release = self.latched & (cnt >= int(self.cfg.contact_release_steps))
        engage = (~self.latched) & ((fn_meas > self.cfg.fn_contact_on) | (bool(hint) & near))
        self.latched = (self.latched & ~release) | engage
        self.loss_count = np.where(release | engage, 0, cnt)
        return self.latched.copy()

    def _node_ref(self, t0: float) -> np.ndarray:
        return node_ref(self.traj_fn, t0, self.N, self.dt_ocp, self.R_mj_from_pin, self.p_site_minus_frame_pin)

    def _command(self, tau_raw, cost, v, tau_bias):
        """The unstable fallback (crocoddyl_classical.py:392-404) and _safe_tau
        (:260-284, safe_tau_batch) -> tau_cmd, |tau_raw|inf, unstable."""
        cfg, B = self.cfg, self.B
        tau_raw_inf = np.max(np.abs(tau_raw), 1)
        unstable = (~np.isfinite(cost)) | (cost > float(cfg.max_solver_cost)) | (tau_raw_inf > float(cfg.max_tau_raw_inf))
        fallback = np.asarray(tau_bias, float).reshape(B, 7) - float(cfg.fallback_dq_damping) * v
        tau_raw = np.where(unstable[:, None], fallback, tau_raw)
        self.valid &= ~unstable
        tau_cmd = safe_tau_batch(tau_raw, self.tau_prev, cfg, float(cfg.dt))
        self.tau_prev = tau_cmd.copy()
        return tau_cmd, tau_raw_inf, unstable


class FleetClassicalMPC(_FleetBase):
    """B classical controllers, one batched solve per tick.

    q_nom (B, 7): each instance's initial posture (the scalar controller's
    ``q_nom = obs0.q``); tau0 (B, 7): its initial command (``obs0.tau_bias``);
    R_site_from_pin_ee / p_site_minus_frame_pin: the site calibration
    (crocoddyl_classical.py:199-226; one robot model, so shared).
    device_tick: run the tick's glue (warm start, keep, packing) through the
    library's two fleet kernels instead of torch operations; same results bit
    for bit (tests/test_gpu_fleet_ff.py).  Off by default.  A scheduled tick
    (mpc_update_steps > 1 or apply_command_filter) is torch indexing around
    the selected-instance solve on either path (_tick_sched).
    """

    variant = "classical"
    nx = 14

    def __init__(self, B: int, traj_fn: Traj, config, q_nom, tau0, R_site_from_pin_ee, p_site_minus_frame_pin,
                 device: int = 0, device_tick: bool = False):
        super().__init__(B, traj_fn, config, q_nom, tau0, R_site_from_pin_ee, p_site_minus_frame_pin, device)
        self.device_tick = bool(device_tick)

    def _tick_torch(self, x0, xreg, tref, surface_now, t: float):
        """The tick's glue as torch operations -> us0, xs0, K0, cost, iters, ok, neg_acc, fn0."""
        torch = self.torch
        cfg, B, N, T = self.cfg, self.B, self.N, self.T
        # the tick's inputs go up as ONE copy (packed float64: x0, inst_ref,
        # tau_prev, surface, warm-start mask per instance, then the shared
        # node references), its outputs come down as one (below)
        pk = np.concatenate([x0, xreg, tref, self.tau_prev, surface_now[:, None].astype(np.float64),
                             self.valid[:, None].astype(np.float64)], 1)
        up = torch.from_numpy(np.concatenate([pk.ravel(), self._node_ref(t).ravel()])).to(self.dev)
        pk_d = up[: B * 44].view(B, 44)
        x0_d = pk_d[:, 0:14]
        T["x0"].copy_(x0_d)
        T["node_ref"].copy_(up[B * 44:].view(1, N + 1, 6).expand(B, N + 1, 6))
        T["inst_ref"].copy_(pk_d[:, 14:35])
        T["surface"].copy_(pk_d[:, 42].to(torch.uint8))
        # warm start (_shift_guess, :733-757): [x0] + xs[1:], us[1:] + [us[-1]]; cold: [x0]*(N+1), [tau_prev]*N
        vmask = pk_d[:, 43] != 0
        xs_i = x0_d[:, None, :].expand(B, N + 1, 14).clone()
        xs_i[:, 1:] = torch.where(vmask[:, None, None], self.keep_xs[:, 1:], xs_i[:, 1:])
        tp = pk_d[:, 35:42][:, None, :].expand(B, N, 7)
        us_sh = torch.cat([self.keep_us[:, 1:], self.keep_us[:, -1:]], 1)
        T["xs_init"].copy_(xs_i)
        T["us_init"].copy_(torch.where(vmask[:, None, None], us_sh, tp))
        self.solver.solve_dev(T, maxiter=int(cfg.max_iters), is_feasible=False, stream=self._stream)
        us0_new = T["us"][:, 0]
        fin = torch.isfinite(us0_new).all(1)
        f3 = fin[:, None, None]
        self.keep_xs.copy_(torch.where(f3, T["xs"], self.keep_xs))
        self.keep_us.copy_(torch.where(f3, T["us"], self.keep_us))
        self.keep_K.copy_(torch.where(fin[:, None, None, None], T["K"], self.keep_K))
        f64 = torch.float64
        down = torch.cat([fin.to(f64)[:, None], self.keep_us[:, 0], self.keep_xs[:, 0], self.keep_K[:, 0].reshape(B, 98),
                          T["cost"][:, None], T["iters"].to(f64)[:, None], T["ok"].to(f64)[:, None],
                          T["stats"][:, 9].to(f64)[:, None], T["fn_pred"][:, 0:1]], 1).cpu().numpy()
        self.valid |= down[:, 0] != 0
        us0, xs0, K0 = down[:, 1:8], down[:, 8:22], down[:, 22:120].reshape(B, 7, 14)
        cost = down[:, 120].copy()
        iters = down[:, 121].astype(np.int32)
        ok = down[:, 122] != 0
        neg_acc = down[:, 123].astype(np.int32)  # ascent-direction acceptances of this solve
        return us0, xs0, K0, cost, iters, ok, neg_acc, down[:, 124]

    def compute_control(self, q, v, tau_bias, fn_meas, ee_z, t: float) -> np.ndarray:
        cfg, B = self.cfg, self.B
        q = np.asarray(q, float).reshape(B, 7)
        v = np.asarray(v, float).reshape(B, 7)
        x0 = np.concatenate([q, v], 1)
        surface_now = self._phase(fn_meas, ee_z, t)
        # problem references (_problem_arrays, crocoddyl_classical.py:521-556)
        mode = str(cfg.posture_ref_mode).strip().lower()
        xreg = np.concatenate([self.q_nom, np.zeros((B, 7))], 1) if mode == "q_nom" else x0.copy()
        tref = self._tau_ref(q)
        need = np.ones(B, bool)
        if self.sched:  # either glue path: the scheduled tick is torch indexing
            r = self._tick_sched(x0, np.concatenate([xreg, tref], 1), self.tau_prev, surface_now, t)
            need = r["need"]
            us0, xs0, K0, cost, iters, ok, neg_acc, fn0 = (r[k] for k in ("us0", "xs0", "K0", "cost", "iters", "ok",
                                                                         "neg_acc", "fn0"))
        elif self.device_tick:
            r = self._tick_device(x0, np.concatenate([xreg, tref], 1), self.tau_prev, surface_now, t)
            us0, xs0, K0, cost, iters, ok, neg_acc, fn0 = (r[k] for k in ("us0", "xs0", "K0", "cost", "iters", "ok",
                                                                         "neg_acc", "fn0"))
        else:
            us0, xs0, K0, cost, iters, ok, neg_acc, fn0 = self._tick_torch(x0, xreg, tref, surface_now, t)
        fn_pred = np.where(surface_now, fn0, np.nan)
        # _policy_control (:759-779): u = us[0] + s K[0] (x - xs[0])
        tau_raw = np.where(self.valid[:, None], us0, self.tau_prev)
        if cfg.use_feedback_policy:
            # stacked matmul: per instance the same gemv as the scalar
            # controller's K[0] @ dx (np.einsum sums in another order and
            # differs in the last bit for about half the entries)
            fb = float(cfg.feedback_gain_scale) * np.matmul(K0, (x0 - xs0)[:, :, None])[:, :, 0]
            tau_raw = np.where(self.valid[:, None], tau_raw + fb, tau_raw)
        policy_idx = np.where(self.valid, 0, -1)
        tau_cmd, tau_raw_inf, unstable = self._command(tau_raw, cost, v, tau_bias)
        self.last_info = dict(ok=ok, cost=cost, iters=iters, tau_raw_inf=tau_raw_inf,
                              tau_cmd_inf=np.max(np.abs(tau_cmd), 1), surface_mode=surface_now, unstable=unstable,
                              fn_pred=fn_pred, solved_now=need, policy_idx=policy_idx,
                              neg_accepted=neg_acc)
        if self.sched:
            self._sched_advance(need)
        return tau_cmd


class FleetForceFeedbackMPC(_FleetBase):
    """B force-feedback controllers, one batched solve per tick: per instance
    exactly the logic of ``ForceFeedbackCrocoddylMPC.compute_control``
    (crocoddyl_force_feedback.py:542-695, our B = 1 mirror in controller.py).

    The constructor is ``FleetClassicalMPC``'s; tau0 (B, 7) is each
    instance's initial command (``obs0.tau_cmd``).  The tick runs on the
    library's fleet kernels: one packed upload, warm start, solve, keep, one
    download of the first-knot records.  The torque policy (Eq. 14-18,
    crocoddyl_force_feedback.py:1041-1093) is evaluated on the host from those
    records so that it rounds like the scalar controller.

    ``last_info`` has the classical fleet's keys plus ``tau_des_inf`` and
    ``fn_pred_raw`` (_predicted_normal_force_next_step, NaN where the instance
    is free).  The scalar controller's windowed regression of the logged
    prediction (_align_logged_force_prediction: a least-squares fit per
    instance and lag, a logged quantity only) is not computed by the fleet:
    ``fn_pred`` equals ``fn_pred_raw``.
    """

    variant = "ff"
    nx = 21

    def compute_control(self, q, v, tau_hat, tau_bias, fn_meas, ee_z, t: float) -> np.ndarray:
        """tau_hat (B, 7): the measured torque state, what the scalar
        controller's _tau_state_from_obs takes from its observation."""
        cfg, B = self.cfg, self.B
        q = np.asarray(q, float).reshape(B, 7)
        v = np.asarray(v, float).reshape(B, 7)
        tau_hat = np.asarray(tau_hat, float).reshape(B, 7)
        y0 = np.concatenate([q, v, tau_hat], 1)
        surface_now = self._phase(fn_meas, ee_z, t)
        # problem references (crocoddyl_force_feedback.py:717-721: "x0" -> y0[:14], else q_nom)
        if str(cfg.posture_ref_mode).strip().lower() == "x0":
            xreg = y0[:, :14].copy()
        else:
            xreg = np.concatenate([self.q_nom, np.zeros((B, 7))], 1)
        # cold start: w = y0[14:21] (_cold_control)
        tick = self._tick_sched if self.sched else self._tick_device
        r = tick(y0, np.concatenate([xreg, self._tau_ref(q)], 1), tau_hat, surface_now, t)
        need = r["need"] if self.sched else np.ones(B, bool)
        cost, xs0, xs1, K0 = r["cost"], r["xs0"], r["xs1"], r["K0"]
        dt_mpc = float(cfg.dt)
        alpha = ff_filter_alpha(cfg, self.dt_ocp)
        eps_pol = float(np.clip(dt_mpc / self.dt_ocp, 0.0, 1.0))  # _policy_epsilon
        # _predicted_normal_force_next_step (:1219-1243)
        f0, f1 = np.abs(r["fn0"]), np.abs(r["fn1"])
        if self.N == 1 or dt_mpc >= self.dt_ocp - 1.0e-9:
            f01 = f0
        else:
            f01 = (1.0 - eps_pol) * f0 + eps_pol * f1
        fn_next = f0 if self.N == 1 else np.where(~np.isfinite(f0), f1, np.where(~np.isfinite(f1), f0, f01))
        fn_pred_raw = np.where(surface_now & np.isfinite(fn_next), fn_next, np.nan)
        # _policy_control, Eq. 14-18 (:1041-1093); instances without a kept solution command tau_hat
        eps = eps_pol if bool(cfg.ff_use_tau_interpolation) else 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            tau0, tau1 = xs0[:, 14:21], xs1[:, 14:21]
            tau_pol = tau0 + eps * (tau1 - tau0)
            if cfg.use_feedback_policy:
                # stacked matmul: per instance the scalar controller's gemv, bit for bit
                Kx, Ktau = K0[:, :, :14], K0[:, :, 14:21]
                x_err = xs0[:, :14] - y0[:, :14]
                tau_err = tau0 - y0[:, 14:21]
                I7 = np.eye(7)
                K_tilde_x = eps * (1.0 - alpha) * Kx
                K_tilde_tau = I7 + eps * (1.0 - alpha) * (Ktau - I7)
                tau_pol = tau_pol + float(cfg.feedback_gain_scale) * (
                    np.matmul(K_tilde_x, x_err[:, :, None])[:, :, 0] + np.matmul(K_tilde_tau, tau_err[:, :, None])[:, :, 0])
        tau_des = np.where(self.valid[:, None], tau_pol, tau_hat)
        policy_idx = np.where(self.valid, 0, -1)
        tau_raw = tau_des.copy()
        if bool(cfg.ff_inverse_actuation_model):
            a_c = ff_filter_alpha(cfg, dt_mpc)  # _ff_alpha_ctrl
            tau_raw = (tau_raw - a_c * tau_hat) / max(1.0e-6, 1.0 - a_c)
        tau_des_inf = np.max(np.abs(tau_des), 1)
        tau_cmd, tau_raw_inf, unstable = self._command(tau_raw, cost, v, tau_bias)
        self.last_info = dict(ok=r["ok"], cost=cost, iters=r["iters"], tau_des_inf=tau_des_inf, tau_raw_inf=tau_raw_inf,
                              tau_cmd_inf=np.max(np.abs(tau_cmd), 1), surface_mode=surface_now, unstable=unstable,
                              fn_pred=fn_pred_raw.copy(), fn_pred_raw=fn_pred_raw, solved_now=need,
                              policy_idx=policy_idx, neg_accepted=r["neg_acc"])
        if self.sched:
            self._sched_advance(need)
        return tau_cmd


def site_calibration(obs0):
    """_calibrate_site_rotation / _calibrate_site_position_offset
    (crocoddyl_classical.py:199-226; controller._MPCBase) from one observation."""
    R_pin_ee, p_pin_ee = _abi.frame_placement(np.asarray(obs0.q, float))
    R_site = R_pin_ee.T @ R.R_MJ_FROM_PIN.T @ _quat_wxyz_to_R(obs0.ee_quat)
    p_off = R.R_MJ_FROM_PIN.T @ np.asarray(obs0.ee_pos, float).reshape(3) - p_pin_ee
    return R_site, p_off


def _sweep_instances(scenarios: Sequence[str], seeds: int):
    from .closed_loop import scenario_seed, scenario_settings

    names, tilt, scale, seed = [], [], [], []
    for s in scenarios:
        st = scenario_settings(s)
        for k in range(seeds):
            names.append(s)
            tilt.append(st["tilt_deg"])
            scale.append(st["torque_scale"])
            seed.append(scenario_seed(s) * 100003 + k)
    return np.array(names), np.array(tilt), np.array(scale), np.array(seed)


def sweep_plant_physics(seed, plant_spread) -> list:
    """run_sweep's plant_spread = (ds, dd): one PlantPhysics per instance seed,
    the contact time constant 0.02 (1 + ds u0) and every joint's damping
    1.0 (1 + dd u1), u = default_rng([seed_b, 2]).uniform(-1, 1, 2)."""
    ds, dd = plant_spread
    out = []
    for s in seed:
        u = np.random.default_rng([int(s), 2]).uniform(-1.0, 1.0, 2)
        out.append(PlantPhysics(damping=JOINT_DAMPING * (1.0 + dd * u[1]), solref=(0.02 * (1.0 + ds * u[0]), 1.0)))
    return out


def sweep_uncertainty_config(scenario: str, seed: int, dt: float, uncertainty_spread=None):
    """The scenario's injector config (None without one) and, with run_sweep's
    uncertainty_spread = (dn, D), its profile varied from g = default_rng(
    [seed, 3]): the three sigmas scaled by 1 + dn g.uniform(-1, 1), then the
    delays d_obs, d_cmd = g.integers(0, D + 1, 2) ticks of dt, written as
    delta_obs_cycles / delta_cmd_s so that delay_steps returns them."""
    cfg = config_for_scenario(str(scenario), seed=int(seed))
    if cfg is None or uncertainty_spread is None:
        return cfg
    dn, D = uncertainty_spread
    g = np.random.default_rng([int(seed), 3])
    f = 1.0 + dn * g.uniform(-1.0, 1.0)
    d_obs, d_cmd = (int(x) for x in g.integers(0, int(D) + 1, 2))
    cfg = dataclasses.replace(cfg, sigma_q=cfg.sigma_q * f, sigma_dq=cfg.sigma_dq * f, sigma_tau=cfg.sigma_tau * f,
                              delta_obs_cycles=int(round(d_obs * dt / 1.0e-3)), delta_cmd_s=d_cmd * dt)
    if delay_steps(cfg, dt) != (d_obs, d_cmd):
        raise ValueError(f"run_sweep: a delay of ({d_obs}, {d_cmd}) ticks of {dt} s is no whole number of 1 kHz cycles")
    return cfg


def _inject_profile(ucfgs, dt: float):
    """(B, 2) delays in ticks and (B, 3) sigmas of a list of configs; -1 / NaN for None."""
    delay, sigma = np.full((len(ucfgs), 2), -1, np.int64), np.full((len(ucfgs), 3), np.nan)
    for b, c in enumerate(ucfgs):
        if c is not None:
            delay[b], sigma[b] = delay_steps(c, dt), (c.sigma_q, c.sigma_dq, c.sigma_tau)
    return delay, sigma


def check_weight_spread(weight_spread) -> dict:
    """run_sweep's weight_spread, checked: {name: (lo, hi)} with names from
    config.COST_WEIGHT_NAMES and finite 0 < lo <= hi (ValueError otherwise), as
    floats in the names' sorted order."""
    if not isinstance(weight_spread, dict) or not weight_spread:
        raise ValueError(f"run_sweep: weight_spread is a dict {{name: (lo, hi)}}, not {weight_spread!r}")
    out = {}
    for name in sorted(weight_spread):
        if name not in COST_WEIGHT_NAMES:
            raise ValueError(f"run_sweep: weight_spread: unknown cost weight {name!r} "
                             f"(one of {', '.join(COST_WEIGHT_NAMES)})")
        rng_ = tuple(float(x) for x in np.atleast_1d(weight_spread[name]))
        if len(rng_) != 2 or not all(np.isfinite(rng_)) or not 0.0 < rng_[0] <= rng_[1]:
            raise ValueError(f"run_sweep: weight_spread[{name!r}] is (lo, hi), 0 < lo <= hi, not {weight_spread[name]!r}")
        out[name] = rng_
    return out


def sweep_cost_weights(seed, weight_spread: dict) -> dict:
    """The sweep's per-instance cost weights: {name: (B,) values}, instance b's
    value of `name` lo (hi / lo)^((1 + u) / 2) with u = one uniform in [-1, 1]
    per name, in the names' sorted order, from default_rng([seed_b, 5]) -- a
    generator of its own, so no other draw of the sweep moves."""
    spread = check_weight_spread(weight_spread)
    names = list(spread)
    out = {name: np.zeros(len(seed)) for name in names}
    for b, s_ in enumerate(seed):
        u = np.random.default_rng([int(s_), 5]).uniform(-1.0, 1.0, len(names))
        for i, name in enumerate(names):
            lo_, hi_ = spread[name]
            out[name][b] = lo_ * (hi_ / lo_) ** (0.5 * (1.0 + u[i]))
    return out


def check_limit_spread(limit_spread) -> Tuple[float, float]:
    """run_sweep's limit_spread, checked: (lo, hi), finite, 0 < lo <= hi (ValueError otherwise)."""
    try:
        rng_ = tuple(float(x) for x in limit_spread)
    except TypeError:
        rng_ = ()
    if len(rng_) != 2 or not all(np.isfinite(rng_)) or not 0.0 < rng_[0] <= rng_[1]:
        raise ValueError(f"run_sweep: limit_spread is (lo, hi), 0 < lo <= hi, not {limit_spread!r}")
    return rng_


def sweep_limit_scales(seed, limit_spread) -> np.ndarray:
    """The sweep's per-instance torque-limit scales (B,): instance b's scale is
    lo (hi / lo)^((1 + u) / 2), log-uniform in [lo, hi], with u one uniform in
    [-1, 1] from default_rng([seed_b, 6]) -- a generator of its own, so no
    other draw of the sweep moves."""
    lo_, hi_ = check_limit_spread(limit_spread)
    out = np.zeros(len(seed))
    for b, s_ in enumerate(seed):
        u = np.random.default_rng([int(s_), 6]).uniform(-1.0, 1.0)
        out[b] = lo_ * (hi_ / lo_) ** (0.5 * (1.0 + u))
    return out


def check_payload_spread(payload_spread) -> Tuple[float, float]:
    """run_sweep's payload_spread, checked: (m_lo, m_hi) in kg, finite, 0 <= m_lo <= m_hi (ValueError otherwise)."""
    try:
        rng_ = tuple(float(x) for x in payload_spread)
    except TypeError:
        rng_ = ()
    if len(rng_) != 2 or not all(np.isfinite(rng_)) or not 0.0 <= rng_[0] <= rng_[1]:
        raise ValueError(f"run_sweep: payload_spread is (m_lo, m_hi), 0 <= m_lo <= m_hi, not {payload_spread!r}")
    return rng_


def sweep_payload_masses(seed, payload_spread) -> np.ndarray:
    """The sweep's per-instance payload masses (B,) in the controllers' models:
    instance b's is m_lo + (m_hi - m_lo) u, with u one uniform in [0, 1] from
    default_rng([seed_b, 7]) -- a generator of its own, so no other draw of
    the sweep moves."""
    lo_, hi_ = check_payload_spread(payload_spread)
    out = np.zeros(len(seed))
    for b, s_ in enumerate(seed):
        u = np.random.default_rng([int(s_), 7]).uniform(0.0, 1.0)
        out[b] = lo_ + (hi_ - lo_) * u
    return out


def sweep_plant_payload_masses(seed, plant_payload_spread) -> np.ndarray:
    """The sweep's per-instance payload masses (B,) on the plants' arms:
    instance b's is m_lo + (m_hi - m_lo) u, with u one uniform in [0, 1] from
    default_rng([seed_b, 8]) -- a generator of its own, so no other draw of
    the sweep moves (sweep_payload_masses' included)."""
    lo_, hi_ = check_payload_spread(plant_payload_spread)
    out = np.zeros(len(seed))
    for b, s_ in enumerate(seed):
        u = np.random.default_rng([int(s_), 8]).uniform(0.0, 1.0)
        out[b] = lo_ + (hi_ - lo_) * u
    return out


def payload_models(masses) -> list:
    """One robot.LinkModel per mass: the nominal arm with a point payload at the EE offset on link 7."""
    return [R.LinkModel().with_payload(float(m), R.EE_P) for m in masses]


def run_sweep(scenarios: Sequence[str] = ("flat", "tilted_5", "tilted_10", "tilted_15", "actuation_uncertainty"),
              seeds: int = 256, total_time: float = 4.0, rank: int = 0, world: int = 1, device: int = 0,
              q_sigma: float = 0.02, verbose: bool = True, record: Sequence[int] = (),
              neg_step_rule: int = 0, variant: str = "classical", device_tick: bool = False,
              device_loop: bool = False, device_noise: Optional[str] = None, solve_period: int = 1,
              command_filter: bool = False, device_refs: bool = False,
              task_spread: Optional[Tuple[float, float]] = None, stagger: int = 0,
              device_summary: bool = False, keep_logs: bool = True,
              plant_spread: Optional[Tuple[float, float]] = None,
              uncertainty_spread: Optional[Tuple[float, int]] = None,
              force_spread: Optional[Tuple[float, float]] = None, force_ramp: Optional[float] = None,
              weight_spread: Optional[dict] = None,
              limit_spread: Optional[Tuple[float, float]] = None,
              payload_spread: Optional[Tuple[float, float]] = None,
              plant_payload_spread: Optional[Tuple[float, float]] = None, payload_known: bool = False,
              tilt_known: bool = False) -> dict:
    """Closed-loop sweep of len(scenarios) * seeds instances; this rank runs
    its contiguous shard.  Returns per-instance summary arrays (this shard).
    record: shard-local instance indices whose controller inputs (the plant
    record as the controller sees it, after any measurement noise) and
    commanded torques are kept per tick, with what a scalar controller needs
    to replay them (the task, the config, the start states).
    neg_step_rule: the solver's ascent-direction comparator (include/ffddp.h
    FFDDP_NEGSTEP_*; 0 = Crocoddyl's, the reference's behaviour).
    variant: "classical" (classical_benchmark_config, FleetClassicalMPC) or
    "ff" (ff_benchmark_config, FleetForceFeedbackMPC).  The force-feedback
    controllers' measured torque state tau_hat is, for instances with an
    uncertainty injector, the injector's filtered torque measurement, and for
    the others the plant's low-pass of the applied command (PandaTablePlant's
    tau_meas_act_filt: alpha 0.2, zero at reset, one update per observation);
    record then also keeps tau_hat per tick.
    device_tick: FleetClassicalMPC(device_tick=...); the ff fleet always
    ticks on the device.
    device_loop: run the whole closed loop on the device (fleet_loop.
    DeviceFleetLoop: no host synchronisation per tick, the logs come down once
    at the end) and build the same summary from them.  Not with ``record``
    (NotImplementedError); ``controller_s`` is None, the ticks are not timed
    apart.
    device_noise (with device_loop): where the device injector's normals come
    from -- "numpy": a table drawn ahead from the instances' Generators, the
    host path's perturbations exactly; "philox": generated on the device, no
    table (another stream).  The summary then also carries ``inject_a`` /
    ``inject_b`` (the injectors' gain and bias, NaN without one).  None: a
    scenario with an injector is refused (NotImplementedError).
    solve_period, command_filter: the controllers' mpc_update_steps (solve
    every solve_period-th tick, the feedback policy in between) and
    apply_command_filter; on the host path they go into the configuration, on
    the device path to the loop.  The summary's ``solved_ticks`` counts each
    instance's ticks with a solve.
    device_refs, task_spread, stagger (with device_loop only, NotImplementedError
    otherwise: the host fleets keep their single traj_fn): the instances'
    references are sampled on the device from per-instance task records
    (DeviceFleetLoop(tasks=...)) instead of a host table.  device_refs alone
    runs the sweep's one task that way.  task_spread = (dr, dw) varies the
    task: instance radius = 0.10 (1 + dr u1), omega = 1.5 (1 + dw u2) with u
    uniform in [-1, 1] from default_rng([seed_b, 1]) (the q0 draws do not
    move).  stagger = S delays instance b (its index in the whole sweep) by
    (b mod S) dt.  Either implies device_refs.  The summary's reference
    position and contact-phase window are then per instance, in task time.
    device_summary, keep_logs (with device_loop only, NotImplementedError
    otherwise): ``per_instance`` and ``solved_ticks`` come from sums the loop
    accumulates on the device per tick (DeviceFleetLoop(metrics=True),
    runlog.metrics_from_accumulators) instead of from the downloaded logs; the
    sums run in tick order where numpy's means sum pairwise, so the two
    summaries agree to summation rounding.  keep_logs = False (needs
    device_summary, ValueError otherwise) drops the per-tick logs altogether
    (logs=False): the run's memory no longer grows with its length and the
    (ticks, B) outputs ``solved`` and ``surface`` are absent.
    plant_spread, uncertainty_spread (host and device path alike): the plant's
    physics and the injectors' profiles per instance.  plant_spread = (ds, dd),
    each in [0, 0.9]: the contact time constant 0.02 (1 + ds u0) -- the
    table's stiffness; it stays at or above twice the 1 ms physics step,
    MuJoCo's floor for solref -- and every joint's damping 1.0 (1 + dd u1),
    u uniform in [-1, 1] from default_rng([seed_b, 2]).  uncertainty_spread =
    (dn, D), dn in [0, 1), D an integer 0..16, for the instances whose scenario
    has an injector: the three sigmas scaled by 1 + dn g.uniform(-1, 1), then
    the delays d_obs, d_cmd = g.integers(0, D + 1, 2) control ticks, g =
    default_rng([seed_b, 3]).  The q0 and task draws do not move.  The
    summary carries ``plant_rows`` (B, PLANT_ROW_W), ``inject_delay`` (B, 2)
    and ``inject_sigma`` (B, 3) (-1 / NaN without an injector).
    force_spread, force_ramp (with device_loop only, NotImplementedError
    otherwise: the host fleets track the configuration's fn_des): each
    instance's own desired normal force (DeviceFleetLoop(force_profiles=...)).
    force_spread = (f_lo, f_hi), 0 <= f_lo <= f_hi: instance b's setpoint f1 =
    f_lo + (f_hi - f_lo) (1 + u) / 2, u uniform in [-1, 1] from
    default_rng([seed_b, 4]) (the other draws do not move).  force_ramp = T > 0
    (needs force_spread): the reference starts at f_lo and ramps to f1 over T
    seconds from the end of the contact hold, in the instance's task time;
    T = 0 or None: f1 from the start.  The summary's ``avg_abs_force_err`` is
    then against each instance's own reference at every sample, from the logs
    and from the device accumulators alike, and ``force_rec`` (B, 4) carries
    the profiles (f0, f1, t_on, t_ramp).
    weight_spread (with device_loop only, NotImplementedError otherwise: the
    host fleets solve with the configuration's weights): the controller's own
    tuning per instance (DeviceFleetLoop(cost_weights=...)).  weight_spread =
    {name: (lo, hi), ...}, names from config.COST_WEIGHT_NAMES, 0 < lo <= hi:
    instance b's value of `name` is lo (hi / lo)^((1 + u) / 2), log-uniform,
    with one u uniform in [-1, 1] per name, in the names' sorted order, from
    default_rng([seed_b, 5]) (sweep_cost_weights; the other draws do not
    move).  The summary carries ``weights`` ({name: (B,) drawn values}) and
    ``cost_rows`` (B, COST_W), the rows the solves took.
    limit_spread (with device_loop only, NotImplementedError otherwise: the
    host fleets solve within the configuration's limits): each instance's own
    torque authority (DeviceFleetLoop(torque_limits=...)).  limit_spread =
    (lo, hi), 0 < lo <= hi: instance b's tau_limits are the configuration's
    times lo (hi / lo)^((1 + u) / 2), log-uniform, u uniform in [-1, 1] from
    default_rng([seed_b, 6]) (sweep_limit_scales; the other draws do not
    move).  The summary carries ``limit_scale`` (B,), the drawn scales, and
    ``tau_limits`` (B, 7), the limits the solves and the command clip took.
    payload_spread (with device_loop only, NotImplementedError otherwise: the
    host fleets plan with the nominal model): each instance's controller plans
    with its own rigid-body model (DeviceFleetLoop(link_models=...)), the
    nominal arm with a point payload at the EE offset
    (robot.LinkModel.with_payload); the plant is not changed, so this is the
    model-mismatch sweep.  payload_spread = (m_lo, m_hi) in kg: instance b's
    payload mass is m_lo + (m_hi - m_lo) u, u uniform in [0, 1] from
    default_rng([seed_b, 7]) (sweep_payload_masses; the other draws do not
    move).  The summary carries ``payload_mass`` (B,), the drawn masses.
    plant_payload_spread, payload_known: the arm itself carries a payload, and
    the controller may or may not know it.  plant_payload_spread = (m_lo, m_hi)
    in kg, checked as payload_spread is (host and device path alike: both step
    a BatchedPlant): instance b's plant integrates with the nominal arm plus a
    point payload at the EE offset on link 7
    (BatchedPlant(link_models=...) / DeviceFleetLoop(plant_link_models=...)),
    of mass m_lo + (m_hi - m_lo) u, u uniform in [0, 1] from
    default_rng([seed_b, 8]) (sweep_plant_payload_masses; the other draws do
    not move).  payload_known = True (needs plant_payload_spread, ValueError
    otherwise; with device_loop only, NotImplementedError otherwise; not
    together with payload_spread, ValueError) gives each instance's controller
    the same model (DeviceFleetLoop(link_models=...)).  A plant step that
    fails under a payload is a result (``plant_fail``), as under plant_spread.
    The summary carries ``plant_payload_mass`` (B,), the drawn masses, and
    ``payload_known``.
    tilt_known (with device_loop only, NotImplementedError otherwise: the host
    fleets plan under the nominal mount): the controllers are told the table's
    tilt, which the scenarios otherwise hide from them.  Instance b plans under
    robot.Mount.table_tilt(tilt_b) (DeviceFleetLoop(mounts=...); None for tilt
    0), that is in the table's frame, where the table is level: its circle lies
    on the table, and its logs and metrics are read in that frame, while a
    hidden-tilt instance tracks the world-horizontal circle and is scored in
    the world frame.  The plant is not changed.  It combines with every other
    spread.  The summary carries ``tilt_known``."""
    variant = str(variant).strip().lower()
    if variant not in ("classical", "ff"):
        raise ValueError(f"run_sweep: unknown variant {variant!r}")
    if isinstance(solve_period, bool) or int(solve_period) != solve_period or int(solve_period) < 1:
        raise ValueError(f"run_sweep: solve_period must be an integer >= 1, not {solve_period!r}")
    if not isinstance(command_filter, (bool, np.bool_)) and command_filter not in (0, 1):
        raise ValueError(f"run_sweep: command_filter must be a flag, not {command_filter!r}")
    solve_period, command_filter = int(solve_period), bool(command_filter)
    if isinstance(stagger, bool) or int(stagger) != stagger or int(stagger) < 0:
        raise ValueError(f"run_sweep: stagger must be an integer >= 0, not {stagger!r}")
    stagger = int(stagger)
    if task_spread is not None:
        task_spread = tuple(float(x) for x in task_spread)
        if len(task_spread) != 2 or not all(0.0 <= x < 1.0 for x in task_spread):
            raise ValueError(f"run_sweep: task_spread is (dr, dw), each in [0, 1), not {task_spread!r}")
    if plant_spread is not None:
        plant_spread = tuple(float(x) for x in plant_spread)
        if len(plant_spread) != 2 or not all(0.0 <= x <= 0.9 for x in plant_spread):
            raise ValueError(f"run_sweep: plant_spread is (ds, dd), each in [0, 0.9], not {plant_spread!r}")
    if uncertainty_spread is not None:
        uncertainty_spread = tuple(uncertainty_spread)
        ok = len(uncertainty_spread) == 2
        if ok:
            dn, D = uncertainty_spread
            ok = (not isinstance(D, (bool, np.bool_)) and isinstance(D, (int, np.integer)) and 0 <= int(D) <= 16
                  and isinstance(dn, (int, float, np.integer, np.floating)) and 0.0 <= float(dn) < 1.0)
        if not ok:
            raise ValueError("run_sweep: uncertainty_spread is (dn, D), dn in [0, 1) and D an integer 0..16, "
                             f"not {uncertainty_spread!r}")
        uncertainty_spread = (float(dn), int(D))
    if force_ramp is not None and force_spread is None:
        raise ValueError("run_sweep: force_ramp needs force_spread")
    if force_spread is not None:
        force_spread = tuple(float(x) for x in force_spread)
        if len(force_spread) != 2 or not all(np.isfinite(force_spread)) or not 0.0 <= force_spread[0] <= force_spread[1]:
            raise ValueError(f"run_sweep: force_spread is (f_lo, f_hi), 0 <= f_lo <= f_hi, not {force_spread!r}")
        force_ramp = 0.0 if force_ramp is None else float(force_ramp)
        if not (np.isfinite(force_ramp) and force_ramp >= 0.0):
            raise ValueError(f"run_sweep: force_ramp must be >= 0, not {force_ramp!r}")
        if not device_loop:
            raise NotImplementedError("run_sweep: force_spread and force_ramp need device_loop=True "
                                      "(the host fleets track the configuration's fn_des)")
    if weight_spread is not None:
        weight_spread = check_weight_spread(weight_spread)
        if not device_loop:
            raise NotImplementedError("run_sweep: weight_spread needs device_loop=True "
                                      "(the host fleets solve with the configuration's weights)")
    if limit_spread is not None:
        limit_spread = check_limit_spread(limit_spread)
        if not device_loop:
            raise NotImplementedError("run_sweep: limit_spread needs device_loop=True "
                                      "(the host fleets solve within the configuration's limits)")
    if not isinstance(payload_known, (bool, np.bool_)) and payload_known not in (0, 1):
        raise ValueError(f"run_sweep: payload_known must be a flag, not {payload_known!r}")
    payload_known = bool(payload_known)
    if plant_payload_spread is not None:
        try:
            plant_payload_spread = check_payload_spread(plant_payload_spread)
        except ValueError:
            raise ValueError("run_sweep: plant_payload_spread is (m_lo, m_hi), 0 <= m_lo <= m_hi, "
                             f"not {plant_payload_spread!r}") from None
    if payload_known:
        if plant_payload_spread is None:
            raise ValueError("run_sweep: payload_known needs plant_payload_spread")
        if payload_spread is not None:
            raise ValueError("run_sweep: payload_known gives the controllers the plants' payloads; "
                             "not together with payload_spread")
        if not device_loop:
            raise NotImplementedError("run_sweep: payload_known needs device_loop=True "
                                      "(the host fleets plan with the nominal model)")
    if not isinstance(tilt_known, (bool, np.bool_)) and tilt_known not in (0, 1):
        raise ValueError(f"run_sweep: tilt_known must be a flag, not {tilt_known!r}")
    tilt_known = bool(tilt_known)
    if tilt_known and not device_loop:
        raise NotImplementedError("run_sweep: tilt_known needs device_loop=True "
                                  "(the host fleets plan under the nominal mount)")
    if payload_spread is not None:
        payload_spread = check_payload_spread(payload_spread)
        if not device_loop:
            raise NotImplementedError("run_sweep: payload_spread needs device_loop=True "
                                      "(the host fleets plan with the nominal model)")
    device_refs = bool(device_refs) or task_spread is not None or stagger > 0
    if device_refs and not device_loop:
        raise NotImplementedError("run_sweep: device_refs, task_spread and stagger need device_loop=True "
                                  "(the host fleets take one traj_fn)")
    device_summary, keep_logs = bool(device_summary), bool(keep_logs)
    if (device_summary or not keep_logs) and not device_loop:
        raise NotImplementedError("run_sweep: device_summary and keep_logs need device_loop=True "
                                  "(the host loop builds its summary as it goes)")
    if not keep_logs and not device_summary:
        raise ValueError("run_sweep: keep_logs=False needs device_summary=True")
    if device_noise is not None:
        if device_noise not in ("numpy", "philox"):
            raise ValueError(f"run_sweep: unknown device_noise {device_noise!r} (numpy or philox)")
        if not device_loop:
            raise ValueError("run_sweep: device_noise needs device_loop=True")
    if device_loop:
        injected = [s for s in scenarios if config_for_scenario(str(s), seed=0) is not None]
        if injected and device_noise is None:
            raise NotImplementedError(f"run_sweep(device_loop=True): the uncertainty injector of {injected} "
                                      "runs on the device only with device_noise=\"numpy\" or \"philox\"")
        if len(record):
            raise NotImplementedError("run_sweep(device_loop=True): record is not supported")
    names, tilt, scale, seed = _sweep_instances(scenarios, seeds)
    n_all = len(names)
    per = (n_all + world - 1) // world
    lo, hi = rank * per, min(n_all, (rank + 1) * per)
    names, tilt, scale, seed = names[lo:hi], tilt[lo:hi], scale[lo:hi], seed[lo:hi]
    B = len(names)
    # nominal geometry and trajectory: planned from the keyframe's EE (run_classical.py:209-264)
    nominal = PandaTablePlant(n_substeps=5, timestep=0.001, device=device)
    obs0 = nominal.reset("neutral")
    z_top = float(TABLE_CENTER[2] + TABLE_HALF_Z)
    z_contact = z_top + TOOL_RADIUS - 8.0e-3
    center = np.array([TABLE_CENTER[0], TABLE_CENTER[1], z_contact])
    base = make_approach_then_circle(center=center, radius=0.10, omega=1.5, z_pre=z_contact + 0.05,
                                     z_contact=z_contact, t_approach=0.55, ee_start=obs0.ee_pos.copy(), t_pre=0.25)
    t_cp = 0.8

    traj = with_contact_hold(base, t_cp, 0.2)

    R_site_from_pin_ee, p_off = site_calibration(obs0)
    nominal.close()
    q0 = np.stack([R.Q_NEUTRAL + np.random.default_rng(int(s)).normal(0.0, q_sigma, 7) for s in seed])
    dt_ctrl = 0.001 * 5  # BatchedPlant.dt
    physics = sweep_plant_physics(seed, plant_spread) if plant_spread is not None else None
    plant_payload = sweep_plant_payload_masses(seed, plant_payload_spread) if plant_payload_spread else None
    sweep_cfgs = [sweep_uncertainty_config(str(names[b]), int(seed[b]), dt_ctrl, uncertainty_spread) for b in range(B)]
    if device_loop:
        ucfgs = None
        if device_noise is not None:  # per instance, as the host path below
            ucfgs = sweep_cfgs
        tasks = None
        if device_refs:
            dr, dw = task_spread if task_spread is not None else (0.0, 0.0)
            tasks = []
            for b in range(B):
                u = np.random.default_rng([int(seed[b]), 1]).uniform(-1.0, 1.0, 2) if task_spread is not None else (0.0, 0.0)
                tasks.append(FleetTask(center=center, radius=0.10 * (1.0 + dr * u[0]), omega=1.5 * (1.0 + dw * u[1]),
                                       z_contact=z_contact, t_approach=0.55, t_pre=0.25, ee_start=obs0.ee_pos.copy(),
                                       z_pre=z_contact + 0.05, t_contact_phase=t_cp, t_hold=0.2,
                                       delay=((lo + b) % stagger) * (0.001 * 5) if stagger else 0.0))  # BatchedPlant.dt
        profiles = None
        if force_spread is not None:
            f_lo, f_hi = force_spread
            profiles = []
            for b in range(B):
                u = np.random.default_rng([int(seed[b]), 4]).uniform(-1.0, 1.0)
                f1 = f_lo + (f_hi - f_lo) * (0.5 * (1.0 + u))
                profiles.append(ForceProfile(f_lo, f1, t_on=t_cp + 0.2, t_ramp=force_ramp) if force_ramp > 0.0
                                else ForceProfile(f1, f1))
        out = _run_sweep_device(variant, q0, tilt, scale, traj, z_contact, (R_site_from_pin_ee, p_off), total_time,
                                neg_step_rule, device, t_cp, verbose, ucfgs, device_noise, solve_period,
                                command_filter, tasks, device_summary, keep_logs, physics,
                                allow_plant_fail=(plant_spread is not None or uncertainty_spread is not None
                                                  or plant_payload is not None),
                                force_profiles=profiles,
                                weights=sweep_cost_weights(seed, weight_spread) if weight_spread else None,
                                limit_scale=sweep_limit_scales(seed, limit_spread) if limit_spread else None,
                                payload_mass=sweep_payload_masses(seed, payload_spread) if payload_spread else None,
                                plant_payload_mass=plant_payload, payload_known=payload_known, tilt_known=tilt_known)
        out.update(names=names, seed=seed, shard=(lo, hi), n_all=n_all)
        return out
    plant = BatchedPlant(B, timestep=0.001, n_substeps=5, device=device, physics=physics,
                         link_models=None if plant_payload is None else payload_models(plant_payload))
    plant.q = q0.copy()
    plant.v = np.zeros((B, 7))
    plant.set_tilt(0.0)
    plant.step(np.zeros((B, 7)), integrate=False)  # mj_forward at the start state
    tau0 = plant.obs[:, 14:21].copy()
    if variant == "ff":
        cfg = ff_benchmark_config(plant.dt, z_contact, neg_step_rule=neg_step_rule)
        cfg.mpc_update_steps, cfg.apply_command_filter = solve_period, command_filter
        mpc = FleetForceFeedbackMPC(B, traj, cfg, q_nom=q0, tau0=np.zeros((B, 7)),
                                    R_site_from_pin_ee=R_site_from_pin_ee, p_site_minus_frame_pin=p_off, device=device)
    else:
        cfg = classical_benchmark_config(plant.dt, z_contact, neg_step_rule=neg_step_rule)
        cfg.mpc_update_steps, cfg.apply_command_filter = solve_period, command_filter
        mpc = FleetClassicalMPC(B, traj, cfg, q_nom=q0, tau0=tau0, R_site_from_pin_ee=R_site_from_pin_ee,
                                p_site_minus_frame_pin=p_off, device=device, device_tick=device_tick)
    plant.set_tilt(tilt)  # hidden from the controllers
    plant.step(tau0 * 0.0, integrate=False)
    # the scenarios' uncertainty injectors, batched (BatchedUncertaintyInjector:
    # draw for draw the per-instance ScenarioUncertaintyInjector)
    ucfg = dict(enumerate(sweep_cfgs))
    inj_idx = np.array([b for b in range(B) if ucfg[b] is not None], dtype=np.int64)
    inj = BatchedUncertaintyInjector(dt=plant.dt, nu=7, configs=[ucfg[b] for b in inj_idx]) if inj_idx.size else None
    steps = int(total_time / plant.dt)
    series = {k: np.zeros((steps, B)) for k in ("t", "err_tan", "err_3d", "fn_meas", "contact")}
    # solver health per instance: ticks on the instability fallback
    # (crocoddyl_classical.py:392-404; solver_unstable, run_classical.py:480)
    # ticks whose solve accepted an ascent-direction step and ticks whose
    # solve returned ok = False
    unstable_ticks = np.zeros(B)
    neg_ticks = np.zeros(B)
    not_ok_ticks = np.zeros(B)
    solved_ticks = np.zeros(B)
    rec_idx = [int(i) for i in record]
    rec_obs = np.zeros((steps, len(rec_idx), plant.obs.shape[1]))
    rec_tau = np.zeros((steps, len(rec_idx), 7))
    rec_tau_hat = np.zeros((steps, len(rec_idx), 7))
    rec_t = np.zeros(steps)
    # the ff variant's torque measurement without an injector (plant.py
    # PandaTablePlant.get_observation: _filt_act).  The plant filters the
    # torque it was stepped with, so this filters tau_app (= tau * scale), not
    # tau; the scenarios that scale the command all carry an injector, whose
    # own measurement replaces this one, so for them the two are the same.
    filt_act = np.zeros((B, 7))
    tau_app = np.zeros((B, 7))
    lpf = 0.2
    obs = plant.obs.copy()
    t = 0.0
    wall0 = time.perf_counter()
    ctrl_s = 0.0
    for k in range(steps):
        q, v, bias = obs[:, 0:7], obs[:, 7:14], obs[:, 14:21]
        fn, ee = obs[:, 46] * (obs[:, 47] > 0.5), obs[:, 28:31]
        if inj is not None:
            q, v = q.copy(), v.copy()
            q[inj_idx], v[inj_idx] = inj.observation_for_controller(q[inj_idx], v[inj_idx])
        if variant == "ff":
            filt_act = (1.0 - lpf) * filt_act + lpf * tau_app
            tau_hat = filt_act.copy()
            if inj is not None:
                tau_hat[inj_idx] = inj.tau_hat_filt
            tc = time.perf_counter()
            tau = mpc.compute_control(q, v, tau_hat, bias, fn, ee[:, 2], t)
        else:
            tc = time.perf_counter()
            tau = mpc.compute_control(q, v, bias, fn, ee[:, 2], t)
        ctrl_s += time.perf_counter() - tc
        unstable_ticks += mpc.last_info["unstable"]
        neg_ticks += mpc.last_info["neg_accepted"] > 0
        not_ok_ticks += ~mpc.last_info["ok"]
        solved_ticks += mpc.last_info["solved_now"]
        if rec_idx:
            rec_t[k] = t
            rec_obs[k] = obs[rec_idx]
            rec_obs[k][:, 0:7], rec_obs[k][:, 7:14] = q[rec_idx], v[rec_idx]
            rec_tau[k] = tau[rec_idx]
            if variant == "ff":
                rec_tau_hat[k] = tau_hat[rec_idx]
        tau_app = tau * scale
        if inj is not None:
            tau_app[inj_idx] = inj.command_for_plant(tau[inj_idx])
        obs = plant.step(tau_app).copy()
        t += plant.dt
        p_ref, _, _ = traj(t)
        err = obs[:, 28:31] - np.asarray(p_ref, float)[None]
        fnm = obs[:, 46] * (obs[:, 47] > 0.5)
        series["t"][k] = t
        series["err_tan"][k] = np.linalg.norm(err[:, :2], axis=1)
        series["err_3d"][k] = np.linalg.norm(err, axis=1)
        series["fn_meas"][k] = fnm
        series["contact"][k] = (fnm > 0.5).astype(float)
        if verbose and k % 100 == 0:
            print(f"k={k:4d} t={t:6.3f}s | B={B} | median |p-p_ref|={np.median(series['err_3d'][k]):.4f} m | "
                  f"median Fn={np.median(fnm):.2f} N | ok={np.mean(mpc.last_info['ok']):.3f}", flush=True)
    wall = time.perf_counter() - wall0
    mpc.close()
    plant.close()
    keys = SUMMARY_KEYS[:-3]
    per_inst = {k: np.zeros(B) for k in SUMMARY_KEYS}
    for b in range(B):
        s = summary_metrics(series["t"][:, b], series["err_tan"][:, b], series["err_3d"][:, b],
                            series["fn_meas"][:, b], series["contact"][:, b], float(cfg.fn_des), t_cp)
        for k_ in keys:
            per_inst[k_][b] = s[k_]
    per_inst["unstable_ticks"] = unstable_ticks
    per_inst["neg_accepted_ticks"] = neg_ticks
    per_inst["solve_not_ok_ticks"] = not_ok_ticks
    out = dict(names=names, seed=seed, per_instance=per_inst, ticks=steps, wall_s=wall, controller_s=ctrl_s,
               instances=B, shard=(lo, hi), n_all=n_all, variant=variant, solved_ticks=solved_ticks)
    inject_delay, inject_sigma = _inject_profile(sweep_cfgs, dt_ctrl)
    out.update(plant_rows=plant_rows(physics if physics is not None else [PlantPhysics()] * B),
               inject_delay=inject_delay, inject_sigma=inject_sigma)
    if plant_payload is not None:
        out.update(plant_payload_mass=plant_payload, payload_known=False)
    if rec_idx:
        out["record"] = dict(index=np.array(rec_idx), t=rec_t, obs=rec_obs, tau=rec_tau, q0=q0[rec_idx], traj=traj,
                             config=cfg, dt=plant.dt, calibration_obs=obs0)
        if variant == "ff":
            out["record"]["tau_hat"] = rec_tau_hat
    return out


def _mismatch_outputs(loop, r: dict, ucfgs, B: int, with_fail: bool) -> dict:
    """The device loop's per-instance physics rows and injector constants for the sweep's summary; with_fail:
    also ``plant_fail`` (B,), each instance's failed plant steps."""
    out = dict(plant_rows=loop.plant_rows.copy(), inject_delay=np.full((B, 2), -1, np.int64),
               inject_sigma=np.full((B, 3), np.nan))
    if ucfgs is not None:
        out.update(inject_a=r["inject_a"], inject_b=r["inject_b"], inject_delay=loop.inject_delay.copy(),
                   inject_sigma=loop.inject_sigma.copy())
    if with_fail:
        out["plant_fail"] = np.asarray(r["plant_fail"])
    return out


DEVICE_MEMORY: dict = {}  # the last device-loop sweep's memory figures (tools/sweep_c4.py reports them)


def _run_sweep_device(variant, q0, tilt, scale, traj, z_contact, calibration, total_time, neg_step_rule, device, t_cp,
                      verbose, ucfgs=None, noise=None, solve_period=1, command_filter=False, tasks=None,
                      device_summary=False, keep_logs=True, plant_physics=None, allow_plant_fail=False,
                      force_profiles=None, weights=None, limit_scale=None, payload_mass=None,
                      plant_payload_mass=None, payload_known=False, tilt_known=False) -> dict:
    """run_sweep's loop on the device (fleet_loop.DeviceFleetLoop) and the
    host path's summary from the downloaded logs.  tasks: per-instance
    FleetTasks in place of traj; the summary's reference position and its
    contact phase are then each instance's own, in its task time.
    device_summary: the summary from the loop's device accumulators instead;
    keep_logs=False: the loop keeps no per-tick logs.  plant_physics: one
    PlantPhysics per instance (None: the scene's constants).  force_profiles:
    one ForceProfile (or None) per instance; the force error is then against
    each instance's own reference at the sample's series time.  weights:
    {name: (B,) values} (sweep_cost_weights), each instance's own cost weights
    over the configuration's.  limit_scale: (B,) scales (sweep_limit_scales) of
    the configuration's tau_limits, each instance's own torque limits.
    payload_mass: (B,) masses (sweep_payload_masses) of a point payload at the
    EE offset in each instance's controller model.  plant_payload_mass: (B,)
    masses (sweep_plant_payload_masses) of the same on each instance's plant;
    payload_known: its controller plans with that model too (payload_mass is
    then None)."""
    import torch

    from .fleet_loop import DeviceFleetLoop

    B = q0.shape[0]
    timestep, n_substeps = 0.001, 5
    dt = float(timestep * n_substeps)  # BatchedPlant.dt
    make_cfg = ff_benchmark_config if variant == "ff" else classical_benchmark_config
    cfg = make_cfg(dt, z_contact, neg_step_rule=neg_step_rule)
    cfg.apply_command_filter = bool(command_filter)
    steps = int(total_time / dt)
    loop = DeviceFleetLoop(variant, B, traj if tasks is None else None, cfg, q0, tilt_deg=tilt, torque_scale=scale,
                           device=device, steps=steps,
                           calibration=calibration, timestep=timestep, n_substeps=n_substeps, uncertainty=ucfgs,
                           noise=noise or "numpy", solve_period=int(solve_period), tasks=tasks,
                           metrics=bool(device_summary), logs=bool(keep_logs),
                           t_contact_phase=float(t_cp) if device_summary and tasks is None else None,
                           plant_physics=plant_physics, force_profiles=force_profiles,
                           cost_weights=None if weights is None else
                           [{name: float(v[b]) for name, v in weights.items()} for b in range(B)],
                           torque_limits=None if limit_scale is None else np.asarray(limit_scale, float),
                           link_models=payload_models(payload_mass) if payload_mass is not None else
                           payload_models(plant_payload_mass) if payload_known else None,
                           plant_link_models=None if plant_payload_mass is None else
                           payload_models(plant_payload_mass),
                           mounts=[R.Mount.table_tilt(float(a)) if float(a) != 0.0 else None for a in tilt]
                           if tilt_known else None)
    wall0 = time.perf_counter()
    loop.run(steps)
    torch.cuda.synchronize(loop.dev)
    wall = time.perf_counter() - wall0
    r = loop.results()
    # device memory while the loop's arrays and the handles' workspaces are alive: torch's own peak, and what
    # the device reports in use (torch's pool, the library's allocations and the runtime's)
    free_b, total_b = torch.cuda.mem_get_info(loop.dev)
    DEVICE_MEMORY.clear()
    DEVICE_MEMORY.update(torch_peak_bytes=int(torch.cuda.max_memory_allocated(loop.dev)),
                         device_used_bytes=int(total_b - free_b))
    loop.close()
    # a failed plant step (non-SPD mass matrix) is an error in the plain sweep; under per-instance physics or
    # profiles an instance may diverge, which is a result: its count is reported (``plant_fail``)
    if np.any(r["plant_fail"]) and not allow_plant_fail:
        raise RuntimeError("run_sweep(device_loop=True): a plant step failed (non-SPD mass matrix)")
    if device_summary:  # B x FLEET_METRICS_W doubles came down; no series is built
        s = r["summary"]
        if verbose:
            print(f"device loop: B={B} ticks={steps} | median rms |p-p_ref|={np.median(s['rms_3d_error']):.4f} m | "
                  f"median max Fn={np.median(s['max_fn']):.2f} N | "
                  f"ok={1.0 - float(np.sum(s['solve_not_ok_ticks'])) / max(B * steps, 1):.3f}", flush=True)
        out = dict(per_instance={k: np.asarray(s[k], float) for k in SUMMARY_KEYS}, ticks=steps, wall_s=wall,
                   controller_s=None, instances=B, variant=variant, solved_ticks=np.asarray(s["solved_ticks"], float))
        out.update(_mismatch_outputs(loop, r, ucfgs, B, allow_plant_fail))
        if "force_rec" in r:
            out["force_rec"] = r["force_rec"]
        if weights is not None:
            out.update(weights=weights, cost_rows=r["cost_rows"])
        if limit_scale is not None:
            out.update(limit_scale=np.asarray(limit_scale, float), tau_limits=loop.tau_limits)
        if payload_mass is not None:
            out.update(payload_mass=np.asarray(payload_mass, float))
        if plant_payload_mass is not None:
            out.update(plant_payload_mass=np.asarray(plant_payload_mass, float), payload_known=bool(payload_known))
        if tilt_known:
            out.update(tilt_known=True)
        if tasks is not None and keep_logs:
            out.update(solved=r["solved"], surface=r["surface"] != 0)
        return out
    # series[k]: the plant after tick k's command, at the time t_k + dt (the host loop's t += dt)
    t_after = np.array([float(t) + dt for t in r["t"]])
    obs = r["obs"][1:]
    if tasks is None:
        p_ref = np.stack([np.asarray(traj(float(t))[0], float) for t in t_after])[:, None, :]
        t_series, t_cps = np.repeat(t_after[:, None], B, 1), np.full(B, float(t_cp))
    else:
        rec = task_records(tasks)
        t_series = r["t_task"] + dt
        p_ref = np.stack([sample_records(rec, t_series[k])[0] for k in range(steps)])
        t_cps = np.array([float(k.t_contact_phase) for k in tasks])
    err = obs[:, :, 0:3] - p_ref
    fnm = obs[:, :, 3] * (obs[:, :, 4] > 0.5)
    series = dict(t=t_series, err_tan=np.linalg.norm(err[:, :, :2], axis=2),
                  err_3d=np.linalg.norm(err, axis=2), fn_meas=fnm, contact=(fnm > 0.5).astype(float))
    if verbose:
        print(f"device loop: B={B} ticks={steps} | final median |p-p_ref|={np.median(series['err_3d'][-1]):.4f} m | "
              f"median Fn={np.median(fnm[-1]):.2f} N | ok={np.mean(r['ok']):.3f}", flush=True)
    per_inst = {k: np.zeros(B) for k in SUMMARY_KEYS}
    # the force reference of every sample: the scalar, or each instance's profile at the series time
    f_ref = sample_force(r["force_rec"], t_series.T) if "force_rec" in r else None  # (B, steps)
    for b in range(B):
        s = summary_metrics(series["t"][:, b], series["err_tan"][:, b], series["err_3d"][:, b],
                            series["fn_meas"][:, b], series["contact"][:, b],
                            float(cfg.fn_des) if f_ref is None else f_ref[b], float(t_cps[b]))
        for k_ in SUMMARY_KEYS[:-3]:
            per_inst[k_][b] = s[k_]
    per_inst["unstable_ticks"] = (r["unstable"] != 0).sum(0).astype(float)
    per_inst["neg_accepted_ticks"] = (r["neg_accepted"] > 0).sum(0).astype(float)
    per_inst["solve_not_ok_ticks"] = (r["ok"] == 0).sum(0).astype(float)
    out = dict(per_instance=per_inst, ticks=steps, wall_s=wall, controller_s=None, instances=B, variant=variant,
               solved_ticks=r["solved"].sum(0).astype(float))
    out.update(_mismatch_outputs(loop, r, ucfgs, B, allow_plant_fail))
    if "force_rec" in r:
        out["force_rec"] = r["force_rec"]
    if weights is not None:
        out.update(weights=weights, cost_rows=r["cost_rows"])
    if limit_scale is not None:
        out.update(limit_scale=np.asarray(limit_scale, float), tau_limits=loop.tau_limits)
    if payload_mass is not None:
        out.update(payload_mass=np.asarray(payload_mass, float))
    if plant_payload_mass is not None:
        out.update(plant_payload_mass=np.asarray(plant_payload_mass, float), payload_known=bool(payload_known))
    if tilt_known:
        out.update(tilt_known=True)
    if tasks is not None:
        out.update(solved=r["solved"], surface=r["surface"] != 0)  # (ticks, B): the per-tick solve share
    return out


SUMMARY_KEYS = ("rms_tangential_error", "rms_tangential_error_contact_phase", "rms_3d_error", "avg_abs_force_err",
                "max_fn", "contact_loss_contact_phase_pct", "fn_mean_contact_phase", "unstable_ticks",
                "neg_accepted_ticks", "solve_not_ok_ticks")


def gather_summaries(res: dict, n_all: int, device=None):
    """All-gather every rank's per-instance summaries into (n_all, len(SUMMARY_KEYS))
    in instance order (the sweep's one exchange; RCCL when the tensors live on
    a GPU, gloo on the CPU)."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size() if dist.is_initialized() else 1
    per = (n_all + world - 1) // world
    local = np.full((per, len(SUMMARY_KEYS)), np.nan)
    m = np.stack([res["per_instance"][k] for k in SUMMARY_KEYS], 1)
    local[: m.shape[0]] = m
    t = torch.from_numpy(local)
    if device is not None:
        t = t.to(device)
    if world == 1:
        return local[:n_all]
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return torch.cat(out, 0).cpu().numpy()[:n_all]


def scenario_table(names, metrics: np.ndarray) -> dict:
    """Per-scenario mean / median / p95 of each summary metric."""
    out = {}
    for s in dict.fromkeys(names):
        sel = metrics[np.asarray(names) == s]
        out[str(s)] = {k: {"mean": float(np.nanmean(sel[:, i])), "median": float(np.nanmedian(sel[:, i])),
                           "p95": float(np.nanpercentile(sel[:, i], 95))} for i, k in enumerate(SUMMARY_KEYS)}
        out[str(s)]["instances"] = int(sel.shape[0])
    return out
