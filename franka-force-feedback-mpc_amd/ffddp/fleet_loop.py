"""The fleet closed loop on the device: B plants and B MPC controllers stepped
together with the host only enqueuing.

``DeviceFleetLoop`` is ``run_sweep``'s loop (fleet.py) with everything a tick
does kept in HBM: per tick it enqueues the plant step (ffddp_plant_step_dev),
the controllers' work before the solve (ffddp_fleet_pre_dev: surface latch,
mode-switch drop, references with the device gravity torque, warm start), the
batched solve, and their work after it (ffddp_fleet_post_dev: keep, torque
policy, unstable fallback, clip, the plant-side actuation and the tick's log
rows).  No host synchronisation and no host<->device copy happens inside
``run``; the logs come down once in ``results``.

With ``uncertainty`` the ``actuation_uncertainty`` scenario's injector runs in
the loop as two more launches per tick: ffddp_fleet_inject_obs_dev after the
plant step (delayed, noisy observations and the noisy torque measurement into
controller-side buffers that pre then reads instead of the plant's records)
and ffddp_fleet_inject_cmd_dev after post (the applied torque becomes a *
(delayed command) + b + noise).  Instances with and without an injector share
one fleet.  The arithmetic is BatchedUncertaintyInjector's bit for bit; the
normals come either from a table drawn ahead from the instances' numpy
Generators (``noise="numpy"``: the host sweep's perturbations exactly,
224 bytes per instance and tick) or from Philox4x64-10 on the device
(``noise="philox"``: no table, another stream; uncertainty.philox_normals).

The node references and the contact hint of every tick depend on the time
only, so they are tabulated on the host before the run (``reference_table``,
the fleets' ``node_ref``) and uploaded once: the solve's inputs are the host
fleets' bit for bit.  Per instance the loop computes what ``FleetClassicalMPC``
/ ``FleetForceFeedbackMPC.compute_control`` compute, up to the order of
summation inside the policy's dot products and the device (rather than host)
evaluation of the gravity torque reference.

With ``solve_period = P > 1`` or ``apply_command_filter`` the tick is the
scheduled one (include/ffddp.h, ffddp_fleet_sched): ffddp_fleet_pre_sched_dev
decides on the device which instances solve (every P-th tick, or at once
after a mode switch, an unstable tick or a non-finite solve), the solve takes
that mask (ffddp_solve_batch_sel_dev), ffddp_fleet_post_sched_dev runs the
policy on the receding plan of the others.  The mask of tick k is row k of a
(steps, B) log, returned as ``solved``.  With period 1 and no filter the loop
enqueues exactly the unscheduled calls.

With ``tasks`` (one trajectory.FleetTask per instance, or one for all) in
place of ``traj_fn`` no table is built: every instance carries a record of its
own task and a start delay, and the pre kernel (ffddp_fleet_pre_task_dev)
samples that instance's N+1 references and its contact hint itself, at the
tick's time minus the delay.  An instance delayed by d ticks waits at the
start pose (the smoothstep clamps at negative task time) and reaches the
contact switch d ticks after its neighbours; ``_need_solve`` re-anchors its
solve grid there, so delays that are no multiples of the period spread the
fleet's solves over the ticks.  ``steps`` then sizes the logs only.

With ``metrics=True`` the sweep's summary is accumulated on the device too:
one more launch per tick (ffddp_fleet_metrics_dev, right after the plant step,
before inject_obs and pre) folds the plant's record after the previous tick's
command into per-instance running sums, maxima and counts, and ``results``
returns them (``metrics``) with the statistics they determine (``summary``).
With ``logs=False`` as well the per-tick logs shrink to rows reused every tick
and, when neither a reference table nor a noise table is sized by ``steps``
(``tasks`` given; no injector, or ``noise="philox"``), the loop runs for any
number of ticks in constant memory.

With ``plant_physics`` every instance integrates with its own physics row
(plant.PlantPhysics: armature, damping, tool radius, contact margin, solref,
solimp; ffddp_plant_set_instance_params) from the start sequence on, and the
``uncertainty`` configs may be any mix: each injected instance keeps its own
delays and sigmas (ffddp_fleet_inject_*_rows_dev), the rings as deep as the
largest delay.  Neither adds a launch; configs that differ by seed only, and
a loop without ``plant_physics``, enqueue exactly the calls they did before.

With ``force_profiles`` (one trajectory.ForceProfile or None per instance)
the desired normal force is each instance's own function of its task time: one
more launch per tick (ffddp_fleet_force_refs_dev, between pre and the solve)
samples the N+1 knots of every instance's profile at the task sampler's knot
times into ``force_ref`` (B, N+1), and the solve takes it
(ffddp_solve_batch_fref_dev) in place of the configuration's ``fn_des``; the
metrics score the force error against the same profile at the series time.
A None entry is the constant ``fn_des``.  The sampler is a function of the
tick's time, so ``state`` / ``load_state`` carry nothing for it.  Without the
argument (or with every entry None) the loop enqueues exactly the calls it did.

With ``cost_weights`` every instance solves with its own scalar cost weights
(ffddp_solve_batch_wts_dev): a (B, COST_W) array of rows, or one dict of named
overrides (or None) per instance over the row that repeats the configuration
(config.cost_weight_row).  The rows are uploaded once and every tick's solve
takes them, whatever else the loop runs; there is no launch more per tick and
``state`` / ``load_state`` carry nothing for them.  Without the argument the
loop enqueues exactly the calls it did.

With ``torque_limits`` every instance solves, and is commanded, within its own
torque limits (ffddp_solve_batch_lim_dev, ffddp_fleet_post_lim_dev): a (B, 7)
array of limits, or one scalar per instance that scales the configuration's
``tau_limits``.  The rows (config.torque_limit_rows) are uploaded once and
every tick's solve and post take them, scheduled or not, together with every
other per-instance option; there is no launch more per tick and ``state`` /
``load_state`` carry nothing for them.  Without the argument the loop enqueues
exactly the calls it did.

With ``link_models`` every instance plans with its own rigid-body model
(ffddp_solve_batch_mdl_dev, ffddp_fleet_pre_mdl_dev): one robot.LinkModel per
instance (None: the nominal one).  The rows (config.link_model_rows) are
uploaded once and every tick's pre -- the gravity torque reference -- and solve
take them, scheduled or not, together with every other per-instance option;
there is no launch more per tick and ``state`` / ``load_state`` carry nothing
for them.  The plant is not touched.  Without the argument the loop enqueues
exactly the calls it did.

With ``plant_link_models`` every instance's plant integrates with its own link
inertial parameters (ffddp_plant_set_instance_links): one robot.LinkModel per
instance (None: the nominal one), the arm the instance really has, whatever
its controller believes (``link_models``).  The rows are handed to the loop's
BatchedPlant once, before the start sequence; there is no launch more per tick
and ``state`` / ``load_state`` carry nothing for them.  It combines with
``plant_physics``, ``link_models`` and every other per-instance option.
Without the argument the loop enqueues exactly the calls it did.

With ``mounts`` every instance plans under its own base mounting and gravity
vector (ffddp_solve_batch_mnt_dev, ffddp_fleet_pre_mnt_dev): one robot.Mount
per instance (None: the nominal one), each with a ``frame`` -- the unchanged
arm seen from another planning frame, such as the tilted table's
(robot.Mount.table_tilt).  The plant stand-in has one mounting, so a
``remounted`` arm is refused.  The rows (config.mount_rows) and the frames
(Mount.obs_frame) are uploaded once.  After every plant step, and at the start
sequence's first observation, one launch (ffddp_fleet_obs_frame_dev) writes the
plant's records re-expressed in each instance's planning frame; the
controllers' inputs, the logs and the metrics read those records, the injector
goes on reading the joint-space q, v of the plant's own.  A mounted instance's
task record, force profile, logs and metrics are therefore read in its planning
frame: under a table_tilt mount the circle lies on the table and the tracking
errors are measured along it.  The site calibration ``p_site_minus_frame`` is
the shared nominal one: it is the site-minus-frame offset with the tool at the
orientation the controller holds, and under a table-frame mount the controller
holds that orientation relative to the table, so the nominal numbers are the
right ones.  The plant and its tilted plane are unchanged, and ``state`` /
``load_state`` carry nothing for the mounts: ``load_state`` re-frames the
plant records it uploaded, with the loop's own frames.  Without the argument, or with
None for every instance, the loop enqueues exactly the calls it did.

Not on the device, and so not supported here: ``run_sweep``'s ``record`` and
any per-tick host callback; ``tick()`` lets a caller look between ticks at the price of its own
synchronisation.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from . import _abi
from . import robot as R
from .config import cost_weight_row, link_model_rows, mount_rows, torque_limit_rows
from .controller import ff_filter_alpha
from .fleet import Traj, fleet_ocp_config, node_ref, site_calibration
from .trajectory import FleetTask, ForceProfile, force_records, task_records
from .uncertainty import UncertaintyProfileConfig, delay_steps, draw_gain_bias, predraw

LPF_ALPHA = 0.2  # PandaTablePlant's tau_meas_lpf_alpha: the ff sweep's torque measurement filter


def reference_table(traj_fn: Traj, steps: int, dt: float, N: int, dt_ocp: float, R_mj_from_pin,
                    p_site_minus_frame_pin, t0: float = 0.0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every tick's node references (steps, N+1, 6), contact hint (steps,) and
    time (steps,), by the fleets' ``node_ref``; tick k runs at t0 advanced k
    times by dt (the sweep's ``t += dt``).  Host only: needs no device."""
    refs = np.zeros((steps, N + 1, 6))
    hints = np.zeros(steps, bool)
    times = np.zeros(steps)
    t = float(t0)
    for k in range(steps):
        refs[k] = node_ref(traj_fn, t, N, dt_ocp, R_mj_from_pin, p_site_minus_frame_pin)
        hints[k] = bool(traj_fn(t)[2])
        times[k] = t
        t += dt
    return refs, hints, times


def fleet_params(cfg, variant: str, dt_ocp: float) -> _abi.FleetParams:
    """ffddp_fleet_params from a ClassicalMPCConfig / ForceFeedbackMPCConfig:
    the scalars the fleets read in _surface, compute_control and _command."""
    p = _abi.FleetParams()
    p.phase_source = 1 if str(cfg.phase_source).strip().lower() == "force_latch" else 0
    p.contact_release_steps = int(cfg.contact_release_steps)
    mode = str(cfg.posture_ref_mode).strip().lower()
    p.posture_mode = (0 if mode == "x0" else 1) if variant == "ff" else (1 if mode == "q_nom" else 0)
    tmode = str(cfg.torque_ref_mode).strip().lower()
    p.torque_mode = 2 if tmode == "zero" else (1 if tmode == "gravity_qnom" else 0)
    p.use_feedback_policy = int(bool(cfg.use_feedback_policy))
    p.z_contact, p.z_contact_band = float(cfg.z_contact), float(cfg.z_contact_band)
    p.fn_contact_on, p.fn_contact_off = float(cfg.fn_contact_on), float(cfg.fn_contact_off)
    p.feedback_gain_scale = float(cfg.feedback_gain_scale)
    p.max_solver_cost, p.max_tau_raw_inf = float(cfg.max_solver_cost), float(cfg.max_tau_raw_inf)
    p.fallback_dq_damping = float(cfg.fallback_dq_damping)
    _abi._fill(p.tau_limits, np.asarray(cfg.tau_limits, float))
    if variant == "ff":
        dt_mpc = float(cfg.dt)
        p.ff_use_tau_interpolation = int(bool(cfg.ff_use_tau_interpolation))
        p.ff_inverse_actuation_model = int(bool(cfg.ff_inverse_actuation_model))
        p.ff_dt_mpc_below_dt_ocp = int(dt_mpc < dt_ocp - 1.0e-9)
        p.eps_pol = float(np.clip(dt_mpc / dt_ocp, 0.0, 1.0))
        p.alpha_ocp = ff_filter_alpha(cfg, dt_ocp)
        p.alpha_ctrl = ff_filter_alpha(cfg, dt_mpc)
    return p


STATE_KEYS = ("valid", "latched", "loss_count", "prev_mode", "tau_prev", "keep_xs", "keep_us", "keep_K")
_PLANT_KEYS = ("q", "v", "obs", "tau_app", "tau_filt")
_INJECT_KEYS = ("obs_ring", "cmd_ring", "tau_hat_filt", "z_cmd")  # the injector's state (ffddp_fleet_inject)
# the scheduled tick's state: its counters (ffddp_fleet_sched) and the solve's output rows post reads for an
# instance that does not solve (its last solve's cost, iters, ok, fn_pred: the controllers' _last_solve_*)
_SCHED_KEYS = ("since", "age", "cost", "iters", "ok", "fn_pred")


def resolve_solve_period(cfg, solve_period: Optional[int]) -> int:
    """The loop's solve period from its ``solve_period`` argument and the
    configuration.  None: the configuration must say 1 (NotImplementedError
    otherwise: a period other than 1 is asked for through the argument).
    P >= 1: the period; a configuration that names another one (neither 1 nor
    P) contradicts it (ValueError).  Host only: needs no device."""
    steps = int(cfg.mpc_update_steps)
    if solve_period is None:
        if steps != 1:
            raise NotImplementedError("DeviceFleetLoop: mpc_update_steps other than 1 is selected with solve_period")
        return 1
    if isinstance(solve_period, bool) or int(solve_period) != solve_period or int(solve_period) < 1:
        raise ValueError(f"DeviceFleetLoop: solve_period must be an integer >= 1, not {solve_period!r}")
    P = int(solve_period)
    if steps not in (1, P):
        raise ValueError(f"DeviceFleetLoop: solve_period={P} contradicts the configuration's mpc_update_steps={steps}")
    return P


def cost_weight_rows(ocp, variant: str, cost_weights, B: int) -> np.ndarray:
    """DeviceFleetLoop's ``cost_weights`` as (B, _abi.COST_W) float64 rows: an
    array is checked (shape, finite, >= 0) and copied; a sequence holds one
    dict of named overrides, or None, per instance over the row that repeats
    the OCP configuration `ocp` (config.cost_weight_row, whose errors apply)."""
    if isinstance(cost_weights, np.ndarray) or (hasattr(cost_weights, "shape") and not isinstance(cost_weights, (list, tuple))):
        rows = np.array(cost_weights, dtype=np.float64)
        if rows.shape != (int(B), _abi.COST_W):
            raise ValueError(f"DeviceFleetLoop: cost_weights must have shape (B, {_abi.COST_W}), not {rows.shape}")
        if not (np.all(np.isfinite(rows)) and np.all(rows >= 0.0)):
            raise ValueError("DeviceFleetLoop: cost_weights must be finite and >= 0")
        return np.ascontiguousarray(rows)
    entries = list(cost_weights)
    if len(entries) != int(B) or not all(e is None or isinstance(e, dict) for e in entries):
        raise ValueError("DeviceFleetLoop: cost_weights takes a (B, COST_W) array, or one entry (a dict of overrides "
                         "or None) per instance")
    return np.stack([cost_weight_row(ocp, variant, **(e or {})) for e in entries])


def instance_torque_limits(tau_limits, torque_limits, B: int) -> np.ndarray:
    """DeviceFleetLoop's ``torque_limits`` as (B, 7) float64 limits: a (B, 7)
    array is taken as it is, a length-B sequence of scalars scales the
    configuration's `tau_limits`.  Another shape, or a value that is not finite
    and > 0, raises ValueError.  Host only: needs no device."""
    a = np.array(torque_limits, dtype=np.float64)
    if a.shape == (int(B), 7):
        lim = a
    elif a.shape == (int(B),):
        if not (np.all(np.isfinite(a)) and np.all(a > 0.0)):
            raise ValueError("DeviceFleetLoop: torque_limits scales must be finite and > 0")
        lim = a[:, None] * np.asarray(tau_limits, dtype=np.float64).reshape(1, 7)
    else:
        raise ValueError(f"DeviceFleetLoop: torque_limits takes a (B, 7) array of limits or B scalars that scale the "
                         f"configuration's, not shape {a.shape}")
    if not (np.all(np.isfinite(lim)) and np.all(lim > 0.0)):
        raise ValueError("DeviceFleetLoop: torque_limits must be finite and > 0")
    return np.ascontiguousarray(lim)


class DeviceFleetLoop:
    """B closed loops (plant + controller) resident on one device.

    variant: "classical" or "ff"; traj_fn: the task, shared by the instances
    and tabulated on the host, or None with ``tasks``: a sequence of B
    FleetTask (or one, broadcast), sampled per instance on the device (both
    or neither is a ValueError); config: the controller
    configuration; solve_period: None (the configuration's mpc_update_steps
    must be 1) or the period P >= 1 of the scheduled tick (a configuration
    with mpc_update_steps other than 1 or P is a ValueError);
    apply_command_filter is taken from the configuration; q0 (B, 7): start
    postures (also each instance's q_nom); tilt_deg,
    torque_scale: per-instance table tilt (hidden from the controllers) and
    command scale, (B, 7) per joint (both broadcast); steps: the most ticks
    the loop will run (sizes the reference table and the logs); calibration:
    (R_site_from_pin_ee, p_site_minus_frame_pin), by default taken from the
    nominal plant at the "neutral" keyframe as run_sweep does.
    uncertainty: None, or one Optional[UncertaintyProfileConfig] per instance
    (None: no injector); the configs may be any mix (delays, sigmas, a / b
    ranges per instance; the rings take the largest delays).  plant_physics:
    None (the scene's constants), one plant.PlantPhysics per instance, or one
    for all.  noise: where
    the injector's normals come from, "numpy" (uncertainty.predraw's table of
    `steps` ticks, uploaded once; at most max_table_bytes) or "philox".
    metrics: accumulate the summary's sums on the device (``acc``
    (FLEET_METRICS_W, B), ``results()["metrics"]`` / ``["summary"]``);
    t_contact_phase: the start of the contact phase the summary uses, a scalar
    or one per instance (required with traj_fn; tasks carry their own).
    logs: False (needs metrics, ValueError otherwise) keeps one row of each
    per-tick log, reused every tick; ``steps`` then bounds the run only where
    a table is sized by it (traj_fn, or the injector's numpy noise).
    force_profiles: None, or one Optional[trajectory.ForceProfile] per instance
    (None: the configuration's fn_des, as is a list of Nones): the desired
    normal force over each instance's task time (the tick's time minus the
    task's delay), sampled per tick and knot on the device (``force_ref``
    (B, N+1), the solve's argument; ``force_rec`` the records).
    cost_weights: None, a (B, _abi.COST_W) array of cost-weight rows, or one
    entry per instance, a dict of overrides for config.cost_weight_row
    (``{"w_fn": 40.0}``) or None (the configuration's weights); ``cost_rows``
    (B, COST_W) keeps the rows as uploaded.
    torque_limits: None, a (B, 7) array of torque limits, or B scalars that
    scale the configuration's tau_limits; ``tau_limits`` (B, 7) keeps the
    limits and ``limit_rows`` (B, TAU_LIM_W) the rows as uploaded.
    link_models: None, or one robot.LinkModel (or None, the nominal model) per
    instance, the model its controller plans with; ``link_rows`` (B, LINK_W)
    keeps the rows as uploaded.
    plant_link_models: None, or one robot.LinkModel (or None, the nominal
    model) per instance, the link inertial parameters its plant integrates
    with; ``plant.link_rows`` (B, LINK_W) keeps the rows as set.

    mounts: None, or one robot.Mount with a ``frame`` (or None, the nominal
    mount) per instance, the base mounting and gravity its controller plans
    under; ``mount_rows`` (B, MOUNT_W) and ``frame_rows`` (B, FRAME_W) keep the
    rows as uploaded, ``obs_frame`` the re-framed records.

    ``S``: the controller state, ``T``: the solve's arrays, ``P``: the plant's
    (q, v, obs, tau_app, tau_filt, plane), ``J``: the injector's (row, a, b,
    seed, the rings, the filter, qv_ctrl, tau_hat, tau_ctrl; with
    ``uncertainty`` only), ``Q``: the scheduled tick's counters (since, age)
    -- all device tensors.
    """

    def __init__(self, variant: str, B: int, traj_fn: Optional[Traj], config, q0, tilt_deg=0.0, torque_scale=1.0,
                 device: int = 0, steps: int = 800, calibration: Optional[tuple] = None, t0: float = 0.0,
                 timestep: float = 0.001, n_substeps: int = 5,
                 uncertainty: Optional[Sequence[Optional[UncertaintyProfileConfig]]] = None, noise: str = "numpy",
                 max_table_bytes: int = 1 << 30, solve_period: Optional[int] = None,
                 tasks: Optional[Sequence[FleetTask]] = None, metrics: bool = False, logs: bool = True,
                 t_contact_phase=None, plant_physics=None,
                 force_profiles: Optional[Sequence[Optional[ForceProfile]]] = None, cost_weights=None,
                 torque_limits=None, link_models=None, plant_link_models=None, mounts=None):
        variant = str(variant).strip().lower()
        if variant not in ("classical", "ff"):
            raise ValueError(f"DeviceFleetLoop: unknown variant {variant!r}")
        inst_limits = None
        if torque_limits is not None:
            inst_limits = instance_torque_limits(config.tau_limits, torque_limits, B)
        if link_models is not None:
            link_models = list(link_models)
            if len(link_models) != int(B) or not all(m is None or isinstance(m, R.LinkModel) for m in link_models):
                raise ValueError("DeviceFleetLoop: link_models takes one robot.LinkModel (or None) per instance")
        if plant_link_models is not None:
            plant_link_models = list(plant_link_models)
            if len(plant_link_models) != int(B) or not all(m is None or isinstance(m, R.LinkModel)
                                                           for m in plant_link_models):
                raise ValueError("DeviceFleetLoop: plant_link_models takes one robot.LinkModel (or None) per instance")
        if mounts is not None:
            mounts = list(mounts)
            if len(mounts) != int(B) or not all(m is None or isinstance(m, R.Mount) for m in mounts):
                raise ValueError("DeviceFleetLoop: mounts takes one robot.Mount (or None) per instance")
            if any(m is not None and m.frame is None for m in mounts):
                raise ValueError("DeviceFleetLoop: every mount must carry a frame (Mount.in_frame / table_tilt); "
                                 "the plant stand-in has one mounting, so a remounted arm cannot run here")
            if all(m is None for m in mounts):
                mounts = None  # the nominal mount for all: the plain loop
        metrics, logs = bool(metrics), bool(logs)
        if not logs and not metrics:
            raise ValueError("DeviceFleetLoop: logs=False needs metrics=True (a run without either reports nothing)")
        if metrics and tasks is None and t_contact_phase is None:
            raise ValueError("DeviceFleetLoop: metrics=True with traj_fn needs t_contact_phase (tasks carry their own)")
        if (traj_fn is None) == (tasks is None):
            raise ValueError("DeviceFleetLoop: give either traj_fn (one task, tabulated on the host) or tasks "
                             "(per instance, sampled on the device)")
        if tasks is not None:
            tasks = [tasks] * int(B) if isinstance(tasks, FleetTask) else list(tasks)
            if len(tasks) != int(B) or not all(isinstance(k, FleetTask) for k in tasks):
                raise ValueError("DeviceFleetLoop: tasks takes one FleetTask per instance, or one for all")
        if noise not in _abi.INJECT_NOISE_MODES:
            raise ValueError(f"DeviceFleetLoop: unknown noise source {noise!r} (numpy or philox)")
        ucfgs = None
        if uncertainty is not None:
            ucfgs = list(uncertainty)
            if len(ucfgs) != int(B):
                raise ValueError("DeviceFleetLoop: uncertainty takes one entry (a config or None) per instance")
            if not all(c is None or isinstance(c, UncertaintyProfileConfig) for c in ucfgs):
                raise ValueError("DeviceFleetLoop: uncertainty entries are UncertaintyProfileConfig or None")
        cfg = config
        if force_profiles is not None:
            force_profiles = list(force_profiles)
            if len(force_profiles) != int(B) or not all(f is None or isinstance(f, ForceProfile) for f in force_profiles):
                raise ValueError("DeviceFleetLoop: force_profiles takes one entry (a ForceProfile or None) per instance")
            if all(f is None for f in force_profiles):
                force_profiles = None  # the configuration's fn_des for all: the plain loop
            elif not float(cfg.w_fn) > 0.0:
                raise ValueError("DeviceFleetLoop: force_profiles need the fn_track cost (w_fn > 0)")
        self.period = resolve_solve_period(cfg, solve_period)
        import torch

        from .plant import BatchedPlant, PandaTablePlant, PlantPhysics, plant_rows, table_plane
        from .solver import BatchedBoxFDDP

        self.torch = torch
        self.variant, self.B, self.cfg, self.traj_fn = variant, int(B), cfg, traj_fn
        self.nx = 21 if variant == "ff" else 14
        self.N = int(cfg.horizon)
        self.steps = int(steps)
        self.dt_ocp = float(cfg.dt_ocp) if cfg.dt_ocp is not None else float(cfg.dt)
        self.dev = torch.device("cuda", device)
        if calibration is None:
            nominal = PandaTablePlant(n_substeps=n_substeps, timestep=timestep, device=device)
            calibration = site_calibration(nominal.reset("neutral"))
            nominal.close()
        R_site, p_off = (np.asarray(a, float) for a in calibration)
        self.R_des = R.R_MJ_FROM_PIN.T @ R.vertical_down_rotation_mj() @ R_site.T
        # the physics rows are in force from the start sequence on (the level table's forward pass included)
        if plant_physics is not None:
            phys = [plant_physics] * self.B if isinstance(plant_physics, PlantPhysics) else list(plant_physics)
            if len(phys) != self.B or not all(isinstance(p, PlantPhysics) for p in phys):
                raise ValueError("DeviceFleetLoop: plant_physics takes one PlantPhysics per instance, or one for all")
            plant_physics = plant_rows(phys)
        self.plant = BatchedPlant(self.B, timestep=timestep, n_substeps=n_substeps, device=device,
                                  physics=plant_physics, link_models=plant_link_models)
        self.plant_rows = plant_rows([PlantPhysics()] * self.B) if plant_physics is None else plant_physics.copy()
        self._has_physics = plant_physics is not None
        self.dt = self.plant.dt
        self.metrics, self.logs, self.t0 = metrics, logs, float(t0)
        # without logs nothing is sized by `steps` unless a table is: the references' or the injector's normals
        self.unbounded = (not logs and tasks is not None
                          and (ucfgs is None or noise == "philox" or all(c is None for c in ucfgs)))
        self._t_run = (0, float(t0))
        self.tasks, self.task_rec, self.task_delay = tasks, None, None
        if tasks is None:
            self.refs, self.hints, self.times = reference_table(traj_fn, self.steps, self.dt, self.N, self.dt_ocp,
                                                                R.R_MJ_FROM_PIN, p_off, t0)
        else:  # no table: the ticks' times only, by the sweep's t += dt
            self.refs = self.hints = None
            self.times = np.zeros(self.steps)
            t = float(t0)
            for k in range(self.steps):
                self.times[k] = t
                t += self.dt
            self.task_rec = task_records(tasks)
            self.task_delay = np.array([float(k.delay) for k in tasks])
        self.params = fleet_params(cfg, variant, self.dt_ocp)
        self.solver = BatchedBoxFDDP(fleet_ocp_config(cfg, variant, self.N, self.dt_ocp, self.R_des),
                                     max_batch=self.B, device=device)
        self.solver.neg_step_rule = int(getattr(cfg, "neg_step_rule", 0))
        self._stream = torch.cuda.current_stream(self.dev).cuda_stream
        B, N, nx = self.B, self.N, self.nx
        f64 = dict(dtype=torch.float64, device=self.dev)
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device=self.dev)  # noqa: E731
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).to(self.dev)  # noqa: E731
        self.S = dict(valid=z(B, dtype=torch.uint8), latched=z(B, dtype=torch.uint8), loss_count=z(B, dtype=torch.int32),
                      prev_mode=torch.full((B,), -1, dtype=torch.int8, device=self.dev), tau_prev=z(B, 7),
                      keep_xs=z(B, N + 1, nx), keep_us=z(B, N, 7), keep_K=z(B, N, 7, nx))
        q0 = np.asarray(q0, float).reshape(B, 7)
        tilt = np.broadcast_to(np.asarray(tilt_deg, float), (B,))
        self.P = dict(q=up(q0), v=z(B, 7), obs=z(B, _abi.PLANT_OBS), tau_app=z(B, 7), tau_filt=z(B, 7),
                      plane=up(np.stack([np.concatenate(table_plane(0.0))] * B)))
        obs = self.P["obs"]
        # per-instance mounts (ffddp_solve_batch_mnt_dev, ffddp_fleet_pre_mnt_dev, ffddp_fleet_obs_frame_dev): the rows
        # and frames, uploaded once, and the re-framed records the controllers, the logs and the metrics read
        self.mount_rows = self.frame_rows = self.mt = self.frame = self.frame_sel = self.obs_frame = None
        self._framed = False  # the start sequence's first plant step is not re-framed (only its bias torque is read)
        if mounts is not None:
            self.mount_rows = mount_rows(mounts)
            self.frame_rows = np.stack([(R.Mount() if m is None else m).obs_frame() for m in mounts])
            self.mt, self.frame = up(self.mount_rows), up(self.frame_rows)
            self.frame_sel = torch.from_numpy(np.array([m is not None for m in mounts], dtype=np.uint8)).to(self.dev)
            self.obs_frame = z(B, _abi.PLANT_OBS)
        plant_obs, obs = obs, (obs if self.obs_frame is None else self.obs_frame)
        self.T = dict(
            x0=z(B, nx), node_ref=z(B, N + 1, 6), inst_ref=z(B, 21), surface=z(B, dtype=torch.uint8),
            xs_init=z(B, N + 1, nx), us_init=z(B, N, 7), xs=z(B, N + 1, nx), us=z(B, N, 7), K=z(B, N, 7, nx),
            cost=z(B), iters=z(B, dtype=torch.int32), ok=z(B, dtype=torch.uint8), fn_pred=z(B, 2),
            stats=z(B, _abi.NSTATS, dtype=torch.int32),
            # the controllers' inputs: views of the plant's records
            q=obs[:, 0:7], v=obs[:, 7:14], tau_bias=obs[:, 14:21], fn_meas=obs[:, 46], contact=obs[:, 47],
            ee_z=obs[:, 30], obs=obs, q_nom=up(q0), tau_cmd=z(B, 7), tau_app=self.P["tau_app"],
            scale=up(np.broadcast_to(np.asarray(torque_scale, float), (B, 7))), **self.S)
        if variant == "ff":
            self.T.update(tau_hat=self.P["tau_filt"], tau_filt=self.P["tau_filt"])
        self.J = self.inject = self.inject_rows = self.inject_a = self.inject_b = None
        self.inject_delay = self.inject_sigma = None
        if ucfgs is not None:
            self.inject_a, self.inject_b = np.full(B, np.nan), np.full(B, np.nan)
            self.inject_delay, self.inject_sigma = np.full((B, 2), -1, np.int64), np.full((B, 3), np.nan)
            if any(c is not None for c in ucfgs):  # else the plain loop
                self._init_inject(ucfgs, noise, max_table_bytes)
        # the scheduled tick: its counters, and one row of `need` per tick (the log `solved`)
        self.Q = dict(since=z(B, dtype=torch.int32), age=z(B, dtype=torch.int32))
        rows = self.steps if logs else 1  # without logs: one row of each, reused every tick
        self.log_need = z(rows, B, dtype=torch.uint8)
        self.sched = None
        if self.period != 1 or bool(cfg.apply_command_filter):
            self.sched = _abi.fleet_sched(cfg, self.period, self.dt)
            self.T.update(self.Q)
        self.Q.update({k: self.T[k] for k in ("cost", "iters", "ok", "fn_pred")})
        self.ref_table = self.rec = self.ktasks = None
        if tasks is None:
            self.ref_table = up(self.refs)
        else:
            self.rec = up(self.task_rec)
            self.ktasks = self.solver.fleet_tasks(self.rec, p_off)
        # per-instance force setpoints (ffddp_fleet_force_refs_dev): the records and the solve's force_ref
        self.force_rec = self.frec = self.force_ref = self.ftasks = None
        if force_profiles is not None:
            fn = float(cfg.fn_des)
            self.force_rec = force_records([ForceProfile(fn, fn) if f is None else f for f in force_profiles])
            self.frec = up(self.force_rec)
            self.force_ref = z(B, N + 1)
            self.ftasks = self.ktasks if self.ktasks is not None else _abi.FleetTasks()
        # per-instance cost weights (ffddp_solve_batch_wts_dev): the rows, uploaded once
        self.cost_rows = self.cw = None
        if cost_weights is not None:
            self.cost_rows = cost_weight_rows(self.solver.cfg, variant, cost_weights, B)
            self.cw = up(self.cost_rows)
        # per-instance torque limits (ffddp_solve_batch_lim_dev, ffddp_fleet_post_lim_dev): the rows, uploaded once
        self.tau_limits = self.limit_rows = self.ul = None
        if inst_limits is not None:
            self.tau_limits = inst_limits
            self.limit_rows = torque_limit_rows(self.solver.cfg, inst_limits)
            self.ul = up(self.limit_rows)
        # per-instance link models (ffddp_solve_batch_mdl_dev, ffddp_fleet_pre_mdl_dev): the rows, uploaded once
        self.link_rows = self.md = None
        if link_models is not None:
            self.link_rows = link_model_rows(link_models)
            self.md = up(self.link_rows)
        self.log_info = torch.full((rows, B, _abi.FLEET_INFO_W), float("nan"), **f64)
        self.log_obs = torch.full((rows + 1 if logs else 1, B, _abi.FLEET_LOG_W), float("nan"), **f64)
        self.log_fail = z(rows + 1, B, dtype=torch.int32)  # without logs: the start's row and the ticks'
        # the task metrics (ffddp_fleet_metrics_dev): the accumulators, each instance's contact-phase start and,
        # in table mode, the reference position after every tick (the sweep's traj(t + dt)[0])
        self.acc = self.t_phase = self.p_tab = self.mtasks = None
        self.m_k = 0  # ticks folded into the accumulators
        if metrics:
            from .runlog import metrics_accumulators

            self.acc = up(metrics_accumulators(B))
            if tasks is not None:
                t_cp = [float(k.t_contact_phase) for k in tasks] if t_contact_phase is None else t_contact_phase
                self.mtasks = self.solver.fleet_tasks(self.rec, np.zeros(3))
            else:
                t_cp = t_contact_phase
                self.p_tab = up(np.stack([np.asarray(traj_fn(float(t) + self.dt)[0], float) for t in self.times]))
            self.t_phase = up(np.broadcast_to(np.asarray(t_cp, float), (B,)))
        # the start: the controllers' first command is the bias torque on a level
        # table (run_sweep); then the tilted plant's first observation
        self._plant_step(integrate=False)
        if variant == "classical":
            self.S["tau_prev"].copy_(plant_obs[:, 14:21])
        self._framed = True
        self.P["plane"].copy_(up(np.stack([np.concatenate(table_plane(t)) for t in tilt])))
        self.k = 0
        self._plant_step(integrate=False)
        self._stepped = True  # obs already is tick k's observation
        torch.cuda.synchronize(self.dev)

    def _init_inject(self, ucfgs, noise: str, max_table_bytes: int):
        """The injector's arrays (``J``) and ffddp_fleet_inject; the controllers'
        inputs q, v (and the ff tau_hat) become views of its outputs."""
        torch, B = self.torch, self.B
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.dev)  # noqa: E731
        idx = [b for b, c in enumerate(ucfgs) if c is not None]
        given = [ucfgs[b] for b in idx]
        row = np.full(B, -1, np.int32)
        row[idx] = np.arange(len(idx), dtype=np.int32)
        c0 = given[0]
        delay = np.array([delay_steps(c, self.dt) for c in given], dtype=np.int32).reshape(len(given), 2)
        sigma = np.array([(c.sigma_q, c.sigma_dq, c.sigma_tau) for c in given], dtype=np.float64)
        d_obs, d_cmd = int(delay[:, 0].max()), int(delay[:, 1].max())  # the ring depths
        self.inject_delay[idx], self.inject_sigma[idx] = delay, sigma
        # the per-row arrays only when the profiles differ: configs that differ by seed (and a / b range: drawn
        # on the host) only take the scalar calls, as before
        mixed = bool(np.any(delay != delay[0]) or np.any(sigma != sigma[0]))
        self.noise, self.z_table = noise, None
        if noise == "numpy":
            a, b, zt = predraw(given, self.steps, max_table_bytes=max_table_bytes)
            self.z_table = torch.from_numpy(zt).to(self.dev)
        else:
            a, b, _ = draw_gain_bias(given)
        self.inject_a[idx], self.inject_b[idx] = a, b
        seed = np.array([int(c.seed) % (1 << 64) for c in given], dtype=np.uint64)
        self.J = dict(row=torch.from_numpy(row).to(self.dev), a=torch.from_numpy(a).to(self.dev),
                      b=torch.from_numpy(b).to(self.dev), seed=torch.from_numpy(seed.view(np.int64)).to(self.dev),
                      obs_ring=z(d_obs + 1, B, 14), cmd_ring=z(d_cmd + 1, B, 7), tau_hat_filt=z(B, 7), z_cmd=z(B, 7),
                      qv_ctrl=z(B, 14), tau_hat=z(B, 7), tau_ctrl=z(B, 7),
                      q=self.P["obs"][:, 0:7], v=self.P["obs"][:, 7:14], tau_cmd=self.T["tau_cmd"],
                      tau_app=self.P["tau_app"])
        if self.variant == "ff":
            self.J["tau_filt"] = self.P["tau_filt"]
        self.inject = self.solver.fleet_inject(self.J, d_obs, d_cmd, (c0.sigma_q, c0.sigma_dq, c0.sigma_tau),
                                               float(np.clip(LPF_ALPHA, 0.0, 1.0)), noise)
        if mixed:
            self.J.update(d_obs=torch.from_numpy(delay[:, 0].copy()).to(self.dev),
                          d_cmd=torch.from_numpy(delay[:, 1].copy()).to(self.dev),
                          sigma=torch.from_numpy(sigma).to(self.dev))
            self.inject_rows = self.solver.fleet_inject_rows(self.J)
        self.T.update(q=self.J["qv_ctrl"][:, 0:7], v=self.J["qv_ctrl"][:, 7:14])
        if self.variant == "ff":
            self.T["tau_hat"] = self.J["tau_ctrl"]

    def close(self):
        self.solver.close()
        self.plant.close()

    # -- the tick ---------------------------------------------------------------------
    def _row(self, k: int) -> int:
        """Tick k's row of the per-tick arrays: its own, or without logs the one reused every tick."""
        return k if self.logs else 0

    def _tick_time(self, k: int) -> float:
        """Tick k's time: t0 advanced k times by dt (the sweep's ``t += dt``), past the sized array too."""
        if k < self.times.shape[0]:
            return float(self.times[k])
        kk, t = self._t_run if self._t_run[0] <= k else (0, self.t0)
        while kk < k:
            t += self.dt
            kk += 1
        self._t_run = (kk, t)
        return t

    def _plant_step(self, integrate: bool = True):
        """The plant step and, with ``metrics``, the fold of the record it leaves -- the observation after tick
        k - 1's command -- into the accumulators: the plant's own record, as the log row, whatever the injector
        shows the controllers."""
        P = self.P
        fail = self.log_fail[(self.k if self.logs else 1) if integrate else 0]
        self.plant.step_dev(P["q"], P["v"], P["tau_app"], P["plane"], P["obs"], fail=fail, integrate=integrate,
                            stream=self._stream)
        rec = P["obs"]
        if self.obs_frame is not None and self._framed:
            rec = self.obs_frame
            self.solver.fleet_obs_frame_dev(P["obs"], self.frame, rec, sel=self.frame_sel, stream=self._stream)
        if self.metrics and integrate and self.m_k < self.k:
            j = self.k - 1
            r = self._row(j)
            kw = dict(info=self.log_info[r], need=self.log_need[r] if self.sched is not None else None, plant_fail=fail,
                      stream=self._stream)
            if self.mtasks is not None:
                self.mtasks.t = self._tick_time(j)
                kw.update(tasks=self.mtasks, dt=self.dt)
            else:
                kw.update(p_ref=self.p_tab[j], ts=float(self.times[j]) + self.dt)
            if self.frec is not None:
                kw.update(force=self.frec)
            self.solver.fleet_metrics_dev(self.acc, rec, self.t_phase, float(self.cfg.fn_des), **kw)
            self.m_k = self.k

    def _enqueue_tick(self):
        k, T = self.k, self.T
        if k >= self.steps and not self.unbounded:
            raise RuntimeError(f"DeviceFleetLoop: the loop was sized for {self.steps} ticks")
        if not self._stepped:
            self._plant_step()
        r = self._row(k)
        T["info"], T["log_obs"] = self.log_info[r], self.log_obs[r]
        if self.ktasks is None:
            T["node_ref1"], hint = self.ref_table[k], bool(self.hints[k])
        else:
            self.ktasks.t, hint = self._tick_time(k), False
        if self.inject is not None:
            self.solver.fleet_inject_obs_dev(self.J, self.inject, k, z=None if self.z_table is None else self.z_table[k],
                                             stream=self._stream, rows=self.inject_rows)
        fkw = {}
        if self.frec is not None:
            self.ftasks.t = self._tick_time(k)
            fkw = dict(force_ref=self.force_ref)
        if self.cw is not None:
            fkw = dict(fkw, cost_weights=self.cw)
        pkw = {}
        if self.ul is not None:
            fkw = dict(fkw, torque_limits=self.ul)
            pkw = dict(torque_limits=self.ul)
        mkw = {}
        if self.md is not None:
            fkw = dict(fkw, link_model=self.md)
            mkw = dict(link_model=self.md)
        if self.mt is not None:
            fkw = dict(fkw, mount=self.mt)
            mkw = dict(mkw, mount=self.mt)
        if self.sched is None:
            self.solver.fleet_pre_dev(T, self.params, hint, stream=self._stream, tasks=self.ktasks, **mkw)
            if self.frec is not None:
                self._force_refs()
            self.solver.solve_dev(T, maxiter=int(self.cfg.max_iters), is_feasible=False, stream=self._stream, **fkw)
            self.solver.fleet_post_dev(T, self.params, lpf=LPF_ALPHA, stream=self._stream, **pkw)
        else:
            T["need"] = self.log_need[r]
            self.solver.fleet_pre_dev(T, self.params, hint, stream=self._stream, sched=self.sched, tasks=self.ktasks,
                                      **mkw)
            if self.frec is not None:
                self._force_refs()
            self.solver.solve_dev(T, maxiter=int(self.cfg.max_iters), is_feasible=False, stream=self._stream,
                                  active=T["need"], **fkw)
            self.solver.fleet_post_dev(T, self.params, lpf=LPF_ALPHA, stream=self._stream, sched=self.sched, **pkw)
        if self.inject is not None:
            self.solver.fleet_inject_cmd_dev(self.J, self.inject, k, stream=self._stream, rows=self.inject_rows)
        self._stepped = False
        self.k = k + 1

    def _force_refs(self):
        """This tick's force_ref from the records, at ``ftasks.t`` (minus each task's delay)."""
        self.solver.fleet_force_refs_dev(self.frec, self.force_ref, tasks=self.ftasks, fn_default=float(self.cfg.fn_des),
                                         stream=self._stream)

    def run(self, steps: int):
        """Enqueue `steps` ticks: plant step, (inject_obs,) pre, (force_refs,) solve, post(, inject_cmd);
        scheduled: pre_sched, the selected-instance solve, post_sched.
        Returns without waiting for the device."""
        for _ in range(int(steps)):
            self._enqueue_tick()

    def tick(self):
        """One tick, waited for, for callers that look at the tensors in between."""
        self._enqueue_tick()
        self.torch.cuda.synchronize(self.dev)

    # -- state and logs -----------------------------------------------------------------
    def state(self) -> dict:
        """Host copies of the controller state (STATE_KEYS), the plant state, the
        injector state (_INJECT_KEYS, with ``uncertainty``), the scheduled
        tick's counters and last-solve rows (_SCHED_KEYS) and the tick counter."""
        self.torch.cuda.synchronize(self.dev)
        s = {k: self.S[k].cpu().numpy().copy() for k in STATE_KEYS}
        s.update({k: self.P[k].cpu().numpy().copy() for k in _PLANT_KEYS})
        if self.J is not None:
            s.update({k: self.J[k].cpu().numpy().copy() for k in _INJECT_KEYS})
        s.update({k: self.Q[k].cpu().numpy().copy() for k in _SCHED_KEYS})
        s.update(k=self.k, stepped=self._stepped)
        if self.metrics:  # the accumulators, the ticks folded, and the last tick's rows its fold will still read
            r = self._row(max(self.k - 1, 0))
            s.update(metrics=self.acc.cpu().numpy().copy(), metrics_k=self.m_k,
                     metrics_info=self.log_info[r].cpu().numpy().copy(), metrics_need=self.log_need[r].cpu().numpy().copy())
        return s

    def load_state(self, s: dict):
        """Upload what ``state`` returned: the loop continues from that tick."""
        torch = self.torch
        for k in STATE_KEYS:
            self.S[k].copy_(torch.from_numpy(np.ascontiguousarray(s[k])).to(self.dev))
        for k in _PLANT_KEYS:
            self.P[k].copy_(torch.from_numpy(np.ascontiguousarray(s[k])).to(self.dev))
        for k in _INJECT_KEYS if self.J is not None else ():
            self.J[k].copy_(torch.from_numpy(np.ascontiguousarray(s[k])).to(self.dev))
        for k in _SCHED_KEYS:
            if k in s:  # a state saved without them: a loop that solves every tick
                self.Q[k].copy_(torch.from_numpy(np.ascontiguousarray(s[k])).to(self.dev))
        self.k, self._stepped = int(s["k"]), bool(s["stepped"])
        if self.metrics:
            if "metrics" in s:
                self.acc.copy_(torch.from_numpy(np.ascontiguousarray(s["metrics"])).to(self.dev))
                self.m_k = int(s["metrics_k"])
                if self.k > 0:
                    r = self._row(self.k - 1)
                    self.log_info[r].copy_(torch.from_numpy(np.ascontiguousarray(s["metrics_info"])).to(self.dev))
                    self.log_need[r].copy_(torch.from_numpy(np.ascontiguousarray(s["metrics_need"])).to(self.dev))
            else:  # a state saved without them: the accumulators go on with the ticks run from here
                self.m_k = self.k
        if self.obs_frame is not None:
            # the re-framed records are derived from the plant's, which were just replaced: a state saved with
            # `stepped` set is followed by a tick that reads them before any plant step rewrites them
            self.solver.fleet_obs_frame_dev(self.P["obs"], self.frame, self.obs_frame, sel=self.frame_sel,
                                            stream=self._stream)
        torch.cuda.synchronize(self.dev)

    def results(self) -> dict:
        """The logs of the k ticks run so far, downloaded once: ``info``
        (k, B, FLEET_INFO_W) and each of its fields by name (k, B), ``obs``
        (k + 1, B, FLEET_LOG_W): row j is the plant record (site position,
        normal force, contact flag) tick j's controllers saw, the last row the
        one after the last command (the plant is stepped for it, once), ``t``
        (k,) the ticks' times, ``plant_fail`` (B,) plant steps that failed,
        ``solved`` (k, B) bool the instances that solved in each tick; with
        ``tasks`` also ``t_task`` (k, B): each instance's task time per tick
        (t minus its delay, the subtraction the pre kernel does); with
        ``uncertainty`` also ``inject_a``, ``inject_b`` (B,): the injectors'
        actuation gain and bias, NaN where there is none, ``inject_delay``
        (B, 2) their (observation, command) delays in ticks and
        ``inject_sigma`` (B, 3) their sigmas, -1 / NaN where there is none;
        and ``plant_rows`` (B, PLANT_ROW_W): the physics each instance
        integrates with (all three are attributes of the loop as well); with
        ``force_profiles`` also ``force_rec`` (B, FLEET_FORCE_W).  With
        ``metrics``
        also ``metrics`` (FLEET_METRICS_W, B): the accumulators over the k
        ticks (the closing plant step's record is folded in here, once), and
        ``summary``: runlog.metrics_from_accumulators of them.  With
        ``logs=False`` only ``ticks`` (k), ``plant_fail``, ``metrics``,
        ``summary`` and the injectors' gain and bias: no per-tick array
        exists; ``plant_rows`` with ``plant_physics`` and ``inject_delay`` /
        ``inject_sigma`` with profiles that differ are added, so a loop
        without either returns the keys it did."""
        torch, k = self.torch, self.k
        if not self._stepped and k > 0:
            self._plant_step()
            self._stepped = True
        if self.logs:
            self.log_obs[k].copy_(self.T["obs"][:, [28, 29, 30, 46, 47]])
        torch.cuda.synchronize(self.dev)
        if self.metrics:
            from .runlog import metrics_from_accumulators

            acc = self.acc.cpu().numpy()[:, : self.B].copy()
            m = dict(metrics=acc, summary=metrics_from_accumulators(acc))
        if not self.logs:
            fails = self.log_fail[0].cpu().numpy() + acc[_abi.FLEET_METRICS_FIELDS.index("plant_fail")].astype(np.int64)
            out = dict(ticks=k, plant_fail=fails, **m)
            if self.inject_a is not None:
                out.update(inject_a=self.inject_a.copy(), inject_b=self.inject_b.copy())
            # the rows and profiles only where they were given: a loop without them returns the keys it did
            if self._has_physics:
                out["plant_rows"] = self.plant_rows.copy()
            if self.inject_rows is not None:
                out.update(inject_delay=self.inject_delay.copy(), inject_sigma=self.inject_sigma.copy())
            if self.force_rec is not None:
                out["force_rec"] = self.force_rec.copy()
            if self.cost_rows is not None:
                out["cost_rows"] = self.cost_rows.copy()
            return out
        info = self.log_info[:k].cpu().numpy()
        out = dict(info=info, obs=self.log_obs[: k + 1].cpu().numpy(), t=self.times[:k].copy(),
                   plant_fail=self.log_fail[: k + 1].sum(0).cpu().numpy(),
                   solved=(self.log_need[:k].cpu().numpy() != 0) if self.sched is not None else np.ones((k, self.B), bool))
        for i, name in enumerate(_abi.FLEET_INFO_FIELDS):
            out[name] = info[:, :, i]
        out["plant_rows"] = self.plant_rows.copy()
        if self.inject_a is not None:
            out.update(inject_a=self.inject_a.copy(), inject_b=self.inject_b.copy(),
                       inject_delay=self.inject_delay.copy(), inject_sigma=self.inject_sigma.copy())
        if self.task_delay is not None:
            out["t_task"] = self.times[:k, None] - self.task_delay[None, :]
        if self.force_rec is not None:
            out["force_rec"] = self.force_rec.copy()
        if self.cost_rows is not None:
            out["cost_rows"] = self.cost_rows.copy()
        if self.metrics:
            out.update(m)
        return out
