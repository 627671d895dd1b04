"""ctypes binding of include/ffddp.h (the drop-in C-ABI).

The library is built in-tree (franka-force-feedback-mpc_amd/lib/libffddp.so)
by __graft_entry__.build() / `make -C franka-force-feedback-mpc_amd/csrc`.
There is no CPU fallback: if the library is missing, import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from pathlib import Path

import numpy as np

from . import robot as R

LIB_PATH = Path(__file__).resolve().parents[1] / "lib" / "libffddp.so"

FFDDP_CLASSICAL = 0
FFDDP_FORCE_FEEDBACK = 1

SYMBOLS = (
    "ffddp_create",
    "ffddp_destroy",
    "ffddp_last_error",
    "ffddp_solve_batch",
    "ffddp_solve_batch_dev",
    "ffddp_solve_batch_sel_dev",
    "ffddp_calc_diff",
    "ffddp_frame_placement",
    "ffddp_gravity_torque",
    "ffddp_gravity_torque_dev",
    "ffddp_build_problem_dev",
    "ffddp_profile_enable",
    "ffddp_profile_read",
    "ffddp_plant_create",
    "ffddp_plant_destroy",
    "ffddp_plant_step",
    "ffddp_plant_step_dev",
    "ffddp_get_solver_params",
    "ffddp_set_solver_params",
    "ffddp_trace_enable",
    "ffddp_trace_read",
    "ffddp_host_alloc",
    "ffddp_host_free",
    "ffddp_plan_create",
    "ffddp_plan_run",
    "ffddp_plan_destroy",
    "ffddp_fleet_warm_start_dev",
    "ffddp_fleet_keep_dev",
    "ffddp_fleet_pre_dev",
    "ffddp_fleet_post_dev",
    "ffddp_fleet_pre_sched_dev",
    "ffddp_fleet_post_sched_dev",
    "ffddp_fleet_inject_obs_dev",
    "ffddp_fleet_inject_cmd_dev",
    "ffddp_fleet_noise_dev",
    "ffddp_fleet_task_refs_dev",
    "ffddp_fleet_pre_task_dev",
    "ffddp_fleet_metrics_dev",
    "ffddp_plant_set_instance_params",
    "ffddp_fleet_inject_obs_rows_dev",
    "ffddp_fleet_inject_cmd_rows_dev",
    "ffddp_solve_batch_fref_dev",
    "ffddp_calc_diff_fref",
    "ffddp_fleet_force_refs_dev",
    "ffddp_fleet_metrics_fref_dev",
    "ffddp_solve_batch_wts_dev",
    "ffddp_calc_diff_wts",
    "ffddp_solve_batch_lim_dev",
    "ffddp_calc_diff_lim",
    "ffddp_torque_limit_rows",
    "ffddp_fleet_post_lim_dev",
    "ffddp_solve_batch_mdl_dev",
    "ffddp_calc_diff_mdl",
    "ffddp_link_model_rows",
    "ffddp_gravity_torque_mdl_dev",
    "ffddp_fleet_pre_mdl_dev",
    "ffddp_plant_set_instance_links",
    "ffddp_solve_batch_mnt_dev",
    "ffddp_calc_diff_mnt",
    "ffddp_mount_rows",
    "ffddp_gravity_torque_mnt_dev",
    "ffddp_fleet_pre_mnt_dev",
    "ffddp_fleet_obs_frame_dev",
)
PLANT_OBS = 69
# FFDDP_PLANT_ROW_*: one instance's physics row (ffddp_plant_set_instance_params)
PLANT_ROW_W = 23
PLANT_ROW_ARMATURE, PLANT_ROW_DAMPING, PLANT_ROW_R_TOOL, PLANT_ROW_MARGIN = 0, 7, 14, 15
PLANT_ROW_SOLREF, PLANT_ROW_SOLIMP = 16, 18
NSTATS = 10
TRACE_W = 10
TRACE_FIELDS = ("iter", "cost", "stop", "grad", "preg", "dreg", "step", "ffeas", "dV", "dV_exp")
NEGSTEP_CROCODDYL = 0
NEGSTEP_BOUNDED_RISE = 1
KERNEL_CLASSES = ("init", "node", "backward", "forward", "accept", "commit", "finalize", "forward2")


def fleet_first_w(nx: int) -> int:
    """FFDDP_FLEET_FIRST_W(nx): doubles per instance of ffddp_fleet_keep_dev's record."""
    return 14 + 9 * int(nx)


FLEET_INFO_W = 12
FLEET_INFO_FIELDS = ("ok", "cost", "iters", "fin", "unstable", "surface", "policy_idx", "neg_accepted", "tau_raw_inf",
                     "tau_cmd_inf", "tau_des_inf", "fn_pred")
FLEET_LOG_W = 5  # site position (3), normal force, contact flag


class FleetState(C.Structure):
    """ffddp_fleet_state: the per-instance controller state of the device fleet loop (device pointers)."""

    _fields_ = [(n, C.c_void_p) for n in ("valid", "latched", "loss_count", "prev_mode", "tau_prev", "keep_xs",
                                          "keep_us", "keep_K")]


class FleetSched(C.Structure):
    """ffddp_fleet_sched: the scheduled tick's period, command filter and per-instance counters (device pointers)."""

    _fields_ = [
        ("period", C.c_int32),
        ("apply_filter", C.c_int32),
        ("tau_trust_inf", C.c_double),
        ("tau_smoothing_alpha", C.c_double),
        ("dt", C.c_double),
        ("tau_rate_limit", C.c_double * 7),
        ("since", C.c_void_p),
        ("age", C.c_void_p),
        ("need", C.c_void_p),
    ]


def fleet_sched(cfg, period: int, dt: float) -> FleetSched:
    """ffddp_fleet_sched's scalars from a controller configuration (the pointers are left null)."""
    s = FleetSched()
    s.period, s.apply_filter = int(period), int(bool(cfg.apply_command_filter))
    s.tau_trust_inf = float(cfg.tau_trust_inf)
    s.tau_smoothing_alpha = float(np.clip(cfg.tau_smoothing_alpha, 0.0, 1.0))
    s.dt = float(dt)
    s.tau_rate_limit[:] = [float(x) for x in np.asarray(cfg.tau_rate_limit, float).reshape(7)]
    return s


INJECT_NOISE_TABLE = 0
INJECT_NOISE_PHILOX = 1
INJECT_NOISE_MODES = {"numpy": INJECT_NOISE_TABLE, "philox": INJECT_NOISE_PHILOX}
INJECT_NZ = 28  # normals per instance and tick: q, dq, tau (observation), tau (command)


class FleetInject(C.Structure):
    """ffddp_fleet_inject: the device uncertainty injector's scalars and device pointers."""

    _fields_ = [
        ("d_obs", C.c_int32),
        ("d_cmd", C.c_int32),
        ("noise", C.c_int32),
        ("rows", C.c_int32),
        ("sigma_q", C.c_double),
        ("sigma_dq", C.c_double),
        ("sigma_tau", C.c_double),
        ("lpf", C.c_double),
    ] + [(n, C.c_void_p) for n in ("row", "a", "b", "seed", "obs_ring", "cmd_ring", "tau_hat_filt", "z_cmd")]


class FleetInjectRows(C.Structure):
    """ffddp_fleet_inject_rows: per-row delays and sigmas of the device injector (device pointers; null = the scalar)."""

    _fields_ = [(n, C.c_void_p) for n in ("d_obs", "d_cmd", "sigma")]


FLEET_TASK_W = 22  # FFDDP_FLEET_TASK_W: doubles per task record (trajectory.task_records fills them)


class FleetTasks(C.Structure):
    """ffddp_fleet_tasks: the site offset, the tick's time and the device pointer to the (B, FLEET_TASK_W) records."""

    _fields_ = [("p_site_minus_frame", C.c_double * 3), ("t", C.c_double), ("rec", C.c_void_p)]


# FFDDP_COST_W / FFDDP_CW_*: one instance's row of scalar cost weights (ffddp_solve_batch_wts_dev): the entry of
# ffddp_ocp_config's w_<name> is COST_INDEX["w_<name>"]; entries 0..9 the frame / contact weights, 16..23 the
# state / control / force-feedback ones, the rest padding (config.cost_weight_row builds a row)
COST_W = 32
COST_INDEX = {
    "w_ee_ori": 0, "w_wdamp": 1, "w_ee_pos": 2, "w_tangent_pos": 3, "w_tangent_vel": 4, "w_plane_z": 5, "w_vz": 6,
    "w_unilateral": 7, "w_fn": 8, "w_friction_cone": 9,
    "w_posture": 16, "w_v": 17, "w_q_soft_limits": 18, "w_tau": 19, "w_tau_soft_limits": 20, "w_y": 21, "w_w": 22,
    "w_w_soft_limits": 23,
}

# FFDDP_TAU_LIM_W: one instance's torque-limit row (ffddp_solve_batch_lim_dev), joint-major: entry 4j u_ub[j],
# 4j + 1 ts_ub[j], 4j + 2 ws_lim[j], the rest padding (config.torque_limit_rows builds rows)
TAU_LIM_W = 32

# FFDDP_LINK_W: one instance's link-model row (ffddp_solve_batch_mdl_dev), joint-major: entry 16j mass[j],
# 16j + 1..3 com[j], 16j + 4..12 inertia[j] row-major, the rest padding (config.link_model_rows builds rows)
LINK_W = 128

# FFDDP_MOUNT_W: one instance's mount row (ffddp_solve_batch_mnt_dev): entries 0..8 base_R row-major, 9..11 base_p,
# 12..14 gravity, 15 padding (config.mount_rows builds rows)
MOUNT_W = 16
# FFDDP_FRAME_W: one instance's planning frame in the MuJoCo world (ffddp_fleet_obs_frame_dev): R row-major, then p
FRAME_W = 12

FLEET_FORCE_W = 4  # FFDDP_FLEET_FORCE_W: doubles per force record, f0, f1, t_on, t_ramp (trajectory.force_records)

FLEET_METRICS_W = 17  # FFDDP_FLEET_METRICS_W: accumulator fields per instance (FFDDP_FLEET_METRICS_*, in order)
FLEET_METRICS_FIELDS = ("n", "n_phase", "sum_tan2", "sum_tan2_phase", "sum_3d2", "sum_abs_tan", "sum_abs_fn_err",
                        "max_fn", "sum_contact", "sum_contact_phase", "sum_fn_phase", "unstable_ticks",
                        "neg_accepted_ticks", "not_ok_ticks", "solved_ticks", "max_err_3d", "plant_fail")


class FleetParams(C.Structure):
    """ffddp_fleet_params: the controller configuration's scalars (fleet_params)."""

    _fields_ = [
        ("phase_source", C.c_int32),
        ("contact_release_steps", C.c_int32),
        ("posture_mode", C.c_int32),
        ("torque_mode", C.c_int32),
        ("use_feedback_policy", C.c_int32),
        ("ff_use_tau_interpolation", C.c_int32),
        ("ff_inverse_actuation_model", C.c_int32),
        ("ff_dt_mpc_below_dt_ocp", C.c_int32),
        ("z_contact", C.c_double),
        ("z_contact_band", C.c_double),
        ("fn_contact_on", C.c_double),
        ("fn_contact_off", C.c_double),
        ("feedback_gain_scale", C.c_double),
        ("max_solver_cost", C.c_double),
        ("max_tau_raw_inf", C.c_double),
        ("fallback_dq_damping", C.c_double),
        ("tau_limits", C.c_double * 7),
        ("eps_pol", C.c_double),
        ("alpha_ocp", C.c_double),
        ("alpha_ctrl", C.c_double),
    ]


class Robot(C.Structure):
    _fields_ = [
        ("joint_R", C.c_double * 9 * 7),
        ("joint_p", C.c_double * 3 * 7),
        ("mass", C.c_double * 7),
        ("com", C.c_double * 3 * 7),
        ("inertia", C.c_double * 9 * 7),
        ("ee_R", C.c_double * 9),
        ("ee_p", C.c_double * 3),
        ("gravity", C.c_double * 3),
    ]


class OcpConfig(C.Structure):
    _fields_ = [
        ("variant", C.c_int32),
        ("horizon", C.c_int32),
        ("nc", C.c_int32),
        ("use_box", C.c_int32),
        ("dt", C.c_double),
        ("z_press", C.c_double),
        ("w_ee_pos", C.c_double),
        ("w_ee_ori", C.c_double),
        ("ori_weights", C.c_double * 3),
        ("w_posture", C.c_double),
        ("w_v", C.c_double),
        ("v_damp_weights", C.c_double * 7),
        ("w_tau", C.c_double),
        ("w_tau_soft_limits", C.c_double),
        ("tau_soft_limit_margin", C.c_double),
        ("w_q_soft_limits", C.c_double),
        ("q_soft_limit_margin", C.c_double),
        ("q_lower", C.c_double * 7),
        ("q_upper", C.c_double * 7),
        ("w_tangent_pos", C.c_double),
        ("w_tangent_vel", C.c_double),
        ("w_plane_z", C.c_double),
        ("w_vz", C.c_double),
        ("w_unilateral", C.c_double),
        ("friction_margin", C.c_double),
        ("w_fn", C.c_double),
        ("fn_des", C.c_double),
        ("w_wdamp", C.c_double),
        ("w_wdamp_weights", C.c_double * 3),
        ("contact_gains", C.c_double * 2),
        ("contact_inv_damping", C.c_double),
        ("tau_limits", C.c_double * 7),
        ("R_des", C.c_double * 9),
        ("ff_alpha", C.c_double),
        ("w_w", C.c_double),
        ("w_w_soft_limits", C.c_double),
        ("w_y", C.c_double),
        ("y_weights", C.c_double * 21),
        ("use_inner_state_reg", C.c_int32),
        ("use_inner_tau_reg", C.c_int32),
        ("w_friction_cone", C.c_double),
        ("mu", C.c_double),
    ]


class PlanIO(C.Structure):
    """ffddp_plan_io (include/ffddp.h): the plan's page-locked inputs / outputs."""

    _fields_ = [(n, C.c_void_p) for n in ("x0", "node_ref", "inst_ref", "surface", "xs_init", "us_init", "xs", "us",
                                          "K", "cost", "iters", "ok", "fn_pred", "stats")]


class SolverParams(C.Structure):
    """ffddp_solver_params: crocoddyl.SolverBoxFDDP / SolverFDDP properties."""

    _fields_ = [
        ("th_stop", C.c_double),
        ("th_grad", C.c_double),
        ("th_acceptstep", C.c_double),
        ("th_acceptnegstep", C.c_double),
        ("th_stepdec", C.c_double),
        ("th_stepinc", C.c_double),
        ("reg_min", C.c_double),
        ("reg_max", C.c_double),
        ("reg_incfactor", C.c_double),
        ("reg_decfactor", C.c_double),
        ("neg_step_rule", C.c_int32),
        ("reserved", C.c_int32),
    ]


def solver_params(use_box: bool = True, **overrides) -> SolverParams:
    """SolverParams with the SolverBoxFDDP (use_box) / SolverFDDP defaults the
    library's handles start from (ffddp_consts.hpp fill_consts), then `overrides`."""
    p = SolverParams()
    vals = dict(th_stop=5e-5 if use_box else 1e-9, th_grad=1e-12, th_acceptstep=0.1, th_acceptnegstep=2.0,
                th_stepdec=0.5, th_stepinc=0.01, reg_min=1e-9, reg_max=1e9, reg_incfactor=10.0, reg_decfactor=10.0,
                neg_step_rule=NEGSTEP_CROCODDYL)
    vals.update(overrides)
    for k, v in vals.items():
        setattr(p, k, v)
    return p


class Task(C.Structure):
    """ffddp_task: the device problem builder's task (trajectories.py:8-93,
    run_classical.py:221-264, crocoddyl_classical.py:250-258, 447-466)."""

    _fields_ = [
        ("center", C.c_double * 3),
        ("radius", C.c_double),
        ("omega", C.c_double),
        ("z_contact", C.c_double),
        ("t_approach", C.c_double),
        ("t_pre", C.c_double),
        ("z_pre", C.c_double),
        ("t_hold", C.c_double),
        ("ee_start", C.c_double * 3),
        ("has_ee_start", C.c_int32),
        ("has_z_pre", C.c_int32),
        ("p_site_minus_frame", C.c_double * 3),
        ("q_nom", C.c_double * 7),
        ("posture_mode", C.c_int32),
        ("torque_mode", C.c_int32),
    ]


class PlantParams(C.Structure):
    """ffddp_plant_params: the closed-loop plant stand-in (ffddp_plant.hpp)."""

    _fields_ = [
        ("timestep", C.c_double),
        ("n_substeps", C.c_int32),
        ("armature", C.c_double * 7),
        ("damping", C.c_double * 7),
        ("r_tool", C.c_double),
        ("margin", C.c_double),
        ("solref", C.c_double * 2),
        ("solimp", C.c_double * 5),
        ("site_R", C.c_double * 2),
    ]


POSTURE_MODES = {"x0": 0, "q_nom": 1}
TORQUE_MODES = {"gravity_x0": 0, "gravity_q_nom": 1, "zero": 2}


def make_task(
    center,
    radius: float,
    omega: float,
    z_contact: float,
    t_approach: float = 2.0,
    ee_start=None,
    z_pre=None,
    t_pre: float = 0.0,
    t_hold: float = 0.0,
    p_site_minus_frame=(0.0, 0.0, 0.0),
    q_nom=None,
    posture_ref_mode: str = "q_nom",
    torque_ref_mode: str = "gravity_x0",
) -> Task:
    """Task with make_approach_then_circle's arguments (trajectories.py:8-17),
    the benchmark hold t_hold (run_classical.py:256-264: 0.2 s) and the
    controller's reference modes (crocoddyl_classical.py:447-466)."""
    t = Task()
    _fill(t.center, center)
    t.radius, t.omega, t.z_contact = float(radius), float(omega), float(z_contact)
    t.t_approach, t.t_pre, t.t_hold = float(t_approach), float(t_pre), float(t_hold)
    t.has_ee_start = int(ee_start is not None)
    if ee_start is not None:
        _fill(t.ee_start, ee_start)
    t.has_z_pre = int(z_pre is not None)
    t.z_pre = float(z_pre) if z_pre is not None else 0.0
    _fill(t.p_site_minus_frame, p_site_minus_frame)
    _fill(t.q_nom, R.Q_NEUTRAL if q_nom is None else q_nom)
    if posture_ref_mode not in POSTURE_MODES or torque_ref_mode not in TORQUE_MODES:
        raise ValueError(f"unknown reference mode {posture_ref_mode!r} / {torque_ref_mode!r}")
    t.posture_mode = POSTURE_MODES[posture_ref_mode]
    t.torque_mode = TORQUE_MODES[torque_ref_mode]
    return t


def _fill(arr, values):
    flat = np.asarray(values, dtype=float).reshape(-1)
    buf = (C.c_double * flat.size).from_buffer(arr)
    for i, v in enumerate(flat):
        buf[i] = float(v)


def make_robot(model=None, mount=None) -> Robot:
    """The Panda's ffddp_robot; model (robot.LinkModel): its inertial
    parameters in place of the nominal ones, the kinematics unchanged; mount
    (robot.Mount): its base placement (joint 1's) and gravity vector in place
    of the nominal ones, everything else unchanged."""
    rb = Robot()
    joint_R, joint_p = R.JOINT_R, R.JOINT_P
    if mount is not None:
        joint_R, joint_p = joint_R.copy(), joint_p.copy()
        joint_R[0], joint_p[0] = mount.base_R, mount.base_p
    _fill(rb.joint_R, joint_R)
    _fill(rb.joint_p, joint_p)
    _fill(rb.mass, R.MASS if model is None else model.mass)
    _fill(rb.com, R.COM if model is None else model.com)
    _fill(rb.inertia, R.INERTIA if model is None else model.inertia)
    _fill(rb.ee_R, R.EE_R)
    _fill(rb.ee_p, R.EE_P)
    _fill(rb.gravity, R.GRAVITY if mount is None else mount.gravity)
    return rb


_lib = None


def load() -> C.CDLL:
    """Load libffddp.so.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch wheels ship their own libamdhip64.so.7
    # and load it by path; if ours (/opt/rocm) were loaded first, torch would
    # bring a second runtime and fail to initialise.  Importing torch first makes
    # the dynamic loader bind our NEEDED libamdhip64.so.7 to the torch copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = Path(os.environ.get("FFDDP_LIB", str(LIB_PATH)))
    if not path.exists():
        raise ImportError(
            f"ffddp: HIP library not found at {path}; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)"
        )
    lib = C.CDLL(str(path))
    dp, ip, up, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p
    lib.ffddp_create.argtypes = [C.POINTER(Robot), C.POINTER(OcpConfig), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ffddp_create.restype = C.c_int
    lib.ffddp_destroy.argtypes = [C.c_void_p]
    lib.ffddp_destroy.restype = None
    lib.ffddp_last_error.argtypes = [C.c_void_p]
    lib.ffddp_last_error.restype = C.c_char_p
    solve_args = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp, C.c_int, C.c_int, dp, dp, dp, dp, ip, up, dp, ip]
    lib.ffddp_solve_batch.argtypes = solve_args
    lib.ffddp_solve_batch.restype = C.c_int
    dev_args = [C.c_void_p, C.c_int] + [vp] * 6 + [C.c_int, C.c_int] + [vp] * 8 + [vp]
    lib.ffddp_solve_batch_dev.argtypes = dev_args
    lib.ffddp_solve_batch_dev.restype = C.c_int
    lib.ffddp_solve_batch_sel_dev.argtypes = dev_args[:-1] + [vp, vp]  # ..., stats, active, stream
    lib.ffddp_solve_batch_sel_dev.restype = C.c_int
    lib.ffddp_calc_diff.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp] + [dp] * 10
    lib.ffddp_calc_diff.restype = C.c_int
    lib.ffddp_solve_batch_fref_dev.argtypes = dev_args[:-1] + [vp, vp, vp]  # ..., stats, active, force_ref, stream
    lib.ffddp_solve_batch_fref_dev.restype = C.c_int
    lib.ffddp_calc_diff_fref.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp, dp] + [dp] * 10
    lib.ffddp_calc_diff_fref.restype = C.c_int
    # ..., stats, active, force_ref, cost_w, stream
    lib.ffddp_solve_batch_wts_dev.argtypes = dev_args[:-1] + [vp, vp, vp, vp]
    lib.ffddp_solve_batch_wts_dev.restype = C.c_int
    lib.ffddp_calc_diff_wts.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp, dp, dp] + [dp] * 10
    lib.ffddp_calc_diff_wts.restype = C.c_int
    # ..., stats, active, force_ref, cost_w, tau_lim, stream
    lib.ffddp_solve_batch_lim_dev.argtypes = dev_args[:-1] + [vp, vp, vp, vp, vp]
    lib.ffddp_solve_batch_lim_dev.restype = C.c_int
    lib.ffddp_calc_diff_lim.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp, dp, dp, dp] + [dp] * 10
    lib.ffddp_calc_diff_lim.restype = C.c_int
    lib.ffddp_torque_limit_rows.argtypes = [C.POINTER(OcpConfig), C.c_int, dp, dp]
    lib.ffddp_torque_limit_rows.restype = C.c_int
    # ..., stats, active, force_ref, cost_w, tau_lim, link_rows, stream
    lib.ffddp_solve_batch_mdl_dev.argtypes = dev_args[:-1] + [vp, vp, vp, vp, vp, vp]
    lib.ffddp_solve_batch_mdl_dev.restype = C.c_int
    lib.ffddp_calc_diff_mdl.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp, dp, dp, dp, dp] + [dp] * 10
    lib.ffddp_calc_diff_mdl.restype = C.c_int
    lib.ffddp_link_model_rows.argtypes = [C.POINTER(Robot), C.c_int, dp]
    lib.ffddp_link_model_rows.restype = C.c_int
    # ..., stats, active, force_ref, cost_w, tau_lim, link_rows, mount_rows, stream
    lib.ffddp_solve_batch_mnt_dev.argtypes = dev_args[:-1] + [vp, vp, vp, vp, vp, vp, vp]
    lib.ffddp_solve_batch_mnt_dev.restype = C.c_int
    lib.ffddp_calc_diff_mnt.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, up, dp, dp, dp, dp, dp, dp, dp] + [dp] * 10
    lib.ffddp_calc_diff_mnt.restype = C.c_int
    lib.ffddp_mount_rows.argtypes = [C.POINTER(Robot), C.c_int, dp]
    lib.ffddp_mount_rows.restype = C.c_int
    lib.ffddp_frame_placement.argtypes = [C.POINTER(Robot), dp, dp, dp]
    lib.ffddp_frame_placement.restype = C.c_int
    lib.ffddp_gravity_torque.argtypes = [C.POINTER(Robot), C.c_int, dp, dp]
    lib.ffddp_gravity_torque.restype = C.c_int
    lib.ffddp_gravity_torque_dev.argtypes = [C.c_void_p, C.c_int, vp, vp, vp]
    lib.ffddp_gravity_torque_dev.restype = C.c_int
    lib.ffddp_gravity_torque_mdl_dev.argtypes = [C.c_void_p, C.c_int, vp, vp, vp, vp]
    lib.ffddp_gravity_torque_mdl_dev.restype = C.c_int
    lib.ffddp_gravity_torque_mnt_dev.argtypes = [C.c_void_p, C.c_int, vp, vp, vp, vp, vp]
    lib.ffddp_gravity_torque_mnt_dev.restype = C.c_int
    lib.ffddp_build_problem_dev.argtypes = [C.c_void_p, C.c_int, C.POINTER(Task)] + [vp] * 6
    lib.ffddp_build_problem_dev.restype = C.c_int
    lib.ffddp_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.ffddp_profile_enable.restype = C.c_int
    lib.ffddp_profile_read.argtypes = [C.c_void_p, dp, C.POINTER(C.c_int64), C.c_int]
    lib.ffddp_profile_read.restype = C.c_int
    lib.ffddp_plant_create.argtypes = [C.POINTER(Robot), C.POINTER(PlantParams), C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]
    lib.ffddp_plant_create.restype = C.c_int
    lib.ffddp_plant_destroy.argtypes = [C.c_void_p]
    lib.ffddp_plant_destroy.restype = None
    lib.ffddp_plant_step.argtypes = [C.c_void_p, C.c_int, dp, dp, dp, dp, C.c_int, dp]
    lib.ffddp_plant_step.restype = C.c_int
    lib.ffddp_plant_step_dev.argtypes = [C.c_void_p, C.c_int] + [vp] * 4 + [C.c_int, vp, vp, vp]
    lib.ffddp_plant_step_dev.restype = C.c_int
    lib.ffddp_get_solver_params.argtypes = [C.c_void_p, C.POINTER(SolverParams)]
    lib.ffddp_get_solver_params.restype = C.c_int
    lib.ffddp_set_solver_params.argtypes = [C.c_void_p, C.POINTER(SolverParams)]
    lib.ffddp_set_solver_params.restype = C.c_int
    lib.ffddp_trace_enable.argtypes = [C.c_void_p, C.c_int]
    lib.ffddp_trace_enable.restype = C.c_int
    lib.ffddp_trace_read.argtypes = [C.c_void_p, C.c_int, dp]
    lib.ffddp_trace_read.restype = C.c_int
    lib.ffddp_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.ffddp_host_alloc.restype = C.c_int
    lib.ffddp_host_free.argtypes = [C.c_void_p]
    lib.ffddp_host_free.restype = C.c_int
    lib.ffddp_plan_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(PlanIO)]
    lib.ffddp_plan_create.restype = C.c_int
    lib.ffddp_plan_run.argtypes = [C.c_void_p]
    lib.ffddp_plan_run.restype = C.c_int
    lib.ffddp_plan_destroy.argtypes = [C.c_void_p]
    lib.ffddp_plan_destroy.restype = None
    lib.ffddp_fleet_warm_start_dev.argtypes = [C.c_void_p, C.c_int] + [vp] * 7 + [vp]
    lib.ffddp_fleet_warm_start_dev.restype = C.c_int
    lib.ffddp_fleet_keep_dev.argtypes = [C.c_void_p, C.c_int] + [vp] * 12 + [vp]
    lib.ffddp_fleet_keep_dev.restype = C.c_int
    fl = [C.c_void_p, C.c_int, C.POINTER(FleetParams), C.POINTER(FleetState)]
    lib.ffddp_fleet_pre_dev.argtypes = (fl + [vp] * 5 + [C.c_int, C.c_int, vp, C.c_int, vp, vp, C.c_int] + [vp] * 6
                                        + [vp])
    lib.ffddp_fleet_pre_dev.restype = C.c_int
    lib.ffddp_fleet_post_dev.argtypes = (fl + [vp] * 8 + [vp, vp, vp, C.c_int, vp, vp] + [vp, vp, vp, C.c_double]
                                         + [vp, C.c_int, vp] + [vp])
    lib.ffddp_fleet_post_dev.restype = C.c_int
    # the scheduled tick: the same arguments, then ffddp_fleet_sched by value before the stream
    lib.ffddp_fleet_pre_sched_dev.argtypes = lib.ffddp_fleet_pre_dev.argtypes[:-1] + [FleetSched, vp]
    lib.ffddp_fleet_pre_sched_dev.restype = C.c_int
    lib.ffddp_fleet_post_sched_dev.argtypes = lib.ffddp_fleet_post_dev.argtypes[:-1] + [FleetSched, vp]
    lib.ffddp_fleet_post_sched_dev.restype = C.c_int
    # per-instance torque limits: const ffddp_fleet_sched* (NULL = unscheduled), tau_lim, stream
    lib.ffddp_fleet_post_lim_dev.argtypes = lib.ffddp_fleet_post_dev.argtypes[:-1] + [C.POINTER(FleetSched), vp, vp]
    lib.ffddp_fleet_post_lim_dev.restype = C.c_int
    fi = [C.c_void_p, C.c_int, C.POINTER(FleetInject), C.c_int]
    lib.ffddp_fleet_inject_obs_dev.argtypes = fi + [vp, vp, vp, C.c_int, vp, vp, vp, vp] + [vp]
    lib.ffddp_fleet_inject_obs_dev.restype = C.c_int
    lib.ffddp_fleet_inject_cmd_dev.argtypes = fi + [vp, vp] + [vp]
    lib.ffddp_fleet_inject_cmd_dev.restype = C.c_int
    # per-row profiles: the same arguments, then const ffddp_fleet_inject_rows* (NULL = the calls above) before the stream
    lib.ffddp_fleet_inject_obs_rows_dev.argtypes = (lib.ffddp_fleet_inject_obs_dev.argtypes[:-1]
                                                    + [C.POINTER(FleetInjectRows), vp])
    lib.ffddp_fleet_inject_obs_rows_dev.restype = C.c_int
    lib.ffddp_fleet_inject_cmd_rows_dev.argtypes = (lib.ffddp_fleet_inject_cmd_dev.argtypes[:-1]
                                                    + [C.POINTER(FleetInjectRows), vp])
    lib.ffddp_fleet_inject_cmd_rows_dev.restype = C.c_int
    lib.ffddp_plant_set_instance_params.argtypes = [C.c_void_p, C.c_int, dp]
    lib.ffddp_plant_set_instance_params.restype = C.c_int
    # per-instance link models of the plant: host rows [n][LINK_W] (NULL = the handle's robot)
    lib.ffddp_plant_set_instance_links.argtypes = [C.c_void_p, C.c_int, dp]
    lib.ffddp_plant_set_instance_links.restype = C.c_int
    lib.ffddp_fleet_noise_dev.argtypes = [C.c_void_p, C.c_int, vp, C.c_int, vp, vp] + [vp]
    lib.ffddp_fleet_noise_dev.restype = C.c_int
    # per-instance tasks: ffddp_fleet_tasks by value; pre_task takes it in place of node_ref1 / contact_hint
    # and a const ffddp_fleet_sched* (NULL = unscheduled) before the stream
    lib.ffddp_fleet_task_refs_dev.argtypes = [C.c_void_p, C.c_int, FleetTasks, vp, vp, vp] + [vp]
    lib.ffddp_fleet_task_refs_dev.restype = C.c_int
    lib.ffddp_fleet_pre_task_dev.argtypes = (fl + [vp] * 5 + [C.c_int, C.c_int, vp, C.c_int, vp, FleetTasks] + [vp] * 6
                                             + [C.POINTER(FleetSched), vp])
    lib.ffddp_fleet_pre_task_dev.restype = C.c_int
    # per-instance link models: tasks (rec NULL = node_ref1 / contact_hint), node_ref1, contact_hint, the outputs,
    # const ffddp_fleet_sched* (NULL = unscheduled), link_rows, stream
    lib.ffddp_fleet_pre_mdl_dev.argtypes = (fl + [vp] * 5 + [C.c_int, C.c_int, vp, C.c_int, vp, FleetTasks, vp, C.c_int]
                                            + [vp] * 6 + [C.POINTER(FleetSched), vp, vp])
    lib.ffddp_fleet_pre_mdl_dev.restype = C.c_int
    # ..., link_rows, mount_rows, stream
    lib.ffddp_fleet_pre_mnt_dev.argtypes = (fl + [vp] * 5 + [C.c_int, C.c_int, vp, C.c_int, vp, FleetTasks, vp, C.c_int]
                                            + [vp] * 6 + [C.POINTER(FleetSched), vp, vp, vp])
    lib.ffddp_fleet_pre_mnt_dev.restype = C.c_int
    # B, obs, ld_obs, frame, sel, obs_out, ld_out, stream
    lib.ffddp_fleet_obs_frame_dev.argtypes = [C.c_void_p, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    lib.ffddp_fleet_obs_frame_dev.restype = C.c_int
    # the task metrics: B, ld, obs, ld_obs, tasks, rows, dt, p_ref, ts, t_phase, fn_des, info, need, plant_fail, acc
    lib.ffddp_fleet_metrics_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, vp, C.c_int, FleetTasks, C.c_int, C.c_double,
                                            vp, C.c_double, vp, C.c_double, vp, vp, vp, vp] + [vp]
    lib.ffddp_fleet_metrics_dev.restype = C.c_int
    # the force profiles: B, tasks, force, rows, fn_default, force_ref; the metrics with ..., acc, force, rows_force
    lib.ffddp_fleet_force_refs_dev.argtypes = [C.c_void_p, C.c_int, FleetTasks, vp, C.c_int, C.c_double, vp] + [vp]
    lib.ffddp_fleet_force_refs_dev.restype = C.c_int
    lib.ffddp_fleet_metrics_fref_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, vp, C.c_int, FleetTasks, C.c_int,
                                                 C.c_double, vp, C.c_double, vp, C.c_double, vp, vp, vp, vp, vp,
                                                 C.c_int] + [vp]
    lib.ffddp_fleet_metrics_fref_dev.restype = C.c_int
    _lib = lib
    return lib


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _pinned_buffer(nbytes: int):
    """One ffddp_host_alloc allocation as a ctypes buffer, freed (weakref
    finalizer, no reference cycle) as soon as the buffer -- and so the last
    numpy array viewing it -- is gone."""
    lib = load()
    n = max(int(nbytes), 1)
    p = C.c_void_p()
    rc = lib.ffddp_host_alloc(n, C.byref(p))
    if rc != 0:
        raise MemoryError(f"ffddp_host_alloc({nbytes}) failed ({rc})")
    buf = (C.c_char * n).from_address(p.value)
    weakref.finalize(buf, lib.ffddp_host_free, C.c_void_p(p.value))
    return buf


def pinned_arrays(specs) -> dict:
    """numpy arrays in one page-locked host allocation (ffddp_host_alloc):
    ffddp_solve_batch copies such arrays by DMA on the slice streams instead
    of through its staging buffer.  specs: {name: (shape, dtype)}."""
    offs, tot = {}, 0
    for k, (shape, dt) in specs.items():
        offs[k] = tot
        tot += (int(np.prod(shape)) * np.dtype(dt).itemsize + 255) // 256 * 256
    buf = _pinned_buffer(tot)
    return {k: np.frombuffer(buf, dtype=dt, count=int(np.prod(shape)), offset=offs[k]).reshape(shape)
            for k, (shape, dt) in specs.items()}


def uptr(a: np.ndarray):
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


_ROBOT = None


def robot_struct() -> Robot:
    global _ROBOT
    if _ROBOT is None:
        _ROBOT = make_robot()
    return _ROBOT


def frame_placement(q, robot: Robot = None) -> tuple[np.ndarray, np.ndarray]:
    """EE placement (R, p) on the host via the library's model code; robot:
    another ffddp_robot (make_robot(mount=...)) than the nominal one."""
    lib = load()
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(7)
    Rm = np.zeros(9)
    p = np.zeros(3)
    rc = lib.ffddp_frame_placement(C.byref(robot_struct() if robot is None else robot), dptr(q), dptr(Rm), dptr(p))
    if rc:
        raise RuntimeError(f"ffddp_frame_placement failed ({rc})")
    return Rm.reshape(3, 3), p


def gravity_torque(q, robot: Robot = None) -> np.ndarray:
    """rnea(q, 0, 0) for a batch (B,7) on the host via the library's model code;
    robot: another ffddp_robot (make_robot(model)) than the nominal one."""
    lib = load()
    q = np.ascontiguousarray(np.atleast_2d(q), dtype=np.float64)
    out = np.zeros_like(q)
    rc = lib.ffddp_gravity_torque(C.byref(robot_struct() if robot is None else robot), q.shape[0], dptr(q), dptr(out))
    if rc:
        raise RuntimeError(f"ffddp_gravity_torque failed ({rc})")
    return out
