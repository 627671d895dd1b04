"""OCP configuration mirroring the reference's controller configs.

`OcpConfig` carries exactly the ClassicalMPCConfig / ForceFeedbackMPCConfig
fields that _build_problem/_make_dam read (crocoddyl_classical.py:12-110,
521-728; crocoddyl_force_feedback.py:12-146, 776-1009).  `classical_preset`
and `ff_preset` are the benchmark-mode presets of src/run/run_classical.py:
269-315 and src/run/run_force_feedback.py:272-330.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _abi
from . import robot as R


@dataclass
class OcpConfig:
    variant: str = "classical"  # "classical" | "ff"
    horizon: int = 30
    dt: float = 0.01
    contact_model: str = "normal_1d"
    use_box_fddp: bool = True
    z_press: float = 0.0065
    w_ee_pos: float = 1.2e3
    w_ee_ori: float = 5.0e1
    ori_weights: np.ndarray = field(default_factory=lambda: np.array([2.4, 2.4, 0.3]))
    w_posture: float = 1.5e-1
    w_v: float = 8.0e-2
    v_damp_weights: np.ndarray = field(default_factory=lambda: np.array([1.0, 1.0, 1.0, 1.0, 0.4, 0.4, 0.4]))
    w_tau: float = 8.0e-4
    w_tau_soft_limits: float = 2.0
    tau_soft_limit_margin: float = 0.2
    w_q_soft_limits: float = 8.0
    q_soft_limit_margin: float = 0.05
    w_tangent_pos: float = 2.6e3
    w_tangent_vel: float = 7.0e2
    w_plane_z: float = 1.2e3
    w_vz: float = 5.0e2
    w_unilateral: float = 3.0e1
    friction_margin: float = 1e-3
    # friction cone (built only for point3d, crocoddyl_classical.py:678); the
    # benchmark presets switch it off (run_classical.py:292-294: weight 0, mu 1)
    w_friction_cone: float = 0.0
    mu: float = 1.0
    w_fn: float = 2.8e1
    fn_des: float = 22.0
    w_wdamp: float = 6.0e1
    w_wdamp_weights: np.ndarray = field(default_factory=lambda: np.array([1.8, 1.8, 0.3]))
    contact_gains: np.ndarray = field(default_factory=lambda: np.array([140.0, 80.0]))
    contact_inv_damping: float = 1.0e-8
    tau_limits: np.ndarray = field(default_factory=lambda: R.TAU_LIMITS.copy())
    R_des: np.ndarray = field(default_factory=R.default_R_des)
    # force feedback
    ff_alpha: float = 0.0
    w_w: float = 0.0
    w_w_soft_limits: float = 0.0
    w_y: float = 0.0
    y_weights: np.ndarray = field(default_factory=lambda: np.zeros(21))
    use_inner_state_reg: bool = True
    use_inner_tau_reg: bool = True

    @property
    def nc(self) -> int:
        return 3 if str(self.contact_model).strip().lower() in ("point3d", "3d", "rigid3d", "route_a_3d") else 1

    @property
    def nx(self) -> int:
        return 21 if self.variant == "ff" else 14

    def to_struct(self) -> _abi.OcpConfig:
        c = _abi.OcpConfig()
        c.variant = _abi.FFDDP_FORCE_FEEDBACK if self.variant == "ff" else _abi.FFDDP_CLASSICAL
        c.horizon = int(self.horizon)
        c.nc = self.nc
        c.use_box = 1 if self.use_box_fddp else 0
        c.dt = max(float(self.dt), 1.0e-6)
        for name in (
            "z_press", "w_ee_pos", "w_ee_ori", "w_posture", "w_v", "w_tau", "w_tau_soft_limits",
            "tau_soft_limit_margin", "w_q_soft_limits", "q_soft_limit_margin", "w_tangent_pos", "w_tangent_vel",
            "w_plane_z", "w_vz", "w_unilateral", "friction_margin", "w_fn", "fn_des", "w_wdamp",
            "contact_inv_damping", "ff_alpha", "w_w", "w_w_soft_limits", "w_y", "w_friction_cone", "mu",
        ):
            setattr(c, name, float(getattr(self, name)))
        _abi._fill(c.ori_weights, self.ori_weights)
        _abi._fill(c.v_damp_weights, self.v_damp_weights)
        _abi._fill(c.q_lower, R.Q_LOWER)
        _abi._fill(c.q_upper, R.Q_UPPER)
        _abi._fill(c.w_wdamp_weights, self.w_wdamp_weights)
        _abi._fill(c.contact_gains, self.contact_gains)
        _abi._fill(c.tau_limits, self.tau_limits)
        _abi._fill(c.R_des, np.asarray(self.R_des, float).reshape(9))
        _abi._fill(c.y_weights, self.y_weights)
        c.use_inner_state_reg = 1 if self.use_inner_state_reg else 0
        c.use_inner_tau_reg = 1 if self.use_inner_tau_reg else 0
        return c


# the scalar cost weights a solve can take per instance (ffddp_solve_batch_wts_dev), in ffddp_ocp_config's order
COST_WEIGHT_NAMES = (
    "w_ee_pos", "w_ee_ori", "w_wdamp", "w_posture", "w_v", "w_tau", "w_tau_soft_limits", "w_q_soft_limits",
    "w_tangent_pos", "w_tangent_vel", "w_plane_z", "w_vz", "w_unilateral", "w_fn", "w_friction_cone",
    "w_w", "w_w_soft_limits", "w_y",
)
_FF_ONLY = ("w_w", "w_w_soft_limits", "w_y")


def cost_weight_row(cfg, variant: str = None, **overrides) -> np.ndarray:
    """(_abi.COST_W,) float64: the cost-weight row that repeats `cfg` (an
    OcpConfig, or any configuration with the w_* fields) for a solve's
    ``cost_weights``, with named overrides (``w_fn=40.0``).  variant
    ("classical" | "ff", default cfg.variant): the classical solve has no
    force-feedback terms, so w_w, w_w_soft_limits and w_y are 0 there as the
    library takes them.  Which terms exist is the handle's configuration:
    an unknown name, a value that is not finite and >= 0, and a positive
    override of a term the configuration does not build (weight 0 there, the
    force-feedback weights of a classical solve, w_friction_cone without
    point3d) raise ValueError."""
    variant = str(getattr(cfg, "variant", "classical") if variant is None else variant).strip().lower()
    if variant not in ("classical", "ff"):
        raise ValueError(f"cost_weight_row: unknown variant {variant!r}")
    nc3 = str(getattr(cfg, "contact_model", "normal_1d")).strip().lower() in ("point3d", "3d", "rigid3d", "route_a_3d")

    def base(name):
        if name in _FF_ONLY and variant != "ff":
            return 0.0
        if name == "w_friction_cone" and not nc3:
            return 0.0
        return max(float(getattr(cfg, name, 0.0)), 0.0)

    row = np.zeros(_abi.COST_W)
    for name in COST_WEIGHT_NAMES:
        row[_abi.COST_INDEX[name]] = base(name)
    for name, val in overrides.items():
        if name not in _abi.COST_INDEX:
            raise ValueError(f"cost_weight_row: unknown cost weight {name!r} (one of {', '.join(COST_WEIGHT_NAMES)})")
        val = float(val)
        if not (np.isfinite(val) and val >= 0.0):
            raise ValueError(f"cost_weight_row: {name} must be finite and >= 0, not {val!r}")
        if val > 0.0 and not base(name) > 0.0:
            raise ValueError(f"cost_weight_row: {name} = {val!r}, but the configuration does not build that term "
                             "(its weight there is 0)")
        row[_abi.COST_INDEX[name]] = val
    return row


def torque_limit_rows(cfg, limits) -> np.ndarray:
    """(B, _abi.TAU_LIM_W) float64: the torque-limit rows of a solve's
    ``torque_limits`` (ffddp_solve_batch_lim_dev) for `limits` of shape (B, 7),
    instance b's tau_limits, built by the library's own code
    (ffddp_torque_limit_rows) from `cfg`'s tau_soft_limit_margin.  A row of
    cfg.tau_limits repeats the handle's constants.  A limit that is not finite
    and > 0, or another shape, raises ValueError."""
    import ctypes as C

    lim = np.ascontiguousarray(limits, dtype=np.float64)
    if lim.ndim != 2 or lim.shape[1] != 7:
        raise ValueError(f"torque_limit_rows: limits must have shape (B, 7), not {lim.shape}")
    if not (np.all(np.isfinite(lim)) and np.all(lim > 0.0)):
        raise ValueError("torque_limit_rows: limits must be finite and > 0")
    st = cfg.to_struct() if hasattr(cfg, "to_struct") else cfg
    rows = np.zeros((lim.shape[0], _abi.TAU_LIM_W))
    rc = _abi.load().ffddp_torque_limit_rows(C.byref(st), int(lim.shape[0]), _abi.dptr(lim), _abi.dptr(rows))
    if rc:
        raise ValueError(f"ffddp_torque_limit_rows failed ({rc})")
    return rows


def link_model_rows(models) -> np.ndarray:
    """(B, _abi.LINK_W) float64: the link-model rows of a solve's
    ``link_model`` (ffddp_solve_batch_mdl_dev) for B robot.LinkModel objects
    (None: the nominal model), packed by the library's own code
    (ffddp_link_model_rows).  A row of the handle's model repeats the handle's
    constants.  A mass that is not finite and > 0, or a com or inertia entry
    that is not finite, raises ValueError."""
    import ctypes as C

    from . import robot as R

    models = [R.LinkModel() if m is None else m for m in models]
    B = len(models)
    robots = (_abi.Robot * max(B, 1))()
    for b, m in enumerate(models):
        robots[b] = _abi.make_robot(m)
    rows = np.zeros((B, _abi.LINK_W))
    rc = _abi.load().ffddp_link_model_rows(robots, B, _abi.dptr(rows))
    if rc:
        raise ValueError(f"link_model_rows: a mass must be finite and > 0, com and inertia finite "
                         f"(ffddp_link_model_rows failed, {rc})")
    return rows


def mount_rows(mounts) -> np.ndarray:
    """(B, _abi.MOUNT_W) float64: the mount rows of a solve's ``mount``
    (ffddp_solve_batch_mnt_dev) for B robot.Mount objects (None: the nominal
    mount), packed by the library's own code (ffddp_mount_rows).  A row of the
    handle's mount repeats the handle's constants.  A non-finite entry raises
    ValueError (robot.Mount itself checks that base_R is a rotation)."""
    from . import robot as R

    mounts = [R.Mount() if m is None else m for m in mounts]
    B = len(mounts)
    robots = (_abi.Robot * max(B, 1))()
    for b, m in enumerate(mounts):
        robots[b] = _abi.make_robot(mount=m)
    rows = np.zeros((B, _abi.MOUNT_W))
    rc = _abi.load().ffddp_mount_rows(robots, B, _abi.dptr(rows))
    if rc:
        raise ValueError(f"mount_rows: base_R, base_p and gravity must be finite (ffddp_mount_rows failed, {rc})")
    return rows


def classical_preset(horizon: int = 30, contact_model: str = "normal_1d") -> OcpConfig:
    """run_classical.py:269-315 (benchmark mode).  The reference preset uses N=36; BASELINE uses 30 (R9)."""
    return OcpConfig(variant="classical", horizon=horizon, contact_model=contact_model)


def ff_alpha_ocp(cutoff_hz: float, dt_ocp: float) -> float:
    """_ff_alpha_ocp (crocoddyl_force_feedback.py:493-497)."""
    wc = 2.0 * np.pi * float(max(cutoff_hz, 0.0))
    return float(np.clip(np.exp(-wc * float(dt_ocp)), 0.0, 0.999999))


def ff_preset(horizon: int = 30, contact_model: str = "normal_1d") -> OcpConfig:
    """run_force_feedback.py:272-330 (benchmark mode).  The reference preset uses N=40 (R9)."""
    return OcpConfig(
        variant="ff",
        horizon=horizon,
        contact_model=contact_model,
        w_ee_pos=1.2e3,
        w_ee_ori=4.5e1,
        ori_weights=np.array([2.2, 2.2, 0.3]),
        w_posture=1.0e-1,
        w_v=5.0e-2,
        w_tau=8.0e-4,
        w_tau_soft_limits=1.5,
        w_q_soft_limits=8.0,
        w_tangent_pos=3.6e3,
        w_tangent_vel=1.2e3,
        w_plane_z=9.0e2,
        w_vz=3.0e2,
        w_unilateral=3.0e1,
        w_fn=3.0e1,
        fn_des=22.0,
        w_wdamp=7.0e1,
        w_wdamp_weights=np.array([1.8, 1.8, 0.3]),
        contact_gains=np.array([145.0, 85.0]),
        ff_alpha=ff_alpha_ocp(25.0, 0.01),
        w_w=6.0e-4,
        w_w_soft_limits=2.0,
        w_y=8.0e-4,
        y_weights=np.concatenate([[0.15] * 4 + [0.08] * 3, [0.05] * 4 + [0.03] * 3, [0.12] * 4 + [0.08] * 3]),
    )
