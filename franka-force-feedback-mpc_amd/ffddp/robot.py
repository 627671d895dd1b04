"""Franka Panda 7-DoF model data (product side).

Transcribed from /root/reference/assets/scenes/panda_robot.xml:98-199 (link
placements, masses, COMs, full inertias, joint ranges, neutral keyframe
:233).  This replaces example_robot_data.load("panda") +
pin.buildReducedModel (crocoddyl_classical.py:137-145, 189-197), which are not
available offline: armature 0, no hand payload.
The Pinocchio world is the MJCF link0 frame; R_MJ_FROM_PIN = diag(-1,-1,1)
(crocoddyl_classical.py:151).
"""
from __future__ import annotations

import numpy as np

# rotations of the MJCF body quats "1 -1 0 0" (-90 deg about x) and "1 1 0 0" (+90 deg about x)
_RX_M90 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
_RX_P90 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
_I3 = np.eye(3)

JOINT_R = np.stack([_I3, _RX_M90, _RX_P90, _RX_P90, _RX_M90, _RX_P90, _RX_P90])
JOINT_P = np.array(
    [
        [0.0, 0.0, 0.333],
        [0.0, 0.0, 0.0],
        [0.0, -0.316, 0.0],
        [0.0825, 0.0, 0.0],
        [-0.0825, 0.384, 0.0],
        [0.0, 0.0, 0.0],
        [0.088, 0.0, 0.0],
    ]
)
MASS = np.array([4.970684, 0.646926, 3.228604, 3.587895, 1.225946, 1.666555, 0.735522])
COM = np.array(
    [
        [0.003875, 0.002081, -0.04762],
        [-0.003141, -0.02872, 0.003495],
        [0.027518, 0.039252, -0.066502],
        [-0.05317, 0.104419, 0.027454],
        [-0.011953, 0.041065, -0.038437],
        [0.060149, -0.014117, -0.010517],
        [0.010517, -0.004252, 0.061597],
    ]
)
# MJCF fullinertia = (Ixx, Iyy, Izz, Ixy, Ixz, Iyz), about the COM, link frame
_FULL = np.array(
    [
        [0.70337, 0.70661, 0.0091170, -0.00013900, 0.0067720, 0.019169],
        [0.0079620, 0.028110, 0.025995, -0.003925, 0.010254, 0.000704],
        [0.037242, 0.036155, 0.01083, -0.004761, -0.011396, -0.012805],
        [0.025853, 0.019552, 0.028323, 0.007796, -0.001332, 0.008641],
        [0.035549, 0.029474, 0.008627, -0.002117, -0.004037, 0.000229],
        [0.001964, 0.004354, 0.005433, 0.000109, -0.001158, 0.000341],
        [0.012516, 0.010027, 0.004815, -0.000428, -0.001196, -0.000741],
    ]
)
INERTIA = np.stack(
    [np.array([[a, d, e], [d, b, f], [e, f, c]]) for (a, b, c, d, e, f) in _FULL]
)
EE_P = np.array([0.0, 0.0, 0.107])  # panda_link8 / tool body (:189)
EE_R = np.eye(3)
GRAVITY = np.array([0.0, 0.0, -9.81])

Q_LOWER = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
Q_UPPER = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])
Q_NEUTRAL = np.array([0.0, -0.758, 0.0, -2.22, 0.0, 1.43, 0.0])
TAU_LIMITS = np.array([87.0, 87.0, 87.0, 87.0, 12.0, 12.0, 12.0])  # crocoddyl_classical.py:87

R_MJ_FROM_PIN = np.diag([-1.0, -1.0, 1.0])
_c, _s = np.cos(np.deg2rad(135.0)), np.sin(np.deg2rad(135.0))
R_SITE_FROM_EE = np.array([[_c, -_s, 0.0], [_s, _c, 0.0], [0.0, 0.0, 1.0]])  # tool quat (:189)


def _spread(d) -> np.ndarray:
    """S(d) = |d|^2 I - d d^T: the parallel-axis term of a unit mass at offset d."""
    d = np.asarray(d, float)
    return float(d @ d) * np.eye(3) - np.outer(d, d)


class LinkModel:
    """The seven links' inertial parameters, what a controller believes about
    its arm: mass (7,), com (7, 3) in the link frames, inertia (7, 3, 3) about
    the com in the link frames.  The default is the Panda's (MASS / COM /
    INERTIA).  The kinematics are not part of it.  Immutable by convention:
    with_payload and scaled return new models."""

    def __init__(self, mass=None, com=None, inertia=None):
        self.mass = np.array(MASS if mass is None else mass, dtype=np.float64)
        self.com = np.array(COM if com is None else com, dtype=np.float64)
        self.inertia = np.array(INERTIA if inertia is None else inertia, dtype=np.float64)
        if self.mass.shape != (7,) or self.com.shape != (7, 3) or self.inertia.shape != (7, 3, 3):
            raise ValueError(f"LinkModel: mass (7,), com (7, 3), inertia (7, 3, 3), not {self.mass.shape}, "
                             f"{self.com.shape}, {self.inertia.shape}")

    def with_payload(self, mass: float, com=EE_P, inertia=None) -> "LinkModel":
        """A rigid payload fixed to link 7, combined into it: `mass`, `com`
        (link-7 frame, by default the EE offset) and `inertia` about the
        payload's own com (link-7 axes; None: a point mass).
        m = m7 + mp, c = (m7 c7 + mp cp) / m,
        I = I7 + m7 S(c7 - c) + Ip + mp S(cp - c), S(d) = |d|^2 I - d d^T."""
        mp, cp = float(mass), np.asarray(com, float).reshape(3)
        Ip = np.zeros((3, 3)) if inertia is None else np.asarray(inertia, float).reshape(3, 3)
        if not (np.isfinite(mp) and mp >= 0.0):
            raise ValueError("LinkModel.with_payload: the payload mass must be finite and >= 0")
        m7, c7, I7 = self.mass[6], self.com[6], self.inertia[6]
        m = m7 + mp
        c = (m7 * c7 + mp * cp) / m
        out = LinkModel(self.mass, self.com, self.inertia)
        out.mass[6] = m
        out.com[6] = c
        out.inertia[6] = I7 + m7 * _spread(c7 - c) + Ip + mp * _spread(cp - c)
        return out

    def scaled(self, mass_scale) -> "LinkModel":
        """Every link's mass times its factor (a scalar or (7,)); the inertia
        scales with the mass, the com is kept."""
        f = np.broadcast_to(np.asarray(mass_scale, float), (7,))
        if not (np.all(np.isfinite(f)) and np.all(f > 0.0)):
            raise ValueError("LinkModel.scaled: factors must be finite and > 0")
        return LinkModel(self.mass * f, self.com, self.inertia * f[:, None, None])


def _check_rotation(Rm, who: str) -> np.ndarray:
    Rm = np.array(Rm, dtype=np.float64)
    if Rm.shape != (3, 3) or not np.all(np.isfinite(Rm)):
        raise ValueError(f"{who}: a rotation is a finite (3, 3) array")
    if np.max(np.abs(Rm.T @ Rm - np.eye(3))) > 1e-9 or abs(np.linalg.det(Rm) - 1.0) > 1e-9:
        raise ValueError(f"{who}: the matrix is not a rotation (orthonormal to 1e-9, determinant +1)")
    return Rm


def _check_vector(v, who: str) -> np.ndarray:
    v = np.array(v, dtype=np.float64)
    if v.shape != (3,) or not np.all(np.isfinite(v)):
        raise ValueError(f"{who}: a vector is a finite (3,) array")
    return v


class Mount:
    """Where the arm's base stands in the planning world and which way gravity
    points there, what a controller believes about its mounting: base_R (3, 3)
    and base_p (3,), the placement of joint 1 in the planning (Pinocchio)
    world, and gravity (3,).  The default is the nominal Panda's (JOINT_R[0],
    JOINT_P[0], GRAVITY).  ``frame``: (R, p) of the planning frame in the
    nominal Pinocchio world when the mount re-expresses the unchanged physical
    system (in_frame, table_tilt), None for the nominal mount's identity and
    for a physically moved base (remounted).  Immutable by convention."""

    def __init__(self, base_R=None, base_p=None, gravity=None):
        self.base_R = _check_rotation(JOINT_R[0] if base_R is None else base_R, "Mount: base_R")
        self.base_p = _check_vector(JOINT_P[0] if base_p is None else base_p, "Mount: base_p")
        self.gravity = _check_vector(GRAVITY if gravity is None else gravity, "Mount: gravity")
        self.frame = None

    @classmethod
    def in_frame(cls, R, p) -> "Mount":
        """The unchanged physical system seen from a frame M with pose
        x_W = R x_M + p in the Pinocchio world: base_R = R^T JOINT_R[0],
        base_p = R^T (JOINT_P[0] - p), gravity = R^T GRAVITY.  Keeps (R, p) as
        ``frame``."""
        R, p = _check_rotation(R, "Mount.in_frame: R"), _check_vector(p, "Mount.in_frame: p")
        m = cls(R.T @ JOINT_R[0], R.T @ (JOINT_P[0] - p), R.T @ GRAVITY)
        m.frame = (R, p)
        return m

    @classmethod
    def remounted(cls, R, p) -> "Mount":
        """A physically moved base (wall, ceiling, pedestal): the base frame has
        pose (R, p) in the world, base_R = R JOINT_R[0], base_p = R JOINT_P[0]
        + p; gravity is the world's.  ``frame`` is None."""
        R, p = _check_rotation(R, "Mount.remounted: R"), _check_vector(p, "Mount.remounted: p")
        return cls(R @ JOINT_R[0], R @ JOINT_P[0] + p, GRAVITY)

    @classmethod
    def table_tilt(cls, tilt_deg: float) -> "Mount":
        """in_frame of the table's frame at tilt_deg: plant.table_plane's
        rotation about the MuJoCo world's y axis through plant.TABLE_BODY_POS,
        mapped to the Pinocchio world with R_MJ_FROM_PIN.  In that frame the
        table is the flat table."""
        from .plant import TABLE_BODY_POS  # plant imports this module through _abi

        a = np.deg2rad(float(tilt_deg))
        if not np.isfinite(a):
            raise ValueError("Mount.table_tilt: the tilt must be finite")
        Ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        p_mj = TABLE_BODY_POS - Ry @ TABLE_BODY_POS
        D = R_MJ_FROM_PIN
        return cls.in_frame(D.T @ Ry @ D, D.T @ p_mj)

    def obs_frame(self) -> np.ndarray:
        """The (12,) frame row of ffddp_fleet_obs_frame_dev, the planning
        frame's pose in the MuJoCo world: R_mj = D R D row-major, then
        p_mj = D p, D = R_MJ_FROM_PIN.  The identity for a mount without a
        frame."""
        R, p = (np.eye(3), np.zeros(3)) if self.frame is None else self.frame
        D = R_MJ_FROM_PIN
        return np.concatenate([(D @ R @ D.T).reshape(9), D @ p])


def vertical_down_rotation_mj() -> np.ndarray:
    """_make_vertical_down_rotation_mj (crocoddyl_classical.py:241-248)."""
    z = np.array([0.0, 0.0, -1.0])
    x = np.array([1.0, 0.0, 0.0])
    y = np.cross(z, x)
    y /= np.linalg.norm(y) + 1e-12
    x = np.cross(y, z)
    x /= np.linalg.norm(x) + 1e-12
    return np.column_stack([x, y, z])


def rot_mj_to_pin(R_mj_site, R_site_from_pin_ee=R_SITE_FROM_EE) -> np.ndarray:
    """_rot_mj_to_pin (crocoddyl_classical.py:257-258)."""
    return R_MJ_FROM_PIN.T @ np.asarray(R_mj_site, float) @ np.asarray(R_site_from_pin_ee).T


def default_R_des() -> np.ndarray:
    """R_des = _rot_mj_to_pin(vertical down) (crocoddyl_classical.py:157)."""
    return rot_mj_to_pin(vertical_down_rotation_mj())
