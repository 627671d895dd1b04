"""EE reference trajectories sampled per OCP node.

Restates src/tasks/trajectories.py:8-93 (make_approach_then_circle) and the
benchmark-mode wrapper of src/run/run_classical.py:221-264 (contact height,
pre/approach timing and the 0.2 s hold at contact onset).  Pinned by golden
vectors generated from the reference module itself (tests/golden/
make_golden.py -> reference_vectors.npz).
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from ._abi import FLEET_FORCE_W, FLEET_TASK_W

Traj = Callable[[float], Tuple[np.ndarray, np.ndarray, bool]]


def _smoothstep(s: float) -> float:
    s = min(max(s, 0.0), 1.0)
    return s * s * (3.0 - 2.0 * s)


def _dsmoothstep(s: float) -> float:
    s = min(max(s, 0.0), 1.0)
    return 6.0 * s * (1.0 - s)


def make_approach_then_circle(
    center,
    radius: float,
    omega: float,
    z_contact: float,
    t_approach: float = 2.0,
    ee_start=None,
    z_pre=None,
    t_pre: float = 0.0,
) -> Traj:
    """traj(t) -> (p_ref[3], v_ref[3], surface_mode) (trajectories.py:8-93)."""
    center = np.asarray(center, dtype=float).reshape(3).copy()
    radius, omega, z_contact = float(radius), float(omega), float(z_contact)
    t_approach = max(float(t_approach), 1.0e-6)
    t_pre = max(float(t_pre), 0.0)

    p_contact_start = center.copy()
    p_contact_start[0] += radius
    p_contact_start[2] = z_contact
    if ee_start is None:
        p_start = p_contact_start.copy()
        p_start[2] += 0.08
    else:
        p_start = np.asarray(ee_start, dtype=float).reshape(3).copy()
    if z_pre is None:
        z_pre = max(z_contact + 0.05, p_start[2])
    z_pre = float(z_pre)
    p_pre = p_contact_start.copy()
    p_pre[2] = z_pre

    def blend(p0, p1, tau, T):
        s_lin = tau / T
        s = _smoothstep(s_lin)
        dsdt = _dsmoothstep(s_lin) / T
        return (1.0 - s) * p0 + s * p1, dsdt * (p1 - p0)

    def traj(t: float):
        t = float(t)
        if t_pre > 0.0 and t < t_pre:
            p, v = blend(p_start, p_pre, t, t_pre)
            return p, v, False
        if t < t_pre + t_approach:
            p0 = p_pre if t_pre > 0.0 else p_start
            p, v = blend(p0, p_contact_start, t - t_pre, t_approach)
            return p, v, False
        th = omega * (t - (t_pre + t_approach))
        p = center.copy()
        p[0] += radius * np.cos(th)
        p[1] += radius * np.sin(th)
        p[2] = z_contact
        v = np.zeros(3)
        v[0] = -radius * omega * np.sin(th)
        v[1] = radius * omega * np.cos(th)
        return p, v, True

    def sample(ts):
        """traj at every time of ts at once: (P [n][3], V [n][3], surface [n]),
        element for element the same arithmetic as traj (so the same bits)."""
        t = np.asarray(ts, dtype=float).reshape(-1)
        P, V = np.empty((t.size, 3)), np.empty((t.size, 3))
        m_pre = (t < t_pre) if t_pre > 0.0 else np.zeros(t.size, bool)
        m_app = ~m_pre & (t < t_pre + t_approach)
        m_cir = ~(m_pre | m_app)

        def blend_v(sel, p0, p1, tau, T):
            s_lin = tau / T
            sc = np.minimum(np.maximum(s_lin, 0.0), 1.0)
            s_ = sc * sc * (3.0 - 2.0 * sc)
            dsdt = 6.0 * sc * (1.0 - sc) / T
            P[sel] = (1.0 - s_)[:, None] * p0 + s_[:, None] * p1
            V[sel] = dsdt[:, None] * (p1 - p0)

        if m_pre.any():
            blend_v(m_pre, p_start, p_pre, t[m_pre], t_pre)
        if m_app.any():
            blend_v(m_app, p_pre if t_pre > 0.0 else p_start, p_contact_start, t[m_app] - t_pre, t_approach)
        if m_cir.any():
            th = omega * (t[m_cir] - (t_pre + t_approach))
            P[m_cir, 0] = center[0] + radius * np.cos(th)
            P[m_cir, 1] = center[1] + radius * np.sin(th)
            P[m_cir, 2] = z_contact
            V[m_cir, 0] = -radius * omega * np.sin(th)
            V[m_cir, 1] = radius * omega * np.cos(th)
            V[m_cir, 2] = 0.0
        return P, V, m_cir.copy()

    traj.sample = sample
    return traj


def with_contact_hold(base: Traj, t_contact_phase: float, t_hold: float = 0.2) -> Traj:
    """The benchmark runner's wrapper (run_classical.py:246-264): for t_hold
    after the contact onset the reference holds the onset point with zero
    velocity.  Keeps base's vectorised sample()."""
    t_cp, t_end = float(t_contact_phase), float(t_contact_phase) + float(t_hold)

    def traj(t: float):
        p, v, s = base(t)
        if s and float(t) < t_end:
            return np.asarray(base(t_cp)[0], float), np.zeros(3), True
        return p, v, s

    if hasattr(base, "sample"):
        p_hold = np.asarray(base(t_cp)[0], float)

        def sample(ts):
            t = np.asarray(ts, dtype=float).reshape(-1)
            P, V, S = base.sample(t)
            h = S & (t < t_end)
            P[h] = p_hold
            V[h] = 0.0
            return P, V, S

        traj.sample = sample
    return traj


@dataclasses.dataclass
class FleetTask:
    """One instance's task in a device fleet (fleet_loop.DeviceFleetLoop(tasks=...)):
    make_approach_then_circle's arguments, with_contact_hold's, and a start
    ``delay`` in seconds (>= 0): the instance runs the task at time t - delay,
    waiting at the start pose while that is negative (the smoothstep clamps)."""

    center: Sequence[float]
    radius: float
    omega: float
    z_contact: float
    t_approach: float = 2.0
    t_pre: float = 0.0
    ee_start: Optional[Sequence[float]] = None
    z_pre: Optional[float] = None
    t_contact_phase: float = 0.0
    t_hold: float = 0.2
    delay: float = 0.0

    def __post_init__(self):
        if not float(self.delay) >= 0.0:
            raise ValueError(f"FleetTask: delay must be >= 0, not {self.delay!r}")

    def base(self) -> Traj:
        return make_approach_then_circle(center=self.center, radius=self.radius, omega=self.omega,
                                         z_contact=self.z_contact, t_approach=self.t_approach, ee_start=self.ee_start,
                                         z_pre=self.z_pre, t_pre=self.t_pre)

    def traj(self) -> Traj:
        """The task as the host fleets take it (without the delay)."""
        return with_contact_hold(self.base(), self.t_contact_phase, self.t_hold)


# a record's layout: include/ffddp.h FFDDP_FLEET_TASK_*
(_R_CENTER, _R_RADIUS, _R_OMEGA, _R_Z_CONTACT, _R_T_PRE, _R_T_APPROACH, _R_P_START, _R_P_PRE, _R_P_CS, _R_P_HOLD,
 _R_T_HOLD_END, _R_DELAY) = 0, 3, 4, 5, 6, 7, 8, 11, 14, 17, 20, 21


def task_records(tasks: Sequence[FleetTask]) -> np.ndarray:
    """(B, FLEET_TASK_W) float64: what the device sampler needs of each task,
    precomputed with make_approach_then_circle's and with_contact_hold's own
    arithmetic (their closure constants), so the values carry numpy's bits."""
    rec = np.zeros((len(tasks), FLEET_TASK_W))
    for b, k in enumerate(tasks):
        center = np.asarray(k.center, dtype=float).reshape(3).copy()
        radius, omega, z_contact = float(k.radius), float(k.omega), float(k.z_contact)
        t_approach = max(float(k.t_approach), 1.0e-6)
        t_pre = max(float(k.t_pre), 0.0)
        p_cs = center.copy()
        p_cs[0] += radius
        p_cs[2] = z_contact
        if k.ee_start is None:
            p_start = p_cs.copy()
            p_start[2] += 0.08
        else:
            p_start = np.asarray(k.ee_start, dtype=float).reshape(3).copy()
        z_pre = float(max(z_contact + 0.05, p_start[2]) if k.z_pre is None else k.z_pre)
        p_pre = p_cs.copy()
        p_pre[2] = z_pre
        r = rec[b]
        r[_R_CENTER:_R_CENTER + 3], r[_R_RADIUS], r[_R_OMEGA], r[_R_Z_CONTACT] = center, radius, omega, z_contact
        r[_R_T_PRE], r[_R_T_APPROACH] = t_pre, t_approach
        r[_R_P_START:_R_P_START + 3], r[_R_P_PRE:_R_P_PRE + 3], r[_R_P_CS:_R_P_CS + 3] = p_start, p_pre, p_cs
        r[_R_P_HOLD:_R_P_HOLD + 3] = np.asarray(k.base()(float(k.t_contact_phase))[0], float)
        r[_R_T_HOLD_END] = float(k.t_contact_phase) + float(k.t_hold)
        r[_R_DELAY] = float(k.delay)
    return rec


def sample_records(rec: np.ndarray, t) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The device sampler (csrc/ffddp_task.hpp) in numpy: row b of the records
    at task time t[b] (the caller subtracts the delay, as on the device) ->
    (P [B][3], V [B][3], surface [B]) in the MuJoCo world, element for element
    the arithmetic of traj.sample with the hold applied."""
    rec = np.asarray(rec, dtype=float).reshape(-1, FLEET_TASK_W)
    t = np.broadcast_to(np.asarray(t, dtype=float), (rec.shape[0],))
    B = rec.shape[0]
    P, V = np.empty((B, 3)), np.empty((B, 3))
    t_pre, t_app = rec[:, _R_T_PRE], rec[:, _R_T_APPROACH]
    p_start, p_pre, p_cs = (rec[:, o:o + 3] for o in (_R_P_START, _R_P_PRE, _R_P_CS))
    m_pre = (t_pre > 0.0) & (t < t_pre)
    m_app = ~m_pre & (t < t_pre + t_app)
    m_cir = ~(m_pre | m_app)

    def blend_v(sel, p0, p1, tau, T):
        s_lin = tau / T
        sc = np.minimum(np.maximum(s_lin, 0.0), 1.0)
        s_ = sc * sc * (3.0 - 2.0 * sc)
        dsdt = 6.0 * sc * (1.0 - sc) / T
        P[sel] = (1.0 - s_)[:, None] * p0 + s_[:, None] * p1
        V[sel] = dsdt[:, None] * (p1 - p0)

    if m_pre.any():
        blend_v(m_pre, p_start[m_pre], p_pre[m_pre], t[m_pre], t_pre[m_pre])
    if m_app.any():
        p0 = np.where((t_pre > 0.0)[:, None], p_pre, p_start)
        blend_v(m_app, p0[m_app], p_cs[m_app], t[m_app] - t_pre[m_app], t_app[m_app])
    if m_cir.any():
        radius, omega = rec[m_cir, _R_RADIUS], rec[m_cir, _R_OMEGA]
        th = omega * (t[m_cir] - (t_pre[m_cir] + t_app[m_cir]))
        P[m_cir, 0] = rec[m_cir, _R_CENTER] + radius * np.cos(th)
        P[m_cir, 1] = rec[m_cir, _R_CENTER + 1] + radius * np.sin(th)
        P[m_cir, 2] = rec[m_cir, _R_Z_CONTACT]
        V[m_cir, 0] = -radius * omega * np.sin(th)
        V[m_cir, 1] = radius * omega * np.cos(th)
        V[m_cir, 2] = 0.0
    h = m_cir & (t < rec[:, _R_T_HOLD_END])
    P[h] = rec[h, _R_P_HOLD:_R_P_HOLD + 3]
    V[h] = 0.0
    return P, V, m_cir.copy()


@dataclasses.dataclass(frozen=True)
class ForceProfile:
    """One instance's desired normal contact force over its task time (a device
    fleet's ``force_profiles``): f0 before t_on, then linearly to f1 over
    t_ramp seconds; t_ramp = 0 steps at t_on.  ForceProfile(f, f) is the
    constant setpoint f."""

    f0: float
    f1: float
    t_on: float = 0.0
    t_ramp: float = 0.0

    def __post_init__(self):
        vals = (float(self.f0), float(self.f1), float(self.t_on), float(self.t_ramp))
        if not all(np.isfinite(v) for v in vals):
            raise ValueError(f"ForceProfile: every field must be finite, not {vals!r}")
        if vals[0] < 0.0 or vals[1] < 0.0:
            raise ValueError(f"ForceProfile: forces must be >= 0, not f0={self.f0!r}, f1={self.f1!r}")
        if vals[3] < 0.0:
            raise ValueError(f"ForceProfile: t_ramp must be >= 0, not {self.t_ramp!r}")


# a force record's layout: include/ffddp.h FFDDP_FLEET_FORCE_*
_F_F0, _F_F1, _F_T_ON, _F_T_RAMP = 0, 1, 2, 3


def force_records(profiles: Sequence[ForceProfile]) -> np.ndarray:
    """(B, FLEET_FORCE_W) float64: f0, f1, t_on, t_ramp of each profile."""
    rec = np.zeros((len(profiles), FLEET_FORCE_W))
    for b, k in enumerate(profiles):
        rec[b] = float(k.f0), float(k.f1), float(k.t_on), float(k.t_ramp)
    return rec


def sample_force(rec: np.ndarray, t) -> np.ndarray:
    """The device force sampler (csrc/ffddp_force.hpp) in numpy: row b of the
    records at task time t[b] (scalar, (B,) or (B, K); the caller subtracts
    the delay, as on the device) -> the desired normal force, shaped as t
    broadcast against the rows: f0 + (f1 - f0) s with
    s = min(max((t - t_on) / t_ramp, 0), 1), or (t >= t_on) where t_ramp == 0.
    min / max are fmin / fmax, as on the device."""
    rec = np.asarray(rec, dtype=float).reshape(-1, FLEET_FORCE_W)
    t = np.asarray(t, dtype=float)
    col = (lambda i: rec[:, i]) if t.ndim < 2 else (lambda i: rec[:, i][:, None])
    f0, f1, t_on, t_ramp = (col(i) for i in (_F_F0, _F_F1, _F_T_ON, _F_T_RAMP))
    t = np.broadcast_to(t, np.broadcast_shapes(t.shape, f0.shape))
    ramp = t_ramp > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        s_ramp = np.fmin(np.fmax((t - t_on) / np.where(ramp, t_ramp, 1.0), 0.0), 1.0)
    s = np.where(ramp, s_ramp, (t >= t_on).astype(float))
    return f0 + (f1 - f0) * s


# Benchmark scene constants (assets/scenes/panda_table_scene.xml:17-29,
# panda_robot.xml:189-199) and run_classical.py:221-255.
TABLE_CENTER = np.array([-0.5, 0.0, 0.3])
TABLE_HALF_Z = 0.02
TOOL_RADIUS = 0.03


def benchmark_traj(ee_start_mj, radius: float = 0.10, omega: float = 1.5) -> Tuple[Traj, dict]:
    """The benchmark-mode trajectory of run_classical.py:221-264 (MuJoCo world)."""
    z_top = TABLE_CENTER[2] + TABLE_HALF_Z
    z_contact = z_top + TOOL_RADIUS - 8.0e-3
    z_pre = z_contact + 0.05
    center = np.array([TABLE_CENTER[0], TABLE_CENTER[1], z_contact])
    t_approach, t_pre = 0.55, 0.25
    base = make_approach_then_circle(
        center=center, radius=radius, omega=omega, z_pre=z_pre, z_contact=z_contact,
        t_approach=t_approach, ee_start=np.asarray(ee_start_mj, float), t_pre=t_pre,
    )
    t_contact_phase = t_pre + t_approach
    traj = with_contact_hold(base, t_contact_phase, 0.2)
    meta = dict(z_contact=z_contact, z_pre=z_pre, center=center, t_contact_phase=t_contact_phase)
    return traj, meta


def benchmark_task(ee_start_mj, radius: float = 0.10, omega: float = 1.5, delay: float = 0.0) -> FleetTask:
    """benchmark_traj as a FleetTask: ``benchmark_task(ee).traj()`` is ``benchmark_traj(ee)[0]``."""
    z_contact = TABLE_CENTER[2] + TABLE_HALF_Z + TOOL_RADIUS - 8.0e-3
    t_approach, t_pre = 0.55, 0.25
    return FleetTask(center=np.array([TABLE_CENTER[0], TABLE_CENTER[1], z_contact]), radius=radius, omega=omega,
                     z_contact=z_contact, t_approach=t_approach, t_pre=t_pre, ee_start=np.asarray(ee_start_mj, float),
                     z_pre=z_contact + 0.05, t_contact_phase=t_pre + t_approach, t_hold=0.2, delay=delay)
