// ffddp_task.hpp — per-instance task records sampled on the device
// (include/ffddp.h: ffddp_fleet_task_refs_dev / ffddp_fleet_pre_task_dev).
// A record (FFDDP_FLEET_TASK_W doubles, ffddp/trajectory.py task_records)
// holds the closure constants of make_approach_then_circle and
// with_contact_hold as the host computed them; fleet_task_ref evaluates it at
// one knot in trajectory.py's order and grouping, without contraction, so
// every kernel that inlines it writes the same bits and every entry outside
// the circle phase carries numpy's.  The circle phase calls the library
// sincos (omega * t grows with the run; the lean sincos_ of ffddp_math.hpp is
// for joint angles), which agrees with numpy's to rounding only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ffddp_consts.hpp"

namespace ffddp {

constexpr int TASK_BLOCK = 256;

// the trajectory's surface flag at task time t: neither the pre nor the approach phase
__device__ __forceinline__ bool fleet_task_surface(const double* __restrict__ rec, double t) {
#pragma clang fp contract(off)
  const double t_pre = rec[FFDDP_FLEET_TASK_T_PRE];
  const bool pre = t_pre > 0.0 && t < t_pre;
  return !pre && !(t < t_pre + rec[FFDDP_FLEET_TASK_T_APPROACH]);
}

// Knot k of the instance's references at task time t0: o[0..5] = (p, v) in the
// Pinocchio frame (R_MJ_FROM_PIN = diag(-1, -1, 1), minus p_site_minus_frame,
// as k_build), the return value the surface flag at the knot.
__device__ __forceinline__ bool fleet_task_ref(const double* __restrict__ rec, const double psf[3], double t0, int k,
                                               double dt_ocp, double* __restrict__ o) {
#pragma clang fp contract(off)
  const double t = t0 + (double)k * dt_ocp;
  const double t_pre = rec[FFDDP_FLEET_TASK_T_PRE], t_app = rec[FFDDP_FLEET_TASK_T_APPROACH];
  double p[3], v[3];
  bool surf;
  const bool pre = t_pre > 0.0 && t < t_pre;
  if (pre || t < t_pre + t_app) {
    const double* p0 = rec + (pre || !(t_pre > 0.0) ? FFDDP_FLEET_TASK_P_START : FFDDP_FLEET_TASK_P_PRE);
    const double* p1 = rec + (pre ? FFDDP_FLEET_TASK_P_PRE : FFDDP_FLEET_TASK_P_CS);
    const double tau = pre ? t : t - t_pre, dur = pre ? t_pre : t_app;
    const double sl = tau / dur, sc = fmin(fmax(sl, 0.0), 1.0);
    const double s = sc * sc * (3.0 - 2.0 * sc), dsdt = 6.0 * sc * (1.0 - sc) / dur;
    for (int i = 0; i < 3; ++i) {
      p[i] = (1.0 - s) * p0[i] + s * p1[i];
      v[i] = dsdt * (p1[i] - p0[i]);
    }
    surf = false;
  } else if (t < rec[FFDDP_FLEET_TASK_T_HOLD_END]) {  // with_contact_hold
    for (int i = 0; i < 3; ++i) p[i] = rec[FFDDP_FLEET_TASK_P_HOLD + i], v[i] = 0.0;
    surf = true;
  } else {
    const double radius = rec[FFDDP_FLEET_TASK_RADIUS], omega = rec[FFDDP_FLEET_TASK_OMEGA];
    const double th = omega * (t - (t_pre + t_app));
    double sn, cs;
    sincos(th, &sn, &cs);
    p[0] = rec[FFDDP_FLEET_TASK_CENTER] + radius * cs;
    p[1] = rec[FFDDP_FLEET_TASK_CENTER + 1] + radius * sn;
    p[2] = rec[FFDDP_FLEET_TASK_Z_CONTACT];
    v[0] = -radius * omega * sn;
    v[1] = radius * omega * cs;
    v[2] = 0.0;
    surf = true;
  }
  o[0] = -p[0] - psf[0];
  o[1] = -p[1] - psf[1];
  o[2] = p[2] - psf[2];
  o[3] = -v[0];
  o[4] = -v[1];
  o[5] = v[2];
  return surf;
}

// the sampler alone: one thread per (instance, knot); knot 0's flag is the hint
__global__ __launch_bounds__(TASK_BLOCK) void k_fleet_task_refs(int B, int N, double dt_ocp, ffddp_fleet_tasks T,
                                                                const double* __restrict__ t,
                                                                double* __restrict__ node_ref,
                                                                uint8_t* __restrict__ hint) {
  const long g = (long)blockIdx.x * TASK_BLOCK + threadIdx.x;
  if (g >= (long)B * (N + 1)) return;
  const long b = g / (N + 1);
  const int k = (int)(g - b * (N + 1));
  const bool surf = fleet_task_ref(T.rec + b * FFDDP_FLEET_TASK_W, T.p_site_minus_frame, t[b], k, dt_ocp, node_ref + g * 6);
  if (k == 0) hint[b] = surf ? 1 : 0;
}

}  // namespace ffddp
