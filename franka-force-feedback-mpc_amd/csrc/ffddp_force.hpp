// ffddp_force.hpp — per-instance force setpoint profiles sampled on the device
// (include/ffddp.h: ffddp_fleet_force_refs_dev, ffddp_fleet_metrics_fref_dev).
// A record (FFDDP_FLEET_FORCE_W doubles, ffddp/trajectory.py force_records) is
// f0, f1, t_on, t_ramp: the desired normal contact force goes from f0 to f1,
// linearly over t_ramp seconds from task time t_on (a step at t_on when t_ramp
// is 0).  fleet_force_at evaluates it in trajectory.sample_force's order and
// grouping, without contraction: add, subtract, multiply, divide, min and max
// only, so every kernel that inlines it writes numpy's bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ffddp_consts.hpp"

namespace ffddp {

constexpr int FORCE_BLOCK = 256;

__device__ __forceinline__ double fleet_force_at(const double* __restrict__ rec, double t) {
#pragma clang fp contract(off)
  const double f0 = rec[FFDDP_FLEET_FORCE_F0], f1 = rec[FFDDP_FLEET_FORCE_F1];
  const double t_on = rec[FFDDP_FLEET_FORCE_T_ON], t_ramp = rec[FFDDP_FLEET_FORCE_T_RAMP];
  double s;
  if (t_ramp > 0.0)
    s = fmin(fmax((t - t_on) / t_ramp, 0.0), 1.0);
  else
    s = t >= t_on ? 1.0 : 0.0;
  return f0 + (f1 - f0) * s;
}

// one lane per (instance, knot), flat index: a wave writes consecutive doubles.
// Knot k of instance b is sampled at (T.t - delay_b) + k dt_ocp, the task
// sampler's knot times (ffddp_task.hpp); an instance beyond the records takes
// fn_default at every knot.
__global__ __launch_bounds__(FORCE_BLOCK) void k_fleet_force_refs(int B, int N, double dt_ocp, ffddp_fleet_tasks T,
                                                                  const double* __restrict__ frec, int rows,
                                                                  double fn_default, double* __restrict__ force_ref) {
#pragma clang fp contract(off)
  const long g = (long)blockIdx.x * FORCE_BLOCK + threadIdx.x;
  if (g >= (long)B * (N + 1)) return;
  const long b = g / (N + 1);
  const int k = (int)(g - b * (N + 1));
  if (b >= rows) {
    force_ref[g] = fn_default;
    return;
  }
  const double delay = T.rec ? T.rec[b * FFDDP_FLEET_TASK_W + FFDDP_FLEET_TASK_DELAY] : 0.0;
  const double t0 = T.t - delay;
  const double t = t0 + (double)k * dt_ocp;
  force_ref[g] = fleet_force_at(frec + b * FFDDP_FLEET_FORCE_W, t);
}

}  // namespace ffddp
