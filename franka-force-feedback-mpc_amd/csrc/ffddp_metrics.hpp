// ffddp_metrics.hpp — the closed-loop sweep's task metrics accumulated on the
// device (include/ffddp.h: ffddp_fleet_metrics_dev).  One call folds one plant
// record per instance -- the observation after a tick's command -- into the
// per-instance running sums, maxima and counts that runlog.summary_metrics and
// the sweep's solver-health counters are made of, so a run of any length
// returns FFDDP_FLEET_METRICS_W doubles per instance instead of its per-tick
// logs.  One lane is one instance and owns its column of the field-major
// accumulators acc [W][ld]: the lanes of a wave touch consecutive doubles in
// every access, nothing is shared, and a sum is sequential in tick order, so it
// is the same from run to run.  The per-tick terms are compiled without
// contraction in the host summary's order and grouping (fleet.py
// _run_sweep_device, runlog._rms): adds, multiplies and square roots only, so
// they are numpy's bits; the reference position of a task record comes from
// fleet_task_ref (ffddp_task.hpp) at knot 0, the pre kernel's sampler.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ffddp_consts.hpp"
#include "ffddp_force.hpp"
#include "ffddp_task.hpp"

namespace ffddp {

constexpr int METRICS_BLOCK = 256;

// np.max's running maximum: a NaN on either side stays (fmax alone drops it)
__device__ __forceinline__ double metrics_max(double m, double x) {
  return (m != m || x != x) ? __builtin_nan("") : fmax(m, x);
}

// the force reference of instance b at series time ts: the scalar, or its own record's
__device__ __forceinline__ double metrics_force_ref(long, double, double fn_des) { return fn_des; }
__device__ __forceinline__ double metrics_force_ref(long b, double ts, double fn_des, const double* __restrict__ frec,
                                                    int frows) {
  return b < frows ? fleet_force_at(frec + b * FFDDP_FLEET_FORCE_W, ts) : fn_des;
}

// TASK: instance b's reference is its own record's at (T.t - delay) + dt (rows
// records; an instance beyond them has no reference: NaN); else the shared row
// p_ref at ts.
// k_fleet_metrics<TASK>: the force error is against the scalar fn_des;
// k_fleet_metrics<TASK, const double*, int>: the trailing arguments are (force
// records, their count) and instance b's reference is its own record's at ts
// (ffddp_force.hpp), fn_des beyond the records.  The pack keeps the first
// instantiation's arguments, and so its code, what they were.
template <bool TASK, class... ForceArgs>
__global__ __launch_bounds__(METRICS_BLOCK) void k_fleet_metrics(
    int B, long ld, const double* __restrict__ obs, long ld_obs, ffddp_fleet_tasks T, int rows, double dt,
    const double* __restrict__ p_ref, double ts1, const double* __restrict__ t_phase, double fn_des,
    const double* __restrict__ info, const uint8_t* __restrict__ need, const int32_t* __restrict__ fail,
    double* __restrict__ acc, ForceArgs... force_args) {
#pragma clang fp contract(off)
  const long b = (long)blockIdx.x * METRICS_BLOCK + threadIdx.x;
  if (b >= B) return;
  const double* o = obs + b * ld_obs;
  double ts, p[3];
  if (TASK) {
    if (b < rows) {
      const double* rec = T.rec + b * FFDDP_FLEET_TASK_W;
      ts = (T.t - rec[FFDDP_FLEET_TASK_DELAY]) + dt;
      const double zero[3] = {0.0, 0.0, 0.0};
      double r[6];
      fleet_task_ref(rec, zero, ts, 0, 0.0, r);  // the Pinocchio-frame knot, read back: both maps are exact
      p[0] = -r[0], p[1] = -r[1], p[2] = r[2];
    } else {
      ts = __builtin_nan("");
      p[0] = p[1] = p[2] = __builtin_nan("");
    }
  } else {
    ts = ts1;
    p[0] = p_ref[0], p[1] = p_ref[1], p[2] = p_ref[2];
  }
  const double ex = o[28] - p[0], ey = o[29] - p[1], ez = o[30] - p[2];
  const double s2 = ex * ex + ey * ey;
  const double et = sqrt(s2), e3 = sqrt(s2 + ez * ez);
  const double fn = o[46] * (o[47] > 0.5 ? 1.0 : 0.0);
  const double contact = fn > 0.5 ? 1.0 : 0.0;
  const bool phase = ts >= t_phase[b];
  const double fref = metrics_force_ref(b, ts, fn_des, force_args...);
  double* a = acc + b;
  const double et2 = et * et;
  a[FFDDP_FLEET_METRICS_N * ld] += 1.0;
  a[FFDDP_FLEET_METRICS_SUM_TAN2 * ld] += et2;
  a[FFDDP_FLEET_METRICS_SUM_3D2 * ld] += e3 * e3;
  a[FFDDP_FLEET_METRICS_SUM_ABS_TAN * ld] += fabs(et);
  a[FFDDP_FLEET_METRICS_SUM_ABS_FN_ERR * ld] += fabs(fn - fref);
  a[FFDDP_FLEET_METRICS_MAX_FN * ld] = metrics_max(a[FFDDP_FLEET_METRICS_MAX_FN * ld], fn);
  a[FFDDP_FLEET_METRICS_SUM_CONTACT * ld] += contact;
  a[FFDDP_FLEET_METRICS_MAX_ERR_3D * ld] = metrics_max(a[FFDDP_FLEET_METRICS_MAX_ERR_3D * ld], e3);
  if (phase) {
    a[FFDDP_FLEET_METRICS_N_PHASE * ld] += 1.0;
    a[FFDDP_FLEET_METRICS_SUM_TAN2_PHASE * ld] += et2;
    a[FFDDP_FLEET_METRICS_SUM_CONTACT_PHASE * ld] += contact;
    a[FFDDP_FLEET_METRICS_SUM_FN_PHASE * ld] += fn;
  }
  if (info) {
    const double* f = info + b * FFDDP_FLEET_INFO_W;
    if (f[4] != 0.0) a[FFDDP_FLEET_METRICS_UNSTABLE_TICKS * ld] += 1.0;
    if (f[7] > 0.0) a[FFDDP_FLEET_METRICS_NEG_ACCEPTED_TICKS * ld] += 1.0;
    if (f[0] == 0.0) a[FFDDP_FLEET_METRICS_NOT_OK_TICKS * ld] += 1.0;
    if (!need || need[b] != 0) a[FFDDP_FLEET_METRICS_SOLVED_TICKS * ld] += 1.0;
  }
  if (fail) a[FFDDP_FLEET_METRICS_PLANT_FAIL * ld] += (double)fail[b];
}

}  // namespace ffddp
