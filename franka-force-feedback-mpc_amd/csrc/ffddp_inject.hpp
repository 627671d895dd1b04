// ffddp_inject.hpp — the closed-loop sweep's actuation-uncertainty injector
// on the device (include/ffddp.h: ffddp_fleet_inject_obs_dev /
// ffddp_fleet_inject_cmd_dev / ffddp_fleet_noise_dev): what
// BatchedUncertaintyInjector (ffddp/uncertainty.py) does per tick on the host,
// bit for bit.  Everything is per instance and per joint, so one lane is one
// (instance, joint): lane t works on instance t / 7, joint t % 7, and
// neighbouring lanes touch neighbouring doubles of the [.][B][14] / [.][B][7]
// rings and of the outputs.  The ring slots come from the tick number the
// host passes; nothing is counted on the device.  No contraction anywhere:
// the sums are numpy's, in the host class's order and grouping.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ffddp_consts.hpp"

namespace ffddp {

constexpr int INJECT_BLOCK = 256;
constexpr int INJECT_QV = 2 * NQ;  // a ring row: (q, dq)

// Philox4x64-10 (Salmon et al., SC'11; the constants of Random123 and numpy's
// philox.h): ten rounds, the key bumped by the Weyl constants between rounds.
__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0,
                                              uint64_t k1, uint64_t w[4]) {
  constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t hi0 = __umul64hi(M0, c0), lo0 = M0 * c0;
    const uint64_t hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// Box-Muller on one pair of words: u1 in (0, 1], u2 in [0, 1), 53 bits each.
__device__ __forceinline__ void inject_box_muller(uint64_t wa, uint64_t wb, double& z0, double& z1) {
#pragma clang fp contract(off)
  const double u1 = (double)((wa >> 11) + 1) * 0x1.0p-53;
  const double u2 = (double)(wb >> 11) * 0x1.0p-53;
  const double r = sqrt(-2.0 * log(u1));
  const double t = 6.283185307179586 * u2;
  z0 = r * cos(t);
  z1 = r * sin(t);
}

// Joint j's four normals of tick k: q, dq, tau (observation), tau (command).
__device__ __forceinline__ void inject_philox_normals(uint64_t seed, int k, int j, double zn[4], uint64_t w[4]) {
  philox4x64_10((uint64_t)k + 1, (uint64_t)j, 0, 0, seed, INJECT_PHILOX_TAG, w);
  inject_box_muller(w[0], w[1], zn[0], zn[1]);
  inject_box_muller(w[2], w[3], zn[2], zn[3]);
}

// A row's delay for a ring of `depth` + 1 slots: the scalar when no array is given, else the row's entry
// clamped into [0, depth], so that no value can index outside the ring.
__device__ __forceinline__ int inject_row_delay(const int32_t* __restrict__ d, int r, int depth) {
  if (!d) return depth;
  const int x = d[r];
  return x < 0 ? 0 : (x > depth ? depth : x);
}

// A row's delays and sigmas (ffddp_fleet_inject_rows) over the scalars of ffddp_fleet_inject: the ring moduli
// no, nc and the sigma triple sg.  An instance with the delay d uses the slots 0..d of its ring column.
__device__ __forceinline__ void inject_row_profile(const ffddp_fleet_inject& I, int r, int& no, int& nc, double sg[3],
                                                   const ffddp_fleet_inject_rows& W) {
  no = inject_row_delay(W.d_obs, r, I.d_obs) + 1;
  nc = inject_row_delay(W.d_cmd, r, I.d_cmd) + 1;
  if (W.sigma) sg[0] = W.sigma[3 * r], sg[1] = W.sigma[3 * r + 1], sg[2] = W.sigma[3 * r + 2];
}

// observation_for_controller.  k_fleet_inject_obs<false>: the scalars of I for every instance;
// k_fleet_inject_obs<true, ffddp_fleet_inject_rows>: the trailing argument carries each row's own delays and
// sigmas.  The pack keeps the first instantiation's arguments, and so its code, what they were.
template <bool ROWS, class... RowArgs>
__global__ __launch_bounds__(INJECT_BLOCK) void k_fleet_inject_obs(
    int B, ffddp_fleet_inject I, int k, const double* __restrict__ z, const double* __restrict__ q,
    const double* __restrict__ v, long ld, const double* __restrict__ tau_filt, double* __restrict__ qv_ctrl,
    double* __restrict__ tau_hat, double* __restrict__ tau_ctrl, RowArgs... row_args) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * INJECT_BLOCK + threadIdx.x;
  if (t >= (long)B * NU) return;
  const long b = t / NU;
  const int j = (int)(t - b * NU);
  const double qj = q[b * ld + j], vj = v[b * ld + j];
  double* out = qv_ctrl + b * INJECT_QV;
  const int r = I.row[b];
  if (r < 0 || r >= I.rows) {  // no injector: the plant's record, and its torque filter
    out[j] = qj;
    out[NQ + j] = vj;
    if (tau_filt) {
      const double f = tau_filt[t];
      if (tau_hat) tau_hat[t] = f;
      if (tau_ctrl) tau_ctrl[t] = f;
    }
    return;
  }
  // the delay line: deque(maxlen).append, the oldest slot takes the newest entry
  int no = I.d_obs + 1, nc = I.d_cmd + 1;
  double sg[3] = {I.sigma_q, I.sigma_dq, I.sigma_tau};
  if constexpr (ROWS) inject_row_profile(I, r, no, nc, sg, row_args...);
  const long so = (long)B * INJECT_QV;
  double* ring = I.obs_ring + b * INJECT_QV;
  if (k == 0) {
    for (int s = 0; s < no; ++s) ring[s * so + j] = qj, ring[s * so + NQ + j] = vj;
  } else {
    const long wo = (long)((k - 1) % no) * so;
    ring[wo + j] = qj;
    ring[wo + NQ + j] = vj;
  }
  const long ro = (long)(k % no) * so;
  const double qo = ring[ro + j], vo = ring[ro + NQ + j];
  double zn[4];
  if (I.noise == FFDDP_INJECT_NOISE_PHILOX) {
    uint64_t w[4];
    inject_philox_normals(I.seed[r], k, j, zn, w);
  } else {
    const double* zr = z + (long)r * FFDDP_INJECT_NZ;
    for (int i = 0; i < 4; ++i) zn[i] = zr[i * NU + j];
  }
  out[j] = qo + (0.0 + sg[0] * zn[0]);
  out[NQ + j] = vo + (0.0 + sg[1] * zn[1]);
  // the torque measurement and its filter (_tau_hat on the oldest command)
  const double cmd = I.cmd_ring[(long)(k % nc) * B * NU + t];
  const double th = I.a[r] * cmd + I.b[r] + (0.0 + sg[2] * zn[2]);
  const double tf = (1.0 - I.lpf) * I.tau_hat_filt[t] + I.lpf * th;
  I.tau_hat_filt[t] = tf;
  I.z_cmd[t] = zn[3];
  if (tau_hat) tau_hat[t] = th;
  if (tau_ctrl) tau_ctrl[t] = tf;
}

// command_for_plant; the instantiations as k_fleet_inject_obs's
template <bool ROWS, class... RowArgs>
__global__ __launch_bounds__(INJECT_BLOCK) void k_fleet_inject_cmd(int B, ffddp_fleet_inject I, int k,
                                                                   const double* __restrict__ tau_cmd,
                                                                   double* __restrict__ tau_app, RowArgs... row_args) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * INJECT_BLOCK + threadIdx.x;
  if (t >= (long)B * NU) return;
  const long b = t / NU;
  const int r = I.row[b];
  if (r < 0 || r >= I.rows) return;  // post's scale * tau_cmd stays
  int no = 1, nc = I.d_cmd + 1;
  double sg[3] = {I.sigma_q, I.sigma_dq, I.sigma_tau};
  if constexpr (ROWS) inject_row_profile(I, r, no, nc, sg, row_args...);
  const long sc = (long)B * NU;
  I.cmd_ring[(long)(k % nc) * sc + t] = tau_cmd[t];
  const double cmd = I.cmd_ring[(long)((k + 1) % nc) * sc + t];
  tau_app[t] = I.a[r] * cmd + I.b[r] + (0.0 + sg[2] * I.z_cmd[t]);
}

// the Philox source alone: z [B][28] and, when asked for, the raw blocks [B][7][4]
__global__ __launch_bounds__(INJECT_BLOCK) void k_fleet_noise(int B, const uint64_t* __restrict__ seed, int k,
                                                              double* __restrict__ z, uint64_t* __restrict__ words) {
  const long t = (long)blockIdx.x * INJECT_BLOCK + threadIdx.x;
  if (t >= (long)B * NU) return;
  const long b = t / NU;
  const int j = (int)(t - b * NU);
  double zn[4];
  uint64_t w[4];
  inject_philox_normals(seed[b], k, j, zn, w);
  for (int i = 0; i < 4; ++i) {
    z[b * FFDDP_INJECT_NZ + i * NU + j] = zn[i];
    if (words) words[t * 4 + i] = w[i];
  }
}

}  // namespace ffddp
