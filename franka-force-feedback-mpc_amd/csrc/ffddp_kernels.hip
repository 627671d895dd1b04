// ffddp_kernels.hip — batched (Box)FDDP on MI355X (gfx950), fp64.
//
// One solve() of crocoddyl::SolverBoxFDDP (reference call sites
// crocoddyl_classical.py:367 / crocoddyl_force_feedback.py:605) for B
// independent OCP instances, as a fixed sequence of kernels per FDDP
// iteration; all per-instance control flow (regularisation, line-search
// acceptance, feasibility, stopping) lives on the device, masked per instance:
//
//   k_node      calc + calcDiff of every (instance, node), 16-lane group per
//               node: lanes 0..7 run the calc (joint lanes + EE lane, log-depth
//               scans: dynamics, costs, gaps) into the group's LDS, then lane j
//               computes state direction j in closed form (Jacobian column j)
//               and the Gauss-Newton Hessians are assembled across the group.
//   k_backward_w  Riccati backward pass, one wavefront per instance, blocks in
//               LDS; Cholesky (infeasible iterations) or BoxQP gains;
//               regularisation retries inside the kernel.
//   k_forward_g8  line search: one 8-lane group per (instance, step length) —
//               the trials of SolverFDDP::solve evaluated concurrently (the
//               first accepted one is the sequential answer).
//   k_accept    acceptance test / regularisation / stopping (SolverFDDP::solve),
//               one lane per instance; the accepted trial stays in place (the
//               next k_node reads it and writes it into xs / us; k_commit at
//               the end of the solve for the rest).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "ffddp_consts.hpp"
#include "ffddp_copy_pool.hpp"
#include "ffddp_group.hpp"
#include "ffddp_inject.hpp"
#include "ffddp_metrics.hpp"
#include "ffddp_plant.hpp"
#include "ffddp_primal_g8.hpp"
#include "ffddp_rollout.hpp"
#include "ffddp_task.hpp"

using namespace ffddp;

namespace {

constexpr int NODE_GROUP = 16;
#ifndef NODE_BLOCK
#define NODE_BLOCK 64
#endif
constexpr int NODE_GPB = NODE_BLOCK / NODE_GROUP;
#ifndef NODE_WAVES
#define NODE_WAVES 2
#endif
#ifndef QC_UNROLL
#define QC_UNROLL 1
#endif
#ifndef QC_FF_LATE
#define QC_FF_LATE 0  // phase C unroll of FF's latency variant (0: full; FF B=1024 +1.4 % over 1 since the LDS diet)
#endif
// BW_PF_LATE: when k_backward_w issues the loads of the next node's record:
// at the top of the node (0), or after phase D with the record staged into
// LDS at the end of the node (S.R is dead after phase C), so the prefetch
// registers are not live across the gains (1: FF only, 2: both variants)
#ifndef BW_PF_LATE
#define BW_PF_LATE 0
#endif
// backward LDS diet (round 5): BW_DIET_UNION puts Y with the factors and M
// with K in one slot each (FF only, BwSlots), BW_DIET_SLOTS stages the
// per-lane inputs in n-entry arrays (lane l writes slot l mod n) instead of
// 64-entry ones
#ifndef BW_DIET_UNION
#define BW_DIET_UNION 1
#endif
#ifndef BW_DIET_SLOTS
#define BW_DIET_SLOTS 1
#endif
#ifndef BW_WAVES
#define BW_WAVES 1
#endif

struct InstState {
  double preg, cost, dg, dq, stop;
  double ffeas;  // max |fs| of the last calcDiff (the trace's ||ffeas||)
  int is_feasible, was_feasible, done, ok, iter, recalc, accepted, bw_ok;
  int n_iters, n_trials, n_retries, n_backward, n_calc, n_forward;
  int n_eval1, n_eval2;  // line-search trials evaluated by the first / second pass
  int n_neg, n_neg_acc;  // trials judged / accepted by the ascent-direction branch (dVexp < 0)
};

struct Dev {
  int B, N, nx, rec;
  double* rec_buf;   // [B][N+1][rec]
  double* fs;        // [B][N+1][nx]
  double* xs;        // [B][N+1][nx]
  double* us;        // [B][N][7]
  double* K;         // [B][N][7][nx]
  double* k;         // [B][N][7]
  double* w;         // [B][N+1][nx]   Vxx_t fs_t
  double* xs_try;    // [B][T][N+1][nx]
  double* us_try;    // [B][T][N][7]
  double* trial;     // [B][T][2]  cost_try, dv
  int* trial_fail;   // [B][T]
  InstState* st;     // [B]
  int* alist;        // [2][B]  active-instance lists (slice-local indices), double-buffered over iterations
  int* acnt;         // [4]     their lengths; [2 + p]: an instance of the iteration that built list p
                     //         needed more step lengths than the host's first pass (first_width)
  double* trace;     // [B][trace_it][FFDDP_TRACE_W] per-iteration records (CallbackVerbose), or null
  int trace_it;
  const double* fref;  // [B][N+1] desired normal contact force per instance and node (ffddp_solve_batch_fref_dev),
                       //          read by the FR instantiations of k_node / k_forward_g8 only; null: C.fn_ref
  const double* cw;    // [B][FFDDP_COST_W] cost-weight rows (ffddp_solve_batch_wts_dev), read by the CW
                       //          instantiations of k_node / k_forward_g8 only; null: C's weights
  const double* ul;    // [B][FFDDP_TAU_LIM_W] torque-limit rows (ffddp_solve_batch_lim_dev), read by the UL
                       //          instantiations of k_node / k_forward_g8 and by the backward pass's fill of its
                       //          BoxQP bounds; null: C's limits
  const double* md;    // [B][FFDDP_LINK_W] link-model rows (ffddp_solve_batch_mdl_dev), read by the MD
                       //          instantiations of k_node / k_forward_g8 only; null: C.rb's inertial parameters
  uint8_t* uni0;       // [B]  the instance starts from one repeated (x, u) point (k_init; k_node_rep)
  double* rep;         // [B][REP_W]  node 0's stash for k_node_rep (ffddp_primal_g8.hpp)
  const double* mt;    // [B][FFDDP_MOUNT_W] mount rows (ffddp_solve_batch_mnt_dev): base placement and gravity, read by
                       //          the MT instantiations of k_node / k_forward_g8 / k_finalize; null: C.rb's
};

// Active-instance compaction.  Iteration it reads list (it & 1): the
// instances not yet done, packed at the front, so the blocks / groups of the
// per-iteration kernels that carry work are the first ones of the grid and
// the rest exit at once.  Without it a late iteration's few active
// instances are scattered over the whole grid, and a grid larger than one
// wave per SIMD (the 1-wave/SIMD line search with 4 trials) ran its active
// waves in two dispatch rounds.  k_accept appends the instances that
// continue to the other list; k_backward_w zeroes that list's length first.
// marks accumulator registers a0..a39 used, so the kernel's register
// allocation (and its SIMD occupancy) includes them
#define RESERVE_AGPR40() asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39")

// a global-memory pointer (address space 1): stays one after an opaque asm
template <class T> using gptr = __attribute__((address_space(1))) T*;

struct ActiveList {
  const int* list;
  int n;
};
__device__ __forceinline__ ActiveList active_list(const Dev& d, int cur) {
  return ActiveList{d.alist + (long)cur * d.B, d.acnt[cur]};
}

// XCD-aware block order.  The hardware hands consecutive workgroups to the 8
// XCDs round-robin, each XCD with its own L2: an instance's node groups (or
// line-search trials) spread over several blocks would pull its shared lines
// (node references, the iterate, K, the instance state, partly written gap
// lines) into several L2s.  Remap so that each XCD processes one contiguous
// range of the n blocks that carry work; blocks >= n keep their index.
constexpr int N_XCD = 8;
__device__ __forceinline__ long xcd_block(long b, long n) {
  if (b >= n) return b;
  const long q = n / N_XCD, r = n % N_XCD;
  const long x = b % N_XCD, i = b / N_XCD;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ---------------------------------------------------------------------------
// init
// ---------------------------------------------------------------------------
// xs_init / us_init may be d.xs / d.us (warm start in place, ffddp.h): not
// __restrict__; each element is read and written by the same thread
//
// SEL (ffddp_solve_batch_sel_dev): `active` [B] selects the instances that
// solve.  An unselected instance's rows of xs_init / us_init are not read and
// its rows of xs / us / K / k not written; it starts done with no accepted
// trial, so no later kernel visits it (k_commit skips it, k_finalize returns
// on the mask).  The first active list is the selected instances in
// ascending order: a chunk of INIT_BLOCK instances per block, its base the
// number of selected instances before the chunk (counted by the block
// itself), the order inside by ballot and popcount -- a function of the mask
// alone, no atomic append.
constexpr int INIT_BLOCK = 256;
template <bool SEL>
__global__ __launch_bounds__(INIT_BLOCK) void k_init(const DevConsts* __restrict__ Cg, Dev d, const double* xs_init,
                                                     const double* us_init, int is_feasible,
                                                     const uint8_t* __restrict__ active,
                                                     const double* __restrict__ node_ref,
                                                     const uint8_t* __restrict__ surface, int nc) {
  const DevConsts& C = *Cg;
  const int N = C.N, nx = C.nx;
  // Uniform start (k_node_rep): the running nodes 0..N-1 of the instance share
  // one (x, u) bit pattern, and so do the node-reference components that enter
  // the contact dynamics (a surface instance's target point along the
  // constrained axes), so their calc differs from node 0's only in the
  // reference-dependent residuals.  xs_init[N] is the terminal model's and not
  // part of the test.  One wave per instance; bit patterns, not ==, so -0 and
  // NaN do not pass as equal.  node_ref null: the replication is off.
  {
    const int l = threadIdx.x % 64;
    const int nw = (int)gridDim.x * (INIT_BLOCK / 64);
    for (int b = (int)blockIdx.x * (INIT_BLOCK / 64) + threadIdx.x / 64; b < d.B; b += nw) {
      bool same = node_ref != nullptr && N >= 2 && (!SEL || active[b] != 0);
      if (same) {
        const long long* x = reinterpret_cast<const long long*>(xs_init + (long)b * (N + 1) * nx);
        for (int i = l; i < (N - 1) * nx; i += 64) same = same && x[nx + i] == x[i % nx];
        const long long* u = reinterpret_cast<const long long*>(us_init + (long)b * N * NU);
        for (int i = l; i < (N - 1) * NU; i += 64) same = same && u[NU + i] == u[i % NU];
        if (surface[b] != 0) {
          const long long* r = reinterpret_cast<const long long*>(node_ref + (long)b * (N + 1) * 6);
          const int c0 = nc == 1 ? 2 : 0;
          for (int i = l; i < (N - 1) * nc; i += 64) same = same && r[(1 + i / nc) * 6 + c0 + i % nc] == r[c0 + i % nc];
        }
      }
      const bool all = __all(same) != 0;
      if (l == 0) d.uni0[b] = all ? 1 : 0;
    }
  }
  if constexpr (SEL) {
    __shared__ int red[INIT_BLOCK / 64], wcnt[INIT_BLOCK / 64];
    const int w = threadIdx.x / 64, l = threadIdx.x % 64;
    for (int c0 = (int)blockIdx.x * INIT_BLOCK; c0 < d.B; c0 += (int)gridDim.x * INIT_BLOCK) {
      int n = 0;  // selected instances before the chunk
      for (int i = threadIdx.x; i < c0; i += INIT_BLOCK) n += active[i] != 0;
      for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
      const int b = c0 + (int)threadIdx.x;
      const bool sel = b < d.B && active[b] != 0;
      const unsigned long long m = __ballot(sel);
      if (l == 0) {
        red[w] = n;
        wcnt[w] = __popcll(m);
      }
      __syncthreads();
      int base = 0, tot = 0;
      for (int j = 0; j < INIT_BLOCK / 64; ++j) {
        base += red[j] + (j < w ? wcnt[j] : 0);
        tot += wcnt[j];
      }
      if (sel) d.alist[base + __popcll(m & ((1ull << l) - 1ull))] = b;
      if (threadIdx.x == 0 && c0 + INIT_BLOCK >= d.B) d.acnt[0] = base + tot;  // the last chunk
      __syncthreads();
    }
  }
  const long nX = (long)d.B * (N + 1) * nx;
  const long nU = (long)d.B * N * NU;
  const long nK = (long)d.B * N * NU * nx;
  const long nT = d.trace ? (long)d.B * d.trace_it * FFDDP_TRACE_W : 0;
  const long perX = (long)(N + 1) * nx, perU = (long)N * NU, perK = perU * nx;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nK || i < nT; i += (long)gridDim.x * blockDim.x) {
    if (i < nT) d.trace[i] = __builtin_nan("");
    if (i >= nK) continue;
    // SEL: the flat index is another instance's in each array
    if (i < nX && (!SEL || active[i / perX] != 0)) d.xs[i] = xs_init[i];
    if (i < nU && (!SEL || active[i / perU] != 0)) {
      d.us[i] = us_init[i];
      d.k[i] = 0.0;
    }
    if (!SEL || active[i / perK] != 0) d.K[i] = 0.0;
    if (i < d.B) {
      if (!SEL) d.alist[i] = (int)i;
      if (i == 0) {
        if (!SEL) d.acnt[0] = d.B;
        d.acnt[1] = 0;
        d.acnt[2] = 0;
        d.acnt[3] = 0;
      }
      InstState s;
      s.preg = C.reg_min;
      s.cost = 0.0;
      s.dg = s.dq = 0.0;
      s.stop = __builtin_nan("");
      s.is_feasible = is_feasible;
      s.was_feasible = 0;
      s.done = (SEL && active[i] == 0) ? 1 : 0;
      s.ok = 0;
      s.iter = 0;
      s.recalc = 1;
      s.accepted = -1;
      s.bw_ok = 0;
      s.n_iters = s.n_trials = s.n_retries = s.n_backward = s.n_calc = s.n_forward = 0;
      s.n_eval1 = s.n_eval2 = 0;
      s.n_neg = s.n_neg_acc = 0;
      s.ffeas = 0.0;
      d.st[i] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// calc + calcDiff of all nodes
// ---------------------------------------------------------------------------
// Per 16-lane group.  The link record is dead once the tangents are in
// registers, so the residual-Jacobian columns reuse its space (a barrier
// separates the last read of lk from the first write of col): 18.3 KB per
// 64-lane block instead of 25 KB, i.e. 8 blocks per CU (the VGPR limit)
// instead of 6 (the LDS limit).
struct NodeGroupShared {
  Primal P;
  union {
    double lk[LK_ALLOC];
    double col[14][NDENSE_MAX];  // residual-Jacobian columns, state directions
  };
  double colu[7][FFDDP_MAX_NC];  // force rows, inner-control directions
};
struct NodeShared {
  NodeGroupShared g[NODE_GPB];
};

// The calc of one node on an 8-lane group (lanes = joints + EE): dynamics,
// costs with their Gauss-Newton weights, gaps; Primal and link record to P /
// lk (the node group's LDS in k_node).
// CW: the scalar cost weights come from the instance's row d.cw[b] (index
// constants FFDDP_CW_* of ffddp.h) instead of C; which terms exist stays C's.
// UL: the torque soft-limit bounds and the w soft limit come from the
// instance's row d.ul[b] (ffddp.h FFDDP_TAU_LIM_W), read where C's were.
// MD: the links' mass, centre of mass and rotational inertia come from the
// instance's row d.md[b] (ffddp.h FFDDP_LINK_W), read where C.rb's were.
// MT: the base placement (joint 0's) and the gravity vector come from the
// instance's row d.mt[b] (ffddp.h FFDDP_MOUNT_W), read where C.rb's were.
template <int NC, bool FF, bool FR, bool CW, bool UL, bool MD, bool MT>
__device__ __forceinline__ void primal_group(const DevConsts& C, const Dev& d, const double* __restrict__ x0,
                                             const double* __restrict__ node_ref, const double* __restrict__ inst_ref,
                                             const uint8_t* __restrict__ surface, int b, int t, Primal* P,
                                             double* lk, const double* __restrict__ xsrc,
                                             const double* __restrict__ usrc, double* __restrict__ stash) {
  const int N = C.N;
  constexpr int nx = FF ? 21 : 14;
  const int li = g8_lane();
  const bool J = li < NQ;
  const int ji = J ? li : 0;
  const bool surf = surface[b] != 0;
  const bool terminal = t == N;
  const int mode = !terminal ? MODE_RUNNING : (FF ? MODE_TERMINAL_U : MODE_TERMINAL_X);
  const double* y = xsrc + (long)t * nx;
  const double* ref = node_ref + ((long)b * (N + 1) + t) * 6;
  const double* xreg = inst_ref + (long)b * 21;
  const double* uin = FF ? (y + 14) : (terminal ? nullptr : usrc + (long)t * NU);
  const double q = y[ji], v = y[7 + ji];
  const double u = (uin != nullptr) ? uin[ji] : 0.0;
  // setCandidate: the accepted line-search trial becomes (xs, us) here, node
  // by node, instead of a whole-trajectory copy on the iteration's chain.
  // Classical: stored at the end of the calc from registers; issued here,
  // the stores sat in front of the vmcnt(0) wait of every later load (the
  // per-lane cost constants in node_primal_g8, the gaps' next state).  FF
  // (at its register limit: the late stores spill) stores here.
  const bool commit = J && xsrc != d.xs + (long)b * (N + 1) * nx;
  double cu = 0.0;
  if (commit) {
    if (FF) {
#pragma unroll
      for (int k = 0; k < 3; ++k) d.xs[((long)b * (N + 1) + t) * nx + 7 * k + li] = y[7 * k + li];
      if (!terminal) d.us[((long)b * N + t) * NU + li] = usrc[(long)t * NU + li];
    } else if (!terminal) {
      cu = usrc[(long)t * NU + li];
    }
  }
  double lam[3];
  const double* cw = CW ? d.cw + (long)b * FFDDP_COST_W : nullptr;
  const double* ul = UL ? d.ul + (long)b * FFDDP_TAU_LIM_W : nullptr;
  const double* md = MD ? d.md + (long)b * FFDDP_LINK_W : nullptr;
  const double* mt = MT ? d.mt + (long)b * FFDDP_MOUNT_W : nullptr;
  // the kernels k_node_rep completes compute the reference-dependent terms through the functions it shares
  constexpr bool STRICT = !FF && !FR && !CW && !UL && !MD && !MT;
  const double pc = node_primal_g8<NC, FR, CW, UL, MD, MT, STRICT>(C, mode, surf, q, v, u, xreg[ji], xreg[7 + ji], xreg[14 + ji], ref, P,
                                                           lk, lam, FR ? d.fref + ((long)b * (N + 1) + t) : nullptr, cw, ul, md,
                                                           mt, stash);
  double* rec = d.rec_buf + ((long)b * (N + 1) + t) * d.rec;
  // node cost (IAM scaling, FF augmentation terms): per-lane shares summed over the group
  double c = FF ? C.dt * pc : (terminal ? pc : C.dt * pc);
  if (FF) {
    double part = 0.0;
    if (J) {
      if (C.w_y > 0.0) {
        double a_ = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double dd = y[7 * k + li] - x0[(long)b * nx + 7 * k + li];
          a_ += C.Wy2[7 * k + li] * dd * dd;
        }
        part += 0.5 * cw_get<CW>(cw, FFDDP_CW_Y, C.w_y) * a_;
      }
      if (!terminal) {
        const double ww = usrc[(long)t * NU + li];
        if (C.w_w > 0.0) part += 0.5 * cw_get<CW>(cw, FFDDP_CW_W, C.w_w) * (ww * ww);
        if (C.w_ws > 0.0) {
          const double ov = fabs(ww) - (UL ? ul[4 * li + 2] : C.ws_lim[li]);
          const double o = ov > 0.0 ? ov : 0.0;
          part += cw_get<CW>(cw, FFDDP_CW_W_SOFT_LIMITS, C.w_ws) * (0.5 * (o * o));
        }
      }
    }
    c += g8_sum(part);
  }
  if (li == 0) {
    rec[rec_off_cost(nx)] = c;
#pragma unroll
    for (int r = 0; r < 3; ++r) rec[rec_off_lam(nx) + r] = (mode == MODE_TERMINAL_X) ? 0.0 : lam[r];
  }
  // gaps fs[t+1] = xnext_t - xs[t+1] ; fs[0] = x0 - xs[0]  (zero once feasible)
  const bool feas = d.st[b].is_feasible != 0;
  if (J) {
    if (!terminal) {
      double* f = d.fs + ((long)b * (N + 1) + t + 1) * nx;
      const double* yn = xsrc + (long)(t + 1) * nx;
      const double dt = C.dt;
      const double a = P->a[li];  // this lane's own store
      const double qn = (mode == MODE_TERMINAL_X) ? q : q + (v * dt + a * dt * dt);
      const double vn = (mode == MODE_TERMINAL_X) ? v : v + a * dt;
      f[li] = feas ? 0.0 : qn - yn[li];
      f[7 + li] = feas ? 0.0 : vn - yn[7 + li];
      if (stash != nullptr) {
        stash[REP_XN + li] = qn;
        stash[REP_XN + 7 + li] = vn;
      }
      if (FF) f[14 + li] = feas ? 0.0 : (C.alpha * y[14 + li] + C.beta * usrc[(long)t * NU + li]) - yn[14 + li];
    }
    if (t == 0) {
      double* f = d.fs + (long)b * (N + 1) * nx;
#pragma unroll
      for (int k = 0; k < (FF ? 3 : 2); ++k) f[7 * k + li] = feas ? 0.0 : x0[(long)b * nx + 7 * k + li] - y[7 * k + li];
    }
  }
  if (!FF && commit) {
    double* xr = d.xs + ((long)b * (N + 1) + t) * nx;
    xr[li] = q;
    xr[7 + li] = v;
    if (!terminal) d.us[((long)b * N + t) * NU + li] = cu;
  }
}

// a^T H b over the contact-force block of the Gauss-Newton Hessian: diagonal
// Dd plus (nc = 3) the friction cone's off-diagonal couplings Do
template <int NC>
__device__ __forceinline__ double fquad(const double* a, const double* Dd, const double* Do, const double* b) {
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < NC; ++r) acc += a[r] * Dd[r] * b[r];
  if (NC == 3)
    acc += Do[0] * (a[1] * b[0] + a[0] * b[1]) + Do[1] * (a[2] * b[0] + a[0] * b[2]) +
           Do[2] * (a[2] * b[1] + a[1] * b[2]);
  return acc;
}

// calc + calcDiff tangents + Gauss-Newton assembly: 16-lane group per node.
// The group's lanes 0..7 first run the node's calc (primal_group) into the
// group's LDS, so the Primal / link records (~4 KB per node) never round-trip
// through HBM: a separate calc kernel writing them and this one reading them
// back was 129 + 366 us per launch at B=4096; fused, 255 us.
// FR: the fn_track cost reads d.fref[b][t] instead of C.fn_ref (a solve with
// a force_ref); FR = false is the kernel as it was.
// CW: the scalar cost weights are those of the instance's row d.cw[b] (a solve
// with cost_w), each loaded where its term is evaluated; CW = false is the
// kernel as it was.
// UL: the torque soft-limit bounds and the w soft limit are those of the
// instance's row d.ul[b] (a solve with tau_lim), each read where C's was;
// UL = false is the kernel as it was.
// MD: the calc's link inertial parameters are those of the instance's row
// d.md[b] (a solve with link_rows), read where C.rb's were; the tangents read
// only what the calc wrote.  MD = false is the kernel as it was.
// MT: the calc's base placement and gravity vector are those of the instance's
// row d.mt[b] (a solve with mount_rows), read where C.rb's were; the state
// tangent's one read of the gravity vector takes the row's too.  MT = false is
// the kernel as it was.
template <int NC, bool FF, bool FR = false, bool CW = false, bool UL = false, bool MD = false, bool MT = false>
__global__ __launch_bounds__(NODE_BLOCK) __attribute__((amdgpu_waves_per_eu(NODE_WAVES))) void k_node(const DevConsts* __restrict__ Cg, Dev d,
                                                      const double* __restrict__ x0,
                                                      const double* __restrict__ node_ref,
                                                      const double* __restrict__ inst_ref,
                                                      const uint8_t* __restrict__ surface, int force_all, int cur,
                                                      int rep0) {
  const DevConsts& C = *Cg;
  const int N = C.N;
  constexpr int nx = FF ? 21 : 14;
  constexpr int nc = NC;
  __shared__ NodeShared S;
  const int grp = threadIdx.x / NODE_GROUP, lane = threadIdx.x % NODE_GROUP;
  const int n_work = force_all ? d.B : d.acnt[cur];  // instances with nodes to evaluate
  const long blk = xcd_block(blockIdx.x, ((long)n_work * (N + 1) + NODE_GPB - 1) / NODE_GPB);
  const long gnode = blk * NODE_GPB + grp;
  const int slot = (int)(gnode / (N + 1)), t = (int)(gnode % (N + 1));
  int b = slot;
  bool active = slot < d.B;
  if (active && !force_all) {
    const ActiveList al = active_list(d, cur);
    active = slot < al.n;
    b = active ? al.list[slot] : 0;
    if (active) active = (d.st[b].done == 0) && (d.st[b].recalc != 0);
  }
  const bool terminal = t == N;
  // rep0 (the first node stage of a solve): of an instance that starts from
  // one repeated (x, u) point, node 0 and the terminal node run; node 0 also
  // stashes what k_node_rep, launched next, builds nodes 1..N-1 from.  The
  // plain classical kernels only: the others have no such branch.
  bool rep_src = false;
  if constexpr (!FF && !FR && !CW && !UL && !MD && !MT) {
    if (rep0 && active && !terminal && d.uni0[b] != 0) {
      if (t == 0)
        rep_src = true;
      else
        active = false;
    }
  }
  const bool surf = active ? surface[b] != 0 : false;
  constexpr bool ff = FF;
  const int mode = !terminal ? MODE_RUNNING : (ff ? MODE_TERMINAL_U : MODE_TERMINAL_X);
  // current iterate: the trial the last line search accepted (not yet copied
  // into xs / us: primal_group does that for its node), else xs / us
  const long perX = (long)(N + 1) * nx, perU = (long)N * NU;
  const int acc = active ? d.st[b].accepted : -1;
  const double* xsrc = acc >= 0 ? d.xs_try + ((long)b * NTRIALS + acc) * perX : d.xs + (long)b * perX;
  const double* usrc = acc >= 0 ? d.us_try + ((long)b * NTRIALS + acc) * perU : d.us + (long)b * perU;
  const double* y = xsrc + (long)t * nx;
  const double* ref = node_ref + ((long)b * (N + 1) + t) * 6;
  NodeGroupShared& G = S.g[grp];
  Primal& P = G.P;
  if (active && lane < G8) primal_group<NC, FF, FR, CW, UL, MD, MT>(C, d, x0, node_ref, inst_ref, surface, b, t, &P, G.lk, xsrc, usrc,
                                                                    rep_src ? d.rep + (long)b * REP_W : nullptr);
  __syncthreads();
  const bool need_u = mode != MODE_TERMINAL_X;
  // control directions first, their results stored at once (neither touches
  // lk), so they are not live across the state tangent: no scratch spill at
  // 2 waves/SIMD
  if (active && lane < 7 && need_u) {
    double dau[NQ], dlamu[3];
    node_tangent_control<NC>(C, surf, P, lane, dau, dlamu);
    double* rec = d.rec_buf + ((long)b * (N + 1) + t) * d.rec;
    for (int i = 0; i < NQ; ++i) rec[rec_off_A() + (14 + lane) * NQ + i] = dau[i];
    for (int r = 0; r < nc; ++r) G.colu[lane][r] = (surf ? dlamu[r] : 0.0);
  }
  double da[NQ], dlam[3], col[NDENSE_MAX], r1[NQ], dh[3];
  if constexpr (MT) {
    if (active && lane < 14)
      node_tangent_state_links<NC, true>(C, mode, surf, G.lk, P, lane, r1, dh, col, d.mt + (long)b * FFDDP_MOUNT_W + 12);
  } else {
    if (active && lane < 14) node_tangent_state_links<NC>(C, mode, surf, G.lk, P, lane, r1, dh, col);
  }
  __syncthreads();  // every lane's reads of lk are done before col overwrites it
  // the column's rows 0..11 go to LDS before the contact solves (which read
  // only P), so they are not live across them: no scratch spill at 2 waves/SIMD
  if (active && lane < 14) {
    for (int r = 0; r < 12; ++r) G.col[lane][r] = col[r];
    node_tangent_state_contact<NC>(mode, surf, P, r1, dh, da, dlam, col);
    for (int r = 12; r < 12 + nc; ++r) G.col[lane][r] = col[r];
  }
  __syncthreads();
  if (active) {
    double* rec = d.rec_buf + ((long)b * (N + 1) + t) * d.rec;
    const int nd = 12 + nc;
    const bool scale = mode != MODE_TERMINAL_X;
    const double sc = scale ? C.dt : 1.0;
    const double* D = P.D;
    const double* g = P.g;
    // FF's y-cost weights of this lane's components, loaded once up front:
    // at each use the scalar w_y and the lane's Wy2 entry were loaded again
    // and waited for with vmcnt(0), i.e. behind every record store in flight
    // (FF k_node 109 -> 104 us at B = 1024; the compiler contracts some of
    // the products differently, so FF solves move by <= 2e-9, classical
    // ones are bit-identical)
    double wy = 0.0, wy2j = 0.0, wy2u = 0.0;
    if (ff) {
      wy = C.w_y;
      wy2j = C.Wy2[lane < 14 ? lane : 0];
      wy2u = C.Wy2[14 + (lane < 7 ? lane : 0)];
      if constexpr (CW) {
        // a term the handle does not build keeps C's (zero) weight: its row entry is not read
        if (C.w_y > 0.0) wy = d.cw[(long)b * FFDDP_COST_W + FFDDP_CW_Y];
        asm volatile("" : "+v"(wy2j), "+v"(wy2u));
      } else {
        asm volatile("" : "+s"(wy), "+v"(wy2j), "+v"(wy2u));
      }
    }
    if (lane < 14) {
      const int j = lane;
      // dynamics Jacobian columns
      if (need_u)
        for (int i = 0; i < NQ; ++i) rec[rec_off_A() + j * NQ + i] = da[i];
      // Lxx_in column j (rows 0..13)
      double* Lxx = rec + rec_off_Lxx(nx);
      for (int i = 0; i < 14; ++i) {
        double acc = 0.0;
        for (int r = 0; r < 12; ++r) acc += G.col[i][r] * D[r] * col[r];
        acc += fquad<NC>(&G.col[i][12], D + 12, P.Dfo, col + 12);
        if (i == j) acc += P.Dx[j];
        acc *= sc;
        if (ff && i == j) acc += wy * wy2j;
        Lxx[i * nx + j] = acc;
      }
      // Lx_in[j]
      double lx = 0.0;
      if constexpr (!FF && !FR && !CW && !UL && !MD && !MT) {
        lx = node_lx_entry<12 + NC>(col, g, P.gx[j], sc);  // shared with k_node_rep
      } else {
        for (int r = 0; r < nd; ++r) lx += col[r] * g[r];
        lx = (lx + P.gx[j]) * sc;
      }
      if (ff) lx += wy * wy2j * (y[j] - x0[(long)b * nx + j]);
      if (rep_src) {
        double* stash = d.rep + (long)b * REP_W;
        for (int r = 0; r < nd; ++r) stash[REP_COL + j * NDENSE_MAX + r] = col[r];
        stash[REP_GX + j] = P.gx[j];
      }
      rec[rec_off_Lx(nx) + j] = lx;
      // Lxu_in row j (force rows only): classical -> Lxu row j; FF -> Lxx_aug[14+k][j]
      if (need_u) {
        for (int kk = 0; kk < NU; ++kk) {
          double acc = 0.0;
          acc = fquad<NC>(col + 12, D + 12, P.Dfo, G.colu[kk]);
          acc *= sc;
          if (ff)
            Lxx[(14 + kk) * nx + j] = acc;
          else
            rec[rec_off_Lxu(nx) + j * NU + kk] = acc;
        }
      }
    }
    if (lane < 7 && need_u) {
      const int kk = lane;
      // Luu_in column kk
      double luu[7];
      for (int m = 0; m < NU; ++m) {
        double acc = 0.0;
        acc = fquad<NC>(G.colu[m], D + 12, P.Dfo, G.colu[kk]);
        if (m == kk) acc += P.Du[kk];
        luu[m] = acc * sc;
      }
      double lu = 0.0;
      for (int r = 0; r < nc; ++r) lu += G.colu[kk][r] * g[12 + r];
      lu = (lu + P.gu[kk]) * sc;
      if (!ff) {
        for (int m = 0; m < NU; ++m) rec[rec_off_Luu(nx) + m * NU + kk] = luu[m];
        rec[rec_off_Lu(nx) + kk] = lu;
      } else {
        double* Lxx = rec + rec_off_Lxx(nx);
        // Lxx_aug column 14+kk: rows 0..13 = Lxu_in[:, kk], rows 14..20 = Luu_in[:, kk] + w_y Wy2
        for (int i = 0; i < 14; ++i) {
          double acc = 0.0;
          acc = fquad<NC>(&G.col[i][12], D + 12, P.Dfo, G.colu[kk]);
          Lxx[i * nx + 14 + kk] = acc * sc;
        }
        for (int m = 0; m < NU; ++m)
          Lxx[(14 + m) * nx + 14 + kk] = luu[m] + (m == kk ? wy * wy2u : 0.0);
        rec[rec_off_Lx(nx) + 14 + kk] = lu + wy * wy2u * (y[14 + kk] - x0[(long)b * nx + 14 + kk]);
        // augmented control terms: Lu = w_w w + w_s g_soft ; Luu = diag ; Lxu = 0
        double wk = 0.0;
        if (!terminal) wk = usrc[(long)t * NU + kk];
        double wsl;
        if constexpr (UL) {
          // a term the handle does not build never reads its entry
          wsl = C.w_ws > 0.0 ? d.ul[(long)b * FFDDP_TAU_LIM_W + 4 * kk + 2] : C.ws_lim[kk];
        } else {
          wsl = C.ws_lim[kk];
        }
        const double ov = fabs(wk) - wsl;
        const bool act = ov > 0.0;
        const double gs = act ? ov * (wk > 0.0 ? 1.0 : (wk < 0.0 ? -1.0 : 0.0)) : 0.0;
        if constexpr (CW) {
          const double* cwb = d.cw + (long)b * FFDDP_COST_W;
          const double w_w = C.w_w > 0.0 ? cwb[FFDDP_CW_W] : C.w_w;
          const double w_ws = C.w_ws > 0.0 ? cwb[FFDDP_CW_W_SOFT_LIMITS] : C.w_ws;
          rec[rec_off_Lu(nx) + kk] = w_w * wk + w_ws * gs;
          for (int m = 0; m < NU; ++m)
            rec[rec_off_Luu(nx) + m * NU + kk] = (m == kk) ? (w_w + w_ws * (act ? 1.0 : 0.0)) : 0.0;
        } else {
          rec[rec_off_Lu(nx) + kk] = C.w_w * wk + C.w_ws * gs;
          for (int m = 0; m < NU; ++m)
            rec[rec_off_Luu(nx) + m * NU + kk] = (m == kk) ? (C.w_w + C.w_ws * (act ? 1.0 : 0.0)) : 0.0;
        }
        for (int i = 0; i < nx; ++i) rec[rec_off_Lxu(nx) + i * NU + kk] = 0.0;
      }
    }
    if (!need_u && lane < 7) {
      // classical terminal: no control blocks (zero them for the calcDiff export)
      for (int i = 0; i < NQ; ++i) rec[rec_off_A() + (14 + lane) * NQ + i] = 0.0;
    }
  }
}


// Nodes 1..N-1 of the instances that start from one repeated (x, u) point
// (d.uni0, k_init), once per solve after the first k_node, which ran their
// nodes 0 and N only.  Such a node's calc is node 0's up to the terms the node
// references enter: the EE residuals' gradients (so Lx) and the cost.  16-lane
// group per node: the record blocks that do not depend on the references (A,
// Lxx, Lxu, Luu, Lu, lambda) are copied from node 0's record with 16-byte
// accesses, Lx and the cost recomputed from node 0's stash (d.rep) through the
// functions k_node computes them with, and the gap written from node 0's next
// state.  (The first node stage has no accepted trial to commit into xs / us.)
template <int NC>
__global__ __launch_bounds__(NODE_BLOCK) void k_node_rep(const DevConsts* __restrict__ Cg, Dev d,
                                                         const double* __restrict__ node_ref,
                                                         const uint8_t* __restrict__ surface) {
  const DevConsts& C = *Cg;
  const int N = C.N;
  constexpr int nx = 14, nd = 12 + NC;
  const int grp = threadIdx.x / NODE_GROUP, lane = threadIdx.x % NODE_GROUP;
  const long gnode = (long)blockIdx.x * NODE_GPB + grp;
  const int b = (int)(gnode / (N - 1)), t = 1 + (int)(gnode % (N - 1));
  if (b >= d.B || d.uni0[b] == 0) return;
  const InstState* st = d.st + b;
  if (st->done != 0) return;
  const double* src = d.rec_buf + (long)b * (N + 1) * d.rec;
  double* rec = d.rec_buf + ((long)b * (N + 1) + t) * d.rec;
  const double* stash = d.rep + (long)b * REP_W;
  // the reference-independent blocks: words [0, Lx) and lambda
  {
    const double2* s2 = reinterpret_cast<const double2*>(src);
    double2* r2 = reinterpret_cast<double2*>(rec);
    // classical layout (rec_off_* of ffddp_node.hpp): Lx starts at word 490 and lambda at 512, both even
    constexpr int o_lx = 147 + nx * nx + nx * 7 + 49, o_lam = o_lx + nx + 7 + 1;
    static_assert(o_lx % 2 == 0 && o_lam % 2 == 0, "16-byte copy ranges");
    const int n2 = rec_off_Lx(nx) / 2;
#pragma unroll 4
    for (int i = lane; i < n2; i += NODE_GROUP) r2[i] = s2[i];
    if (lane < 2) r2[rec_off_lam(nx) / 2 + lane] = s2[rec_off_lam(nx) / 2 + lane];
    if (lane < NU) rec[rec_off_Lu(nx) + lane] = src[rec_off_Lu(nx) + lane];
  }
  // the residual terms of this node's references
  double rr[3], wee[3], pee[3], vp[3], lm[3], Dd[NDENSE_MAX], gd[NDENSE_MAX], Ho[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rr[k] = stash[REP_RR + k];
    wee[k] = stash[REP_WEE + k];
    pee[k] = stash[REP_PEE + k];
    vp[k] = stash[REP_VP + k];
    lm[k] = stash[REP_LM + k];
  }
  const double* ref = node_ref + ((long)b * (N + 1) + t) * 6;
  const double cee = ee_contact_costs<NC, false, false>(C, surface[b] != 0, rr, wee, pee, vp, lm, ref, nullptr, nullptr, Dd,
                                                        gd, Ho);
  if (lane == 0) rec[rec_off_cost(nx)] = C.dt * (stash[REP_CJ] + cee);
  if (lane < 14) {
    double col[nd];
#pragma unroll
    for (int r = 0; r < nd; ++r) col[r] = stash[REP_COL + lane * NDENSE_MAX + r];
    rec[rec_off_Lx(nx) + lane] = node_lx_entry<nd>(col, gd, stash[REP_GX + lane], C.dt);
  }
  // the gap to the next node's state: node 0's next state against xs[t + 1]
  if (lane < 14) {
    const bool feas = st->is_feasible != 0;
    const double* yn = d.xs + ((long)b * (N + 1) + t + 1) * nx;
    d.fs[((long)b * (N + 1) + t + 1) * nx + lane] = feas ? 0.0 : stash[REP_XN + lane] - yn[lane];
  }
}

__device__ __forceinline__ bool bad(double v) { return isnan(v) || isinf(v) || v >= 1e30; }


// sum over the 64 lanes, wave-uniform result: DPP butterflies inside each
// 16-lane row (quad swaps, half-row and row mirrors), then the four row sums
// by readlane -- no ds_bpermute round trips on the backward pass's chain
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp64<0x141>(v);  // row_half_mirror
  v += dpp64<0x140>(v);  // row_mirror
  const double r0 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 0),
                                     __builtin_amdgcn_readlane(__double2loint(v), 0));
  const double r1 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16),
                                     __builtin_amdgcn_readlane(__double2loint(v), 16));
  const double r2 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 32),
                                     __builtin_amdgcn_readlane(__double2loint(v), 32));
  const double r3 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 48),
                                     __builtin_amdgcn_readlane(__double2loint(v), 48));
  return (r0 + r1) + (r2 + r3);
}

// max over the 64 lanes (values >= 0), wave-uniform result
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp64<0xB1>(v));
  v = fmax(v, dpp64<0x4E>(v));
  v = fmax(v, dpp64<0x141>(v));
  v = fmax(v, dpp64<0x140>(v));
  double m = v;
#pragma unroll
  for (int r = 16; r < 64; r += 16)
    m = fmax(m, __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), r),
                                 __builtin_amdgcn_readlane(__double2loint(v), r)));
  return fmax(m, __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 0),
                                  __builtin_amdgcn_readlane(__double2loint(v), 0)));
}

// ---------------------------------------------------------------------------
// backward pass, one wavefront per instance (k_backward_w)
//
// The Riccati recursion of one instance is a chain of 30 small dense steps;
// what bounds it is latency, not flops.  One wave (64 lanes) owns one
// instance and spreads each step's algebra over all lanes:
//   [Fx Fu] = I~ + D A^        (Euler structure: I~ sparse, D = [dt^2 I; dt I],
//                               A^ = node acceleration Jacobian, 7 x (nx+nu))
//   Q = L + I~'V I~ + M A^ + (M A^)',   M = I~'(V D) + 1/2 A^'(D'V D)
// so the full Q (x and u blocks) is one symmetric rank-7 update plus sparse
// terms; every lane computes a few lower-triangle entries.  The node record
// for t-1 is prefetched into registers while node t is processed (LDS-only
// fences between phases, so the prefetch stays in flight), and with no
// per-lane arrays beyond that the kernel fits several waves per SIMD, so
// instances hide each other's latency.  Gains (LLT / BoxQP on 7x7) stay on
// lane 0.
// ---------------------------------------------------------------------------
constexpr int rec_words(int nx) { return ((147 + nx * nx + nx * 7 + 49 + nx + 7 + 1) + 3 + 15) & ~15; }

__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Y (D' V D) lives in phases A-B, the factors L (packed masked Cholesky
// factor, reciprocal diagonal) and L1 (k_backward_w2: wave 1's factor of the
// full set) in D-E; M in B-C, K in D/E-G (k_backward_w2: G runs beside the
// next node's A, still before its B).  U: one slot each for Y / {L, L1} and
// M / K.  It saves FF's backward 1.5 KB of LDS (8 blocks per CU, with the
// rest of the diet), but the aliasing costs the classical pass at B = 4096
// (522k-526k vs 546k-548k solves/s without it), so only FF takes it.
template <bool U, int NM, int NK> struct BwSlots {
  double Y[NU * NU], L[28], L1[28], M[NM], K[NK];
};
template <int NM, int NK> struct BwSlots<true, NM, NK> {
  union {
    double Y[NU * NU];
    struct {
      double L[28];
      double L1[28];
    };
  };
  union {
    double M[NM];
    double K[NK];
  };
};

template <bool FF> struct BwW {
  static constexpr int NX = FF ? 21 : 14;
  static constexpr int ND = NX + NU;
  static constexpr int REC = rec_words(NX);
  // Q's distinct blocks, contiguous so that phase C stores an entry through
  // one flat index: Qxx (full, mirrored) | Qxu (row-major, NX x 7) | H =
  // Quu + preg I (full, mirrored); Qux and the Quu copy of the full ND x ND
  // matrix are never read (round 5: FF 25.7 -> 19.8 KB per wave, 8 blocks
  // per CU instead of 6)
  static constexpr int QXU = NX * NX, QH = NX * NX + NX * NU, NQQ = NX * NX + NX * NU + NU * NU;
  double R[(REC + 63) / 64 * 64];  // staged node record (A | Lxx | Lxu | Luu | Lx | Lu | cost | lam), padded
  double V[NX * NX];  // V_xx' on entry to a node, V_xx on exit
  double QQ[NQQ];
  double W[NX * NU];  // V D
  // Y lives in phases A-B, the factors in D-E: one slot
  BwSlots<FF && BW_DIET_UNION, ND * NU, NU * NX> sl;  // Y, L, L1, M, K
  int spec;           // k_backward_w2: wave 1's K (and LLT k) from L1 are valid
  double Vx[NX], Qv[ND], kk[NU], z[NU];
  // staged per node by every lane without lane guards: lane l writes slot
  // l mod n, which the lanes load from the matching index (duplicate writers
  // store the same value)
  double fs[BW_DIET_SLOTS ? NX : 64], kp[BW_DIET_SLOTS ? NU : 64], uu[BW_DIET_SLOTS ? NU : 64];
  double ulb[BW_DIET_SLOTS ? NU : 64], uub[BW_DIET_SLOTS ? NU : 64];
  double fsb[2][BW_DIET_SLOTS ? NX : 64];  // k_backward_w2: node t's gap in slot t & 1 (staged before node t+1's phase G reads its own)
  int flag;
  int badw[2];  // k_backward_w2: per-wave NaN flags of phases F / G
#ifdef BW_PAD_CL
  double pad[FF ? 1 : BW_PAD_CL];  // development: classical LDS footprint back to the round-4 size
#endif
};

// Phase C's entry for flat index e of a pass over the lower triangle (NQE
// entries, the last pass starting at `last`): a lane past the last entry
// takes an entry of that same pass, so its duplicate store is computed by the
// same instruction from the same operands as the owner's (identical bits in
// any unrolling or contraction), with no address select and no spare slot
__device__ __forceinline__ int spare_entry(int e, int nqe, int last) {
  return e < nqe ? e : last + (e - last) % (nqe - last);
}
// phase C's packed entry (r >= c): r, c and the two flat BwW::QQ indices its
// value is stored at (Qxx mirrored; Qux stored once as Qxu[c][r - NX]; Quu
// mirrored into H)
template <int NX> __device__ __forceinline__ unsigned q_entry(int r, int c) {
  // fields: r, c 5 bits each, i1, i2 11 bits each
  static_assert(NX + NU <= 32 && (NX + NU) * (NX + NU) <= 2048, "q_entry packing");
  unsigned i1, i2;
  if (r < NX) {
    i1 = r * NX + c;
    i2 = c * NX + r;
  } else if (c < NX) {
    i1 = i2 = NX * NX + c * NU + (r - NX);
  } else {
    i1 = NX * NX + NX * NU + (r - NX) * NU + (c - NX);
    i2 = NX * NX + NX * NU + (c - NX) * NU + (r - NX);
  }
  return ((unsigned)r << 27) | ((unsigned)c << 22) | (i1 << 11) | i2;
}

// nonzeros of column c of I~ (the Euler identity part of [Fx Fu]):
// returns the count and fills (row, coef) pairs.
template <bool FF> __device__ __forceinline__ int itilde(int c, double dt, double alpha, double beta, int (&row)[2],
                                                         double (&cf)[2]) {
  if (c < 7) {
    row[0] = c;
    cf[0] = 1.0;
    return 1;
  }
  if (c < 14) {
    row[0] = c;
    cf[0] = 1.0;
    row[1] = c - 7;
    cf[1] = dt;
    return 2;
  }
  if (!FF) return 0;  // classical u columns: Fu = D A_u only
  if (c < 21) {
    row[0] = c;
    cf[0] = alpha;
    return 1;
  }
  row[0] = c - 7;
  cf[0] = beta;
  return 1;
}

// branch-free form of itilde: two (row, coef) terms, coef 0 where absent (row kept in range)
template <bool FF>
__device__ __forceinline__ void itilde2(int c, double dt, double alpha, double beta, int& r0, double& a0, int& r1,
                                        double& a1) {
  const bool lo = c < 14;
  a0 = lo ? 1.0 : (FF ? (c < 21 ? alpha : beta) : 0.0);
  r0 = lo ? c : (FF ? (c < 21 ? c : c - 7) : 0);
  const bool vel = c >= 7 && c < 14;
  a1 = vel ? dt : 0.0;
  r1 = vel ? c - 7 : 0;
}

// A^[m][c] = d a_m / d dir_c (record rows 0..20; FF w-columns 21..27 are zero)
template <bool FF> __device__ __forceinline__ double ahat(const double* Ar, int m, int c) {
  return (FF && c >= 21) ? 0.0 : Ar[c * 7 + m];
}

// lower-triangle index e -> (r, c), r >= c
__device__ __forceinline__ void tri_rc(int e, int& r, int& c) {
  int rr = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while ((rr + 1) * (rr + 2) / 2 <= e) ++rr;
  while (rr * (rr + 1) / 2 > e) --rr;
  r = rr;
  c = e - rr * (rr + 1) / 2;
}

// ---- 7x7 algebra with one row / variable per lane (lanes 0..6), uniform control flow ----
// lane k's value to every lane of its 16-lane row (DPP row_newbcast: one
// v_mov_b64_dpp, no SGPR round trip).  The 7x7 algebra below lives on lanes
// 0..6 of row 0; the other rows compute on their own (unused) lanes.
// k is a constant after unrolling: the switch folds away
__device__ __forceinline__ double rowb(double v, int k) {
  switch (k) {
    case 0: return g8_rowb<0>(v);
    case 1: return g8_rowb<1>(v);
    case 2: return g8_rowb<2>(v);
    case 3: return g8_rowb<3>(v);
    case 4: return g8_rowb<4>(v);
    case 5: return g8_rowb<5>(v);
    default: return g8_rowb<6>(v);
  }
}

// In-place LLT of the SPD matrix whose row i is held by lane i: on exit
// a[j] (j < i) = L_ij and a[i] = 1 / L_ii.  Returns false (uniformly) if a
// pivot is not positive.  The pivot test is one ballot after the
// factorisation, not a branch per pivot: past a bad pivot the values are
// garbage (NaN) but unused, and a good factorisation takes the same
// operations either way.  Every product-sum is an explicit fma (and the
// reciprocal square root's Newton steps too), so the larger basic block
// cannot change how the compiler contracts them: every backward variant and
// BoxQP's refactorisations round alike (wave 1's speculative factor in
// k_backward_w2 must equal BoxQP's for an empty clamped set, bit for bit).
__device__ __forceinline__ bool chol_rows(double (&a)[NU], int lane) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    double d = a[k];
#pragma unroll
    for (int m = 0; m < k; ++m) d = __builtin_fma(-a[m], a[m], d);
    const double dk = rowb(d, k);
    bad = bad || !(dk > 0.0);  // dk is uniform across the row
    double il = __builtin_amdgcn_rsq(dk);
    const double h = 0.5 * dk;
    il = il * __builtin_fma(-(h * il), il, 1.5);
    il = il * __builtin_fma(-(h * il), il, 1.5);
    double s = a[k];
#pragma unroll
    for (int m = 0; m < k; ++m) s = __builtin_fma(-a[m], rowb(a[m], k), s);
    a[k] = (lane == k) ? il : ((lane > k) ? s * il : a[k]);
  }
  return !(__ballot(bad) & 1ull);  // lane 0 holds row 0's pivots
}

// solve L L^T x = r with L held as rows (chol_rows layout); r / result per lane
__device__ __forceinline__ double chol_solve_rows(const double (&Lr)[NU], double r, int lane) {
  double y[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    double s = r;
#pragma unroll
    for (int m = 0; m < k; ++m) s -= Lr[m] * y[m];
    y[k] = rowb(s * Lr[k], k);
  }
  double x[NU];
#pragma unroll
  for (int k = NU - 1; k >= 0; --k) {
    double s = y[k];
#pragma unroll
    for (int m = k + 1; m < NU; ++m) s -= rowb(Lr[k], m) * x[m];
    x[k] = s * rowb(Lr[k], k);
  }
  double out = 0.0;
#pragma unroll
  for (int k = 0; k < NU; ++k) out = (lane == k) ? x[k] : out;
  return out;
}

// phase E's factor without the LDS round trip: the lower triangle of the
// chol_rows factor (rows on lanes 0..6) in tri layout in every lane of DPP
// row 0 (lanes 0..15: the classical pass's K columns and k), by row_newbcast.
// chol_solve then reads the same values it would read from the LDS copy.
constexpr bool e_from_regs(int nx) { return nx + 1 <= 16; }
__device__ __forceinline__ void rows_to_tri(const double (&Lr)[NU], double (&Lt)[NU * (NU + 1) / 2]) {
#pragma unroll
  for (int i = 0; i < NU; ++i)
#pragma unroll
    for (int k = 0; k <= i; ++k) Lt[tri(i, k)] = rowb(Lr[k], i);
}

// a branch on lane 0's value of a condition (lane 0 holds the 8-lane sums /
// maxima like every lane of its group): a ballot bit, no readlane round trip
__device__ __forceinline__ bool lane0(bool c) { return (__ballot(c) & 1ull) != 0; }
// max over lanes 0..7 of |v| below th, as one ballot instead of max8's three
// DPP steps: the same decision (v_max_f64 skips a NaN operand and a NaN lane
// fails `>= th` alike; lane 7 holds 0 in every BoxQP vector, so the maximum
// is never taken over NaN lanes only)
__device__ __forceinline__ bool all8_below(double av, double th) { return (__ballot(av >= th) & 0x7Full) == 0; }

// crocoddyl::BoxQP::solve with variable i on lane i: projected Newton on the
// free set, refactored when it changes, Armijo line search over the same
// alphas.  hrow = row i of H; x in = warm start, out = solution; Lr = rows of
// the masked factor of the final free set; clmask = final clamped set.  The
// scalar products (objective values, directional derivative) and the step
// norm are lane-local terms summed / maxed by DPP over the 8 lanes; only the
// vectors a mat-vec needs (x, the trial point) are broadcast.
__device__ __forceinline__ bool boxqp_lanes(const DevConsts& C, const double (&hrow)[NU], double q, double lb,
                                            double ub, double& x, double (&Lr)[NU], int& clmask, int lane,
                                            unsigned long long* pq = nullptr) {
  (void)pq;  // FFDDP_PHASE_PROF builds: the split of this QP's time (BQ_*)
  BQ_T0();
  x = fmax(fmin(x, ub), lb);
  bool have = false, cl = false;
  double xsf = 0.0;
#pragma unroll 1
  for (int it = 0; it < C.qp_maxiter; ++it) {
    double xb[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) xb[j] = rowb(x, j);
    double hx = 0.0;
#pragma unroll
    for (int j = 0; j < NU; ++j) hx += hrow[j] * xb[j];
    const double g = q + hx;
    // the objective at x: needed only if this iteration steps, but computed
    // here it overlaps the factorisation and solve instead of following them
    // (a cross-lane sum cannot move across the convergence branch by itself)
    const double fold = g8_sum(0.5 * x * hx + q * x);
    const bool c = (x == lb && g > 0.0) || (x == ub && g < 0.0);
    const bool changed = !have || ((__ballot(c != cl) & 0x7Full) != 0);
    cl = c;
    BQ_CNT(6);
    BQ_ACC(0);
    if (changed) {
      const int m = (int)(__ballot(cl) & 0x7Full);
#pragma unroll
      for (int j = 0; j < NU; ++j) {
        const bool cj = (m >> j) & 1;
        Lr[j] = (!cl && !cj) ? hrow[j] + (lane == j ? C.qp_reg : 0.0) : (lane == j ? 1.0 : 0.0);
      }
      if (!chol_rows(Lr, lane)) return false;
      BQ_CNT(7);
      BQ_ACC(1);
      have = true;
      double r = -q;
#pragma unroll
      for (int j = 0; j < NU; ++j)
        if ((m >> j) & 1) r -= hrow[j] * xb[j];
      xsf = chol_solve_rows(Lr, cl ? 0.0 : r, lane);
      clmask = m;
      BQ_ACC(2);
    }
    const double dx = cl ? 0.0 : xsf - x;
    if (all8_below(fabs(dx), C.qp_th_grad)) {
      BQ_ACC(3);
      break;
    }
    BQ_ACC(3);
    bool moved = false;
#pragma unroll 1
    for (int ia = 0; ia < NTRIALS; ++ia) {
      const double al = C.alphas[ia];
      const double xn = fmax(fmin(x + al * dx, ub), lb);
      double hxn = 0.0;
#pragma unroll
      for (int j = 0; j < NU; ++j) hxn += hrow[j] * rowb(xn, j);
      const double fnew = g8_sum(0.5 * xn * hxn + q * xn);
      const double gd = g8_sum(g * (x - xn));
      if (lane0(fold - fnew > C.qp_th_acceptstep * gd)) {
        x = xn;
        moved = true;
        break;
      }
    }
    // No step length accepted: x is unchanged, so every remaining iteration
    // recomputes the same gradient, clamped set and direction and rejects the
    // same trials (BoxQP::solve runs them to maxiter).  Stopping here returns
    // exactly what the remaining iterations would.  On the random-x0 workload
    // ~1 QP in 3700 stalls this way (numpy oracle, tests/golden/
    // make_boxqp_stagnation.py), and its ~90 repeated iterations (10 trials
    // each) set the backward launch's tail.
    BQ_ACC(4);
    if (!moved) break;
    // The next iteration's convergence test without its mat-vec: with no
    // control clamped now and none at a bound after the step, that
    // iteration's clamped set is empty again (no refactor, same xsf) and its
    // step is dx = xsf - x, so when that is below th_grad it stops right
    // there with this x.  (Otherwise it runs as usual.)
    if (!(__ballot(cl || x == lb || x == ub) & 0x7Full) && all8_below(fabs(xsf - x), C.qp_th_grad)) {
      BQ_ACC(5);
      break;
    }
    BQ_ACC(5);
  }
  return true;
}

// LATE: the variant for the latency-bound iterations (few instances left):
// phase C fully unrolled (classical), 1 wave/SIMD register budget.  Both variants are
// launched every iteration; the device-side active count picks the one that
// works (late_max: the most active instances the LATE variant takes, so its
// waves fit one per SIMD), the other one's blocks exit at once.
template <bool FF, bool LATE = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LATE ? 1 : (FF ? 2 : BW_WAVES)))) void k_backward_w(
    const DevConsts* __restrict__ Cg, Dev d, int iter, int cur, int late_max, int w2_max) {
  using S_t = BwW<FF>;
  constexpr int NX = S_t::NX, ND = S_t::ND, REC = S_t::REC, QXU = S_t::QXU, QH = S_t::QH;
  constexpr int NPF = (REC + 63) / 64;  // prefetch registers per lane
  constexpr bool PF_LATE = BW_PF_LATE == 2 || (BW_PF_LATE == 1 && FF);
  const DevConsts& C = *Cg;
  const int N = C.N;
  const int l = threadIdx.x;
  if (blockIdx.x == 0 && l == 0) d.acnt[cur ^ 1] = d.acnt[2 + (cur ^ 1)] = 0;  // the list k_accept builds
  const ActiveList al = active_list(d, cur);
  // active-count ranges: (late_max, B] this variant, (w2_max, late_max] LATE,
  // [1, w2_max] the two-wave k_backward_w2
  if ((int)blockIdx.x >= al.n || (LATE ? (al.n > late_max || al.n <= w2_max) : al.n <= late_max)) return;
  // one instance per block: the index (and every address derived from it) in SGPRs
  const int b = __builtin_amdgcn_readfirstlane(al.list[blockIdx.x]);
  InstState* st = d.st + b;
  if (st->done) return;
  // LATE runs a slice's latency-bound tail: its wave should have its SIMD to
  // itself.  FF's pass fits 254 VGPRs, which would let another slice's
  // k_node wave (253) share the SIMD (FF B = 1024: backward 306 -> 330 us
  // per launch); 40 reserved AGPRs keep the allocation above 256
  if (LATE && FF) RESERVE_AGPR40();
#ifdef FFDDP_PHASE_PROF
  const bool pp_on = (b == 0);
#endif
  PP_INIT();
  __shared__ S_t S;
  const bool feas = st->is_feasible != 0;
  const bool use_qp = C.use_box && feas;
  const double dt = C.dt, dt2 = C.dt * C.dt, alpha = C.alpha, beta = C.beta;
  const double* recb = d.rec_buf + (long)b * (N + 1) * REC;
  // this instance's slices of the state arrays (uniform bases, 32-bit lane
  // offsets in the node loop)
  const double* fs_i = d.fs + (long)b * (N + 1) * NX;
  const double* k_i = d.k + (long)b * N * NU;
  const double* us_i = d.us + (long)b * N * NU;
  double* K_i = d.K + (long)b * N * NU * NX;
  double* kw_i = d.k + (long)b * N * NU;
  double* w_i = d.w + (long)b * (N + 1) * NX;
  if (st->recalc) {
    double c = 0.0;
    for (int t = l; t <= N; t += 64) c += recb[(long)t * REC + rec_off_cost(NX)];
    c = wave_sum(c);
    if (l == 0) {
      st->cost = c;
      st->n_calc += 1;
    }
  }
  double preg = st->preg;
  int retries = 0;
  bool fail_inst = false;
  double dg = 0.0, dq = 0.0, stop = 0.0, ffl = 0.0;
  {
    // per-instance torque limits (d.ul, wave-uniform): the row's u_ub and its negation; once per pass
    double ulb_l = C.u_lb[l % NU], uub_l = C.u_ub[l % NU];
    if (d.ul && C.use_box) {
      uub_l = d.ul[(long)b * FFDDP_TAU_LIM_W + 4 * (l % NU)];
      ulb_l = -uub_l;
    }
    S.ulb[BW_DIET_SLOTS ? l % NU : l] = ulb_l;
    S.uub[BW_DIET_SLOTS ? l % NU : l] = uub_l;
  }
  // this lane's lower-triangle entries of Q (phase C) and V (phase F), fixed for the whole pass
  constexpr int NQE = ND * (ND + 1) / 2, NQL = (NQE + 63) / 64;
  // phase C unroll: full in the latency variants (FF's 7 passes move into
  // AGPRs, but since the LDS diet that is 1.4 % faster at B=1024)
  constexpr int QC_N = LATE ? (FF ? (QC_FF_LATE ? QC_FF_LATE : NQL) : NQL) : QC_UNROLL;
  constexpr int NVE = NX * (NX + 1) / 2, NVL = (NVE + 63) / 64;
  unsigned qrc[NQL];
  int vij[NVL];
#pragma unroll
  for (int k = 0; k < NQL; ++k) {
    int r = 0, c = 0;
    tri_rc(spare_entry(l + 64 * k, NQE, 64 * (NQL - 1)), r, c);
    qrc[k] = q_entry<NX>(r, c);
  }
#pragma unroll
  for (int k = 0; k < NVL; ++k) {
    int i = 0, j = 0;
    if (l + 64 * k < NVE) tri_rc(l + 64 * k, i, j);
    vij[k] = (i << 8) | j;
  }
  for (;;) {
    dg = dq = stop = ffl = 0.0;
    bool failed = false;
    // the bases, opaque per pass: the addresses of the terminal node's
    // inputs and of the first prefetch are then formed in each pass instead
    // of being hoisted out of the retry loop and held across it (FF: 15 of
    // them spilled, classical 8 more VGPRs)
    gptr<const double> rbase = (gptr<const double>)recb, fsb = (gptr<const double>)fs_i,
                       kb = (gptr<const double>)k_i, usb = (gptr<const double>)us_i;
    gptr<double> wb = (gptr<double>)w_i;
    asm volatile("" : "+s"(rbase), "+s"(fsb), "+s"(kb), "+s"(usb), "+s"(wb));
    // ---- terminal node: Vxx = Lxx_N + preg I ; Vx = Lx_N (+ Vxx fs_N) ----
    {
      gptr<const double> rT = rbase + (long)N * REC;
      for (int e = l; e < NX * NX; e += 64) {
        const int i = e / NX, j = e % NX;
        S.V[e] = rT[rec_off_Lxx(NX) + e] + (i == j ? preg : 0.0);
      }
      S.fs[BW_DIET_SLOTS ? l % NX : l] = fsb[N * NX + l % NX];
    }
    lds_sync();
    // Prefetch of the next node's inputs: unconditional loads from clamped
    // addresses and unguarded LDS stores, so the code stays straight-line and
    // the compiler can wait on exactly these loads (a guarded store makes it
    // wait vmcnt(0), i.e. also on the previous node's K / k / w stores).
    const int lx = l % NX, lu = l % NU;  // every lane loads and stages slot l mod n
    const int sx = BW_DIET_SLOTS ? lx : l, su = BW_DIET_SLOTS ? lu : l;
    double pf[NPF];
    {
      gptr<const double> r1 = rbase + (long)(N - 1) * REC;
#pragma unroll
      for (int k = 0; k < NPF; ++k) pf[k] = r1[(l + 64 * k < REC) ? l + 64 * k : REC - 1];
    }
    double pfs = fsb[(N - 1) * NX + lx];
    double pkp = kb[(N - 1) * NU + lu];
    double pus = usb[(N - 1) * NU + lu];
    {
      double cdg = 0.0, cdq = 0.0;
      if (l < NX) {
        gptr<const double> rT = rbase + (long)N * REC;
        double vfs = 0.0;
        for (int i = 0; i < NX; ++i) vfs += S.V[i * NX + l] * S.fs[i];
        const double fj = S.fs[l];
        ffl = fabs(fj);
        const double vx = rT[rec_off_Lx(NX) + l] + (feas ? 0.0 : vfs);
        if (!feas) {
          wb[N * NX + l] = vfs;
          cdg = -vx * fj;
          cdq = fj * vfs;
        }
        S.Vx[l] = vx;
      }
      dg += cdg;  // lane-local; summed over the wave after the node loop
      dq += cdq;
    }
    lds_sync();
    if (PF_LATE) {
#pragma unroll
      for (int k = 0; k < NPF; ++k) S.R[l + 64 * k] = pf[k];  // record N-1; the node loop stages the rest
    }
    for (int t = N - 1; t >= 0; --t) {
      // ---- stage record t (prefetched) ; start loading record t-1 ----
      if (!PF_LATE) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) S.R[l + 64 * k] = pf[k];
      }
      S.fs[sx] = pfs;
      S.kp[su] = pkp;
      S.uu[su] = pus;
      {
        const int tn = t > 0 ? t - 1 : 0;
        if (!PF_LATE) {
#pragma unroll
          for (int k = 0; k < NPF; ++k) pf[k] = recb[(unsigned)(tn * REC + ((l + 64 * k < REC) ? l + 64 * k : REC - 1))];
        }
        pfs = fs_i[(unsigned)(tn * NX + lx)];
        pkp = k_i[(unsigned)(tn * NU + lu)];
        pus = us_i[(unsigned)(tn * NU + lu)];
      }
      // no barrier here: phase A reads only V / Vx, and its closing barrier
      // publishes the staged record and gap before phase B reads them
      PP(0);
      const double* Ar = S.R + rec_off_A();
      // ---- phase A: W = V D (NX x 7), Y = D' V D (7 x 7), z = D' Vx ----
#pragma unroll
      for (int k = 0; k < (NX * NU + 63) / 64; ++k) {
        const int e = l + 64 * k;
        if (e < NX * NU) {
          const int i = e / NU, m = e - (e / NU) * NU;
          S.W[e] = dt2 * S.V[i * NX + m] + dt * S.V[i * NX + 7 + m];
        }
      }
      if (l < NU * NU) {
        const int m = l / NU, n = l - (l / NU) * NU;
        const double wq = dt2 * S.V[m * NX + n] + dt * S.V[m * NX + 7 + n];
        const double wv = dt2 * S.V[(7 + m) * NX + n] + dt * S.V[(7 + m) * NX + 7 + n];
        S.sl.Y[l] = dt2 * wq + dt * wv;
      }
      if (l < NU) S.z[l] = dt2 * S.Vx[l] + dt * S.Vx[7 + l];
      lds_sync();
      PP(1);
      // ---- phase B: row c = l of M = I~'W + 1/2 A^'Y ; Qv[c] = [Lx; Lu] + I~'Vx + A^'z ----
      if (l < ND) {
        const int c = l;
        int r0, r1;
        double a0, a1;
        itilde2<FF>(c, dt, alpha, beta, r0, a0, r1, a1);
        const double ac = (FF && c >= 21) ? 0.0 : 1.0;
        const int cc = (FF && c >= 21) ? 0 : c;
        double Acol[NU];
#pragma unroll
        for (int n = 0; n < NU; ++n) Acol[n] = ac * Ar[cc * 7 + n];
#pragma unroll
        for (int m = 0; m < NU; ++m) {
          double h = 0.0;
#pragma unroll
          for (int n = 0; n < NU; ++n) h += Acol[n] * S.sl.Y[n * NU + m];
          S.sl.M[c * NU + m] = (a0 * S.W[r0 * NU + m] + a1 * S.W[r1 * NU + m]) + 0.5 * h;
        }
        double qv = (c < NX) ? S.R[rec_off_Lx(NX) + c] : S.R[rec_off_Lu(NX) + c - NX];
        qv += a0 * S.Vx[r0] + a1 * S.Vx[r1];
#pragma unroll
        for (int m = 0; m < NU; ++m) qv += Acol[m] * S.z[m];
        S.Qv[c] = qv;
      }
      lds_sync();
      PP(2);
      // ---- phase C: Q lower triangle (mirrored), entries fixed per lane ----
#pragma unroll QC_N
      for (int k = 0; k < NQL; ++k) {
        // no range guard: a lane past the last entry recomputes an entry of
        // the same (last) pass (spare_entry), so the passes need no divergent
        // branch and can interleave
        {
          const int r = (qrc[k] >> 27) & 31, c = (qrc[k] >> 22) & 31;
          double lv;
          if (r < NX)
            lv = S.R[rec_off_Lxx(NX) + r * NX + c];
          else if (c < NX)
            lv = S.R[rec_off_Lxu(NX) + c * NU + (r - NX)];
          else
            lv = S.R[rec_off_Luu(NX) + (r - NX) * NU + (c - NX)];
          int rr0, rr1, cr0, cr1;
          double ra0, ra1, ca0, ca1;
          itilde2<FF>(r, dt, alpha, beta, rr0, ra0, rr1, ra1);
          itilde2<FF>(c, dt, alpha, beta, cr0, ca0, cr1, ca1);
          const double g = ra0 * (ca0 * S.V[rr0 * NX + cr0] + ca1 * S.V[rr0 * NX + cr1]) +
                           ra1 * (ca0 * S.V[rr1 * NX + cr0] + ca1 * S.V[rr1 * NX + cr1]);
          const double sr = (FF && r >= 21) ? 0.0 : 1.0, sc = (FF && c >= 21) ? 0.0 : 1.0;
          const int ir = (FF && r >= 21) ? 0 : r, ic = (FF && c >= 21) ? 0 : c;
          double h1 = 0.0, h2 = 0.0;
#pragma unroll
          for (int m = 0; m < NU; ++m) {
            h1 += S.sl.M[r * NU + m] * Ar[ic * 7 + m];
            h2 += S.sl.M[c * NU + m] * Ar[ir * 7 + m];
          }
          double v = lv + g + (sc * h1 + sr * h2);
          if (r == c && r >= NX) v += preg;
          S.QQ[(qrc[k] >> 11) & 2047] = v;
          S.QQ[qrc[k] & 2047] = v;
        }
      }
      lds_sync();
      PP(3);
      // ---- phase D: gains (Eigen::LLT or BoxQP), row / variable i on lane i ----
      int clm = 0;  // the final clamped set (uniform: phase E runs on this wave)
      constexpr bool EREG = e_from_regs(NX);
      double Lr[NU];  // the factor (EREG: read by phase E from these registers)
      {
        double hrow[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) hrow[j] = (l < NU) ? S.QQ[QH + l * NU + j] : (l == j ? 1.0 : 0.0);
        bool ok;
        if (!use_qp) {
#pragma unroll
          for (int j = 0; j < NU; ++j) Lr[j] = hrow[j];
          ok = chol_rows(Lr, l);
        } else {
          const bool v = l < NU;
          const double q = v ? S.Qv[NX + l] : 0.0;
          const double lb = v ? S.ulb[l % NU] - S.uu[l % NU] : 0.0;
          const double ub = v ? S.uub[l % NU] - S.uu[l % NU] : 0.0;
          double x = v ? S.kp[l % NU] : 0.0;
          ok = boxqp_lanes(C, hrow, q, lb, ub, x, Lr, clm, l);
          if (ok && v) {
            const bool c = (clm >> l) & 1;
            S.kk[l] = -x;
            if (c) S.Qv[NX + l] = 0.0;  // BoxFDDP: clamped Qu entries are zeroed
          }
        }
        if (!ok) {
          failed = true;
          break;
        }
        if (!EREG && l < NU)
#pragma unroll
          for (int j = 0; j < NU; ++j)
            if (j <= l) S.sl.L[tri(l, j)] = Lr[j];
      }
      lds_sync();
      PP(4);
      if (PF_LATE) {  // the next node's record (S.R is dead after phase C)
        const int tn = t > 0 ? t - 1 : 0;
#pragma unroll
        for (int k = 0; k < NPF; ++k) pf[k] = recb[(unsigned)(tn * REC + ((l + 64 * k < REC) ? l + 64 * k : REC - 1))];
      }
      // ---- phase E: K columns (and k for LLT) ----
      if (l < NX || (!use_qp && l == NX)) {
        double col[NU];
        if (l < NX) {
#pragma unroll
          for (int c = 0; c < NU; ++c) col[c] = ((clm >> c) & 1) ? 0.0 : S.QQ[QXU + l * NU + c];
        } else {
#pragma unroll
          for (int c = 0; c < NU; ++c) col[c] = S.Qv[NX + c];
        }
        if (EREG) {
          double Lt[NU * (NU + 1) / 2];
          rows_to_tri(Lr, Lt);
          chol_solve<NU>(Lt, col);
        } else {
          chol_solve<NU>(S.sl.L, col);
        }
        if (l < NX) {
#pragma unroll
          for (int c = 0; c < NU; ++c) {
            S.sl.K[c * NX + l] = col[c];
            K_i[(unsigned)((t * NU + c) * NX + l)] = col[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < NU; ++c) S.kk[c] = col[c];
        }
      }
      lds_sync();
      PP(5);
      // ---- phase F: Vxx = sym(Qxx - Qxu K) + preg I (lower triangle, mirrored) ----
      int badv = 0;
#pragma unroll 1
      for (int k = 0; k < NVL; ++k) {
        if (l + 64 * k >= NVE) continue;
        const int i = vij[k] >> 8, j = vij[k] & 255;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) {
          a1 += S.QQ[QXU + i * NU + c] * S.sl.K[c * NX + j];
          a2 += S.QQ[QXU + j * NU + c] * S.sl.K[c * NX + i];
        }
        const double v = S.QQ[i * NX + j] - 0.5 * (a1 + a2) + (i == j ? preg : 0.0);
        S.V[i * NX + j] = v;
        S.V[j * NX + i] = v;
        badv |= bad(fabs(v)) ? 1 : 0;
      }
      lds_sync();
      PP(6);
      // ---- phase G: Vx, gap terms, expected improvement, k ----
      double cdg = 0.0, cdq = 0.0, cst = 0.0;
      if (l < NX) {
        // V fs (the gap term) only while infeasible: a feasible pass never
        // reads it (uniform branch; FF computes it always: the branch costs
        // its throughput pass a 12 B spill)
        double vfs = 0.0;
        if (FF || !feas) {
#pragma unroll
          for (int i = 0; i < NX; ++i) vfs += S.V[i * NX + l] * S.fs[i];
        }
        double vx = S.Qv[l];
#pragma unroll
        for (int c = 0; c < NU; ++c) vx -= S.sl.K[c * NX + l] * S.Qv[NX + c];
        if (!feas) vx += vfs;
        badv |= bad(fabs(vx)) ? 1 : 0;
        ffl = fmax(ffl, fabs(S.fs[l]));
        if (!feas) {
          w_i[(unsigned)(t * NX + l)] = vfs;
          cdg -= vx * S.fs[l];
          cdq += S.fs[l] * vfs;
        }
        if (l < NU) {
          double quk = 0.0;
#pragma unroll
          for (int m = 0; m < NU; ++m) quk += S.QQ[QH + l * NU + m] * S.kk[m];
          const double qu = S.Qv[NX + l], kl = S.kk[l];
          cdg += qu * kl;
          cdq -= kl * quk;
          cst += qu * qu;
          kw_i[(unsigned)(t * NU + l)] = kl;
        }
        S.Vx[l] = vx;  // old Vx is dead after phase B
      }
      badv = __any(badv);
      if (badv) {
        failed = true;
        break;
      }
      dg += cdg;
      dq += cdq;
      stop += cst;
      if (PF_LATE) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) S.R[l + 64 * k] = pf[k];
      }
      lds_sync();
      PP(7);
    }
    // ---- retry bookkeeping (SolverFDDP::solve: increaseRegularization) ----
    if (!failed) {
      // expected-improvement terms: lane-local sums over the nodes, reduced
      // once here instead of three wave reductions per node
      dg = wave_sum(dg);
      dq = wave_sum(dq);
      stop = wave_sum(stop);
      ffl = wave_max(ffl);
      break;
    }
    retries++;
    preg = fmin(preg * C.reg_inc, C.reg_max);
    if (preg == C.reg_max) {
      fail_inst = true;
      break;
    }
    lds_sync();
  }
  PP_FLUSH();
  if (l == 0) {
    st->preg = preg;
    st->n_retries += retries;
    // the trial k_node read in place has been written into (xs, us): no
    // later kernel may take it for the current iterate (k_commit)
    st->accepted = -1;
    if (fail_inst) {
      st->bw_ok = 0;
      st->iter = iter;
      st->done = 1;
      st->ok = 0;
      st->n_backward += retries;
    } else {
      st->dg = dg;
      st->dq = dq;
      st->stop = stop;
      st->ffeas = ffl;
      st->bw_ok = 1;
      st->n_backward += retries + 1;
      st->n_iters += 1;
    }
  }
}

// ---------------------------------------------------------------------------
// k_backward_w2: the backward pass on TWO wavefronts per instance, for slices
// whose active instances fit two waves per SIMD-pair (the latency-bound
// end of a solve and small per-GPU batches).  Same per-entry arithmetic as
// k_backward_w (bit-identical results), spread over 128 lanes:
//   A, B, C, F  the entry-parallel phases on both waves (half the passes),
//   D           gains on wave 0 (rows on lanes 0..6) while wave 1 stages the
//               next node's record into LDS (S.R is dead after phase C) and
//               issues the prefetch of the one after,
//   E, G        wave 0 (one column / state component per lane, as before).
// ---------------------------------------------------------------------------
// WPE: waves per SIMD the register budget allows.  1 (296 registers) for
// small slices, where the pass is the solve's chain; 2 (256, some spilled)
// in the tails of large slices, where a block that needs two whole SIMDs
// waits for the other slices' kernels to drain them: at 2 its waves share a
// SIMD with one of theirs (B = 4096: +2 % over the one-wave LATE variant
// there).  Same arithmetic either way.
template <bool FF, int WPE = 1>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(WPE))) void k_backward_w2(
    const DevConsts* __restrict__ Cg, Dev d, int iter, int cur, int w2_max) {
  using S_t = BwW<FF>;
  constexpr int NX = S_t::NX, ND = S_t::ND, REC = S_t::REC, QXU = S_t::QXU, QH = S_t::QH;
  constexpr int NPF = (REC + 63) / 64;  // prefetch registers per lane of wave 1
  const DevConsts& C = *Cg;
  const int N = C.N;
  const int tid = threadIdx.x;
  const int wv = tid >> 6, l = tid & 63;
  if (blockIdx.x == 0 && tid == 0) d.acnt[cur ^ 1] = d.acnt[2 + (cur ^ 1)] = 0;  // the list k_accept builds
  const ActiveList al = active_list(d, cur);
  if ((int)blockIdx.x >= al.n || al.n > w2_max) return;
  // one instance per block: the index (and every address derived from it) in SGPRs
  const int b = __builtin_amdgcn_readfirstlane(al.list[blockIdx.x]);
  InstState* st = d.st + b;
  if (st->done) return;
#ifdef FFDDP_PHASE_PROF
  const bool pp_on = (b == 0) && tid == 0;
  unsigned long long dwave = 0;
#endif
  PP_INIT();
  __shared__ S_t S;
  const bool feas = st->is_feasible != 0;
  const bool use_qp = C.use_box && feas;
  const double dt = C.dt, dt2 = C.dt * C.dt, alpha = C.alpha, beta = C.beta;
  const double* recb = d.rec_buf + (long)b * (N + 1) * REC;
  // this instance's slices of the state arrays (uniform bases, 32-bit lane
  // offsets in the node loop)
  const double* fs_i = d.fs + (long)b * (N + 1) * NX;
  const double* k_i = d.k + (long)b * N * NU;
  const double* us_i = d.us + (long)b * N * NU;
  double* K_i = d.K + (long)b * N * NU * NX;
  double* kw_i = d.k + (long)b * N * NU;
  double* w_i = d.w + (long)b * (N + 1) * NX;
  if (st->recalc && wv == 0) {
    double c = 0.0;
    for (int t = l; t <= N; t += 64) c += recb[(long)t * REC + rec_off_cost(NX)];
    c = wave_sum(c);
    if (l == 0) {
      st->cost = c;
      st->n_calc += 1;
    }
  }
  double preg = st->preg;
  int retries = 0;
  bool fail_inst = false;
  double dg = 0.0, dq = 0.0, stop = 0.0, ffl = 0.0;
  if (wv == 0) {
    // per-instance torque limits (d.ul, wave-uniform): the row's u_ub and its negation; once per pass
    double ulb_l = C.u_lb[l % NU], uub_l = C.u_ub[l % NU];
    if (d.ul && C.use_box) {
      uub_l = d.ul[(long)b * FFDDP_TAU_LIM_W + 4 * (l % NU)];
      ulb_l = -uub_l;
    }
    S.ulb[BW_DIET_SLOTS ? l % NU : l] = ulb_l;
    S.uub[BW_DIET_SLOTS ? l % NU : l] = uub_l;
  }
  // this lane's lower-triangle entries of Q (phase C) and V (phase F) over 128 lanes
  constexpr int NQE = ND * (ND + 1) / 2, NQL = (NQE + 127) / 128;
  constexpr int NVE = NX * (NX + 1) / 2, NVL = (NVE + 127) / 128;
  unsigned qrc[NQL];
  int vij[NVL];
#pragma unroll
  for (int k = 0; k < NQL; ++k) {
    int r = 0, c = 0;
    tri_rc(spare_entry(tid + 128 * k, NQE, 128 * (NQL - 1)), r, c);
    qrc[k] = q_entry<NX>(r, c);
  }
#pragma unroll
  for (int k = 0; k < NVL; ++k) {
    int i = 0, j = 0;
    if (tid + 128 * k < NVE) tri_rc(tid + 128 * k, i, j);
    vij[k] = (i << 8) | j;
  }
  const int lx = l % NX, lu = l % NU;  // every lane loads and stages slot l mod n
  const int sx = BW_DIET_SLOTS ? lx : l, su = BW_DIET_SLOTS ? lu : l;
  for (;;) {
    dg = dq = stop = ffl = 0.0;
    bool failed = false;
    // the bases, opaque per pass (k_backward_w)
    gptr<const double> rbase = (gptr<const double>)recb, fsb = (gptr<const double>)fs_i,
                       kb = (gptr<const double>)k_i, usb = (gptr<const double>)us_i;
    gptr<double> wb = (gptr<double>)w_i;
    asm volatile("" : "+s"(rbase), "+s"(fsb), "+s"(kb), "+s"(usb), "+s"(wb));
    // ---- terminal node: Vxx = Lxx_N + preg I ; Vx = Lx_N (+ Vxx fs_N) ----
    {
      gptr<const double> rT = rbase + (long)N * REC;
      for (int e = tid; e < NX * NX; e += 128) {
        const int i = e / NX, j = e % NX;
        S.V[e] = rT[rec_off_Lxx(NX) + e] + (i == j ? preg : 0.0);
      }
      if (wv == 0) S.fs[sx] = fsb[N * NX + lx];
    }
    // wave 1: record N-1 into LDS now, the prefetch of record N-2 in flight
    double pf[NPF];
    if (wv == 1) {
      gptr<const double> r1 = rbase + (long)(N - 1) * REC;
#pragma unroll
      for (int k = 0; k < NPF; ++k) pf[k] = r1[(l + 64 * k < REC) ? l + 64 * k : REC - 1];
#pragma unroll
      for (int k = 0; k < NPF; ++k) S.R[l + 64 * k] = pf[k];
      gptr<const double> r2 = rbase + (long)(N > 1 ? N - 2 : 0) * REC;
#pragma unroll
      for (int k = 0; k < NPF; ++k) pf[k] = r2[(l + 64 * k < REC) ? l + 64 * k : REC - 1];
    }
    lds_sync();
    double pfs = 0.0, pkp = 0.0, pus = 0.0;
    if (wv == 0) {
      pfs = fsb[(N - 1) * NX + lx];
      pkp = kb[(N - 1) * NU + lu];
      pus = usb[(N - 1) * NU + lu];
      double cdg = 0.0, cdq = 0.0;
      if (l < NX) {
        gptr<const double> rT = rbase + (long)N * REC;
        double vfs = 0.0;
        for (int i = 0; i < NX; ++i) vfs += S.V[i * NX + l] * S.fs[i];
        const double fj = S.fs[l];
        ffl = fabs(fj);
        const double vx = rT[rec_off_Lx(NX) + l] + (feas ? 0.0 : vfs);
        if (!feas) {
          wb[N * NX + l] = vfs;
          cdg = -vx * fj;
          cdq = fj * vfs;
        }
        S.Vx[l] = vx;
      }
      dg += cdg;
      dq += cdq;
    }
    lds_sync();
    // ---- phase G of node tg: Vx, gap terms, expected improvement, k (wave 0) ----
    int badf = 0;  // wave 0's non-finite V entries of phase F, reported with its phase G
    auto phase_g = [&](int tg) {
      double cdg = 0.0, cdq = 0.0, cst = 0.0;
      int badv = badf;
      if (l < NX) {
        double vfs = 0.0;
        const double* fsg = S.fsb[tg & 1];
        if (FF || !feas) {  // the gap term only while infeasible (uniform branch)
#pragma unroll
          for (int i = 0; i < NX; ++i) vfs += S.V[i * NX + l] * fsg[i];
        }
        double vx = S.Qv[l];
#pragma unroll
        for (int c = 0; c < NU; ++c) vx -= S.sl.K[c * NX + l] * S.Qv[NX + c];
        if (!feas) vx += vfs;
        badv |= bad(fabs(vx)) ? 1 : 0;
        ffl = fmax(ffl, fabs(fsg[l]));
        if (!feas) {
          w_i[(unsigned)(tg * NX + l)] = vfs;
          cdg -= vx * fsg[l];
          cdq += fsg[l] * vfs;
        }
        if (l < NU) {
          double quk = 0.0;
#pragma unroll
          for (int m = 0; m < NU; ++m) quk += S.QQ[QH + l * NU + m] * S.kk[m];
          const double qu = S.Qv[NX + l], kl = S.kk[l];
          cdg += qu * kl;
          cdq -= kl * quk;
          cst += qu * qu;
          kw_i[(unsigned)(tg * NU + l)] = kl;
        }
        S.Vx[l] = vx;  // old Vx is dead after phase B
      }
      badv = __any(badv);
      if (l == 0) S.badw[0] = badv;
      // (a failed node aborts the pass, which restarts with dg / dq / stop reset)
      dg += cdg;
      dq += cdq;
      stop += cst;
    };
    for (int t = N - 1; t >= 0; --t) {
      // ---- wave 0: phase G of node t+1 beside this node's phase A (one
      // barrier less per node), then this node's gap / warm start / control
      // (record t is in LDS) ----
      if (wv == 0) {
        // staging first: its wait for the loads prefetched one node ago
        // would otherwise also wait for phase G's global stores (w, k) just
        // issued (vmcnt counts loads and stores in issue order, and the
        // lane-guarded stores leave the compiler only vmcnt(0)); staged
        // here, the stores have a whole node to complete before the next wait
        S.fsb[t & 1][sx] = pfs;
        S.kp[su] = pkp;
        S.uu[su] = pus;
        const int tn = t > 0 ? t - 1 : 0;
        pfs = fs_i[(unsigned)(tn * NX + lx)];
        pkp = k_i[(unsigned)(tn * NU + lu)];
        pus = us_i[(unsigned)(tn * NU + lu)];
        PP(8);  // (profiling build: wave 0's staging apart from its phase G)
        if (t < N - 1) {
          phase_g(t + 1);
          // z below reads Vx entries other lanes of this wave just wrote
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        }
      }
      PP(0);
      const double* Ar = S.R + rec_off_A();
      // ---- phase A: W = V D (NX x 7), Y = D' V D (7 x 7), z = D' Vx ----
      for (int e = tid; e < NX * NU; e += 128) {
        const int i = e / NU, m = e - (e / NU) * NU;
        S.W[e] = dt2 * S.V[i * NX + m] + dt * S.V[i * NX + 7 + m];
      }
      if (tid >= 128 - NU * NU) {
        const int e = tid - (128 - NU * NU);
        const int m = e / NU, n = e - (e / NU) * NU;
        const double wq = dt2 * S.V[m * NX + n] + dt * S.V[m * NX + 7 + n];
        const double wv_ = dt2 * S.V[(7 + m) * NX + n] + dt * S.V[(7 + m) * NX + 7 + n];
        S.sl.Y[e] = dt2 * wq + dt * wv_;
      }
      if (tid < NU) S.z[tid] = dt2 * S.Vx[tid] + dt * S.Vx[7 + tid];
      lds_sync();
      PP(1);
      // node t+1's phase F / G flags: read now, tested after phase B (whose
      // results a failed pass discards), so the LDS round trip is not on the
      // node's chain
      const int badprev = t < N - 1 ? (S.badw[0] | S.badw[1]) : 0;
      // ---- phase B: row c of M = I~'W + 1/2 A^'Y (columns m split over the
      // two waves) ; Qv[c] = [Lx; Lu] + I~'Vx + A^'z (wave 1) ----
      if (l < ND) {
        const int c = l;
        int r0, r1;
        double a0, a1;
        itilde2<FF>(c, dt, alpha, beta, r0, a0, r1, a1);
        const double ac = (FF && c >= 21) ? 0.0 : 1.0;
        const int cc = (FF && c >= 21) ? 0 : c;
        double Acol[NU];
#pragma unroll
        for (int n = 0; n < NU; ++n) Acol[n] = ac * Ar[cc * 7 + n];
        // columns [M0, M1) with compile-time bounds, so their independent
        // 7-term chains interleave (a runtime column range kept each column in
        // a basic block of its own: one LDS round trip and one dependent
        // chain after another)
        auto mcols = [&](auto m0c, auto m1c) {
          constexpr int M0 = decltype(m0c)::value, M1 = decltype(m1c)::value;
          double h[M1 - M0];
#pragma unroll
          for (int m = M0; m < M1; ++m) {
            h[m - M0] = 0.0;
#pragma unroll
            for (int n = 0; n < NU; ++n) h[m - M0] += Acol[n] * S.sl.Y[n * NU + m];
          }
#pragma unroll
          for (int m = M0; m < M1; ++m)
            S.sl.M[c * NU + m] = (a0 * S.W[r0 * NU + m] + a1 * S.W[r1 * NU + m]) + 0.5 * h[m - M0];
        };
        if (wv == 0)
          mcols(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{});
        else
          mcols(std::integral_constant<int, 4>{}, std::integral_constant<int, NU>{});
        if (wv == 1) {
          double qv = (c < NX) ? S.R[rec_off_Lx(NX) + c] : S.R[rec_off_Lu(NX) + c - NX];
          qv += a0 * S.Vx[r0] + a1 * S.Vx[r1];
#pragma unroll
          for (int m = 0; m < NU; ++m) qv += Acol[m] * S.z[m];
          S.Qv[c] = qv;
        }
      }
      lds_sync();
      if (badprev) {
        failed = true;
        break;
      }
      PP(2);
      // ---- phase C: Q lower triangle (mirrored), entries over 128 lanes ----
#pragma unroll
      for (int k = 0; k < NQL; ++k) {
        // no range guard: a lane past the last entry recomputes an entry of
        // the same (last) pass (spare_entry), so the passes need no divergent
        // branch and can interleave
        {
          const int r = (qrc[k] >> 27) & 31, c = (qrc[k] >> 22) & 31;
          double lv;
          if (r < NX)
            lv = S.R[rec_off_Lxx(NX) + r * NX + c];
          else if (c < NX)
            lv = S.R[rec_off_Lxu(NX) + c * NU + (r - NX)];
          else
            lv = S.R[rec_off_Luu(NX) + (r - NX) * NU + (c - NX)];
          int rr0, rr1, cr0, cr1;
          double ra0, ra1, ca0, ca1;
          itilde2<FF>(r, dt, alpha, beta, rr0, ra0, rr1, ra1);
          itilde2<FF>(c, dt, alpha, beta, cr0, ca0, cr1, ca1);
          const double g = ra0 * (ca0 * S.V[rr0 * NX + cr0] + ca1 * S.V[rr0 * NX + cr1]) +
                           ra1 * (ca0 * S.V[rr1 * NX + cr0] + ca1 * S.V[rr1 * NX + cr1]);
          const double sr = (FF && r >= 21) ? 0.0 : 1.0, sc = (FF && c >= 21) ? 0.0 : 1.0;
          const int ir = (FF && r >= 21) ? 0 : r, ic = (FF && c >= 21) ? 0 : c;
          double h1 = 0.0, h2 = 0.0;
#pragma unroll
          for (int m = 0; m < NU; ++m) {
            h1 += S.sl.M[r * NU + m] * Ar[ic * 7 + m];
            h2 += S.sl.M[c * NU + m] * Ar[ir * 7 + m];
          }
          double v = lv + g + (sc * h1 + sr * h2);
          if (r == c && r >= NX) v += preg;
          S.QQ[(qrc[k] >> 11) & 2047] = v;
          S.QQ[qrc[k] & 2047] = v;
        }
      }
      lds_sync();
      PP(3);
#ifdef FFDDP_PHASE_PROF
      const unsigned long long dwt0 = __builtin_readcyclecounter();
#endif
      // ---- phase D: gains on wave 0 (rows on lanes 0..6); wave 1 stages the
      // next node's record (S.R is not read after phase C) ----
      constexpr bool EREG = e_from_regs(NX);
      double Lr0[NU];  // wave 0's factor (EREG: read by phase E from these registers)
      if (wv == 0) {
        double hrow[NU];
        double (&Lr)[NU] = Lr0;
#pragma unroll
        for (int j = 0; j < NU; ++j) hrow[j] = (l < NU) ? S.QQ[QH + l * NU + j] : (l == j ? 1.0 : 0.0);
        bool ok;
        int clm = 0;
        if (!use_qp) {
#pragma unroll
          for (int j = 0; j < NU; ++j) Lr[j] = hrow[j];
          ok = chol_rows(Lr, l);
        } else {
          const bool v = l < NU;
          const double q = v ? S.Qv[NX + l] : 0.0;
          const double lb = v ? S.ulb[l % NU] - S.uu[l % NU] : 0.0;
          const double ub = v ? S.uub[l % NU] - S.uu[l % NU] : 0.0;
          double x = v ? S.kp[l % NU] : 0.0;
#ifdef FFDDP_PHASE_PROF
          unsigned long long bq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          ok = boxqp_lanes(C, hrow, q, lb, ub, x, Lr, clm, l, b == 0 ? bq : nullptr);
          if (b == 0 && l == 0)
            for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&g_pp[32 + k_], bq[k_]);
#else
          ok = boxqp_lanes(C, hrow, q, lb, ub, x, Lr, clm, l);
#endif
          if (ok && v) {
            const bool c = (clm >> l) & 1;
            S.kk[l] = -x;
            if (c) S.Qv[NX + l] = 0.0;  // BoxFDDP: clamped Qu entries are zeroed
          }
        }
        if (!EREG && ok && l < NU)
#pragma unroll
          for (int j = 0; j < NU; ++j)
            if (j <= l) S.sl.L[tri(l, j)] = Lr[j];
        // ok, and the final clamped set above it (one LDS word for the tests below)
        if (l == 0) S.flag = ok ? 1 | (clm << 1) : 0;
      } else {
        if (t > 0) {
#pragma unroll
          for (int k = 0; k < NPF; ++k) S.R[l + 64 * k] = pf[k];
          const int tn = t > 1 ? t - 2 : 0;
#pragma unroll
          for (int k = 0; k < NPF; ++k) pf[k] = recb[(unsigned)(tn * REC + ((l + 64 * k < REC) ? l + 64 * k : REC - 1))];
        }
        // Speculative gains on wave 1: the factor of the full set (Quu, or
        // Quu + qp_reg I as BoxQP factors an empty clamped set: the same
        // operations, so the same bits) and phase E's K columns (and the LLT
        // k) from it, while wave 0 runs the gains.  Used when the final
        // clamped set is empty (always for LLT); otherwise phase E runs.
        double hrow[NU], Lr[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) hrow[j] = (l < NU) ? S.QQ[QH + l * NU + j] : (l == j ? 1.0 : 0.0);
#pragma unroll
        for (int j = 0; j < NU; ++j) Lr[j] = use_qp ? hrow[j] + (l == j ? C.qp_reg : 0.0) : hrow[j];
        const bool ok1 = chol_rows(Lr, l);
        if (ok1) {
          if (l < NU)
#pragma unroll
            for (int j = 0; j < NU; ++j)
              if (j <= l) S.sl.L1[tri(l, j)] = Lr[j];
          // lanes of this wave read the rows the others just wrote: LDS
          // accesses of one wave complete in order; the fence keeps the
          // compiler from moving the reads above the writes
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
          if (l < NX || (!use_qp && l == NX)) {
            double col[NU];
            if (l < NX) {
#pragma unroll
              for (int c = 0; c < NU; ++c) col[c] = S.QQ[QXU + l * NU + c];
            } else {
#pragma unroll
              for (int c = 0; c < NU; ++c) col[c] = S.Qv[NX + c];
            }
            chol_solve<NU>(S.sl.L1, col);
            if (l < NX) {
              double* Kt = K_i + (unsigned)(t * NU * NX);
#pragma unroll
              for (int c = 0; c < NU; ++c) {
                S.sl.K[c * NX + l] = col[c];
                Kt[c * NX + l] = col[c];
              }
            } else {
#pragma unroll
              for (int c = 0; c < NU; ++c) S.kk[c] = col[c];
            }
          }
        }
        if (l == 0) S.spec = ok1 ? 1 : 0;
      }
#ifdef FFDDP_PHASE_PROF
      // development: each wave's own phase-D time (instance 0) into g_pp[28 + wave]
      if (b == 0 && l == 0) dwave += __builtin_readcyclecounter() - dwt0;
#endif
      lds_sync();
      PP(4);
      const int dflag = S.flag;
      if (dflag == 0) {
        failed = true;
        break;
      }
      // wave 1's gains stand unless BoxQP clamped a control
      const bool spec_ok = S.spec != 0 && (dflag >> 1) == 0;
      // ---- phase E: K columns (and k for LLT), wave 0 ----
      if (!spec_ok && wv == 0 && (l < NX || (!use_qp && l == NX))) {
        double col[NU];
        if (l < NX) {
#pragma unroll
          for (int c = 0; c < NU; ++c) col[c] = ((dflag >> (1 + c)) & 1) ? 0.0 : S.QQ[QXU + l * NU + c];
        } else {
#pragma unroll
          for (int c = 0; c < NU; ++c) col[c] = S.Qv[NX + c];
        }
        if (EREG) {
          double Lt[NU * (NU + 1) / 2];
          rows_to_tri(Lr0, Lt);
          chol_solve<NU>(Lt, col);
        } else {
          chol_solve<NU>(S.sl.L, col);
        }
        if (l < NX) {
          double* Kt = K_i + (unsigned)(t * NU * NX);
#pragma unroll
          for (int c = 0; c < NU; ++c) {
            S.sl.K[c * NX + l] = col[c];
            Kt[c * NX + l] = col[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < NU; ++c) S.kk[c] = col[c];
        }
      }
      if (!spec_ok) lds_sync();  // (uniform: read from LDS)
      PP(5);
      // ---- phase F: Vxx = sym(Qxx - Qxu K) + preg I, entries over 128 lanes ----
      int badv = 0;
#pragma unroll
      for (int k = 0; k < NVL; ++k) {
        if (tid + 128 * k >= NVE) continue;
        const int i = vij[k] >> 8, j = vij[k] & 255;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) {
          a1 += S.QQ[QXU + i * NU + c] * S.sl.K[c * NX + j];
          a2 += S.QQ[QXU + j * NU + c] * S.sl.K[c * NX + i];
        }
        const double v = S.QQ[i * NX + j] - 0.5 * (a1 + a2) + (i == j ? preg : 0.0);
        S.V[i * NX + j] = v;
        S.V[j * NX + i] = v;
        badv |= bad(fabs(v)) ? 1 : 0;
      }
      if (wv == 1) {
        badv = __any(badv);
        if (l == 0) S.badw[1] = badv;
      } else {
        badf = badv;
      }
      lds_sync();
      PP(6);
    }
    if (!failed) {
      if (wv == 0) phase_g(0);
      lds_sync();
      PP(7);
      if (S.badw[0] | S.badw[1]) failed = true;
    }
    // ---- retry bookkeeping (SolverFDDP::solve: increaseRegularization) ----
    if (!failed) {
      if (wv == 0) {
        dg = wave_sum(dg);
        dq = wave_sum(dq);
        stop = wave_sum(stop);
        ffl = wave_max(ffl);
      }
      break;
    }
    retries++;
    preg = fmin(preg * C.reg_inc, C.reg_max);
    if (preg == C.reg_max) {
      fail_inst = true;
      break;
    }
    lds_sync();
  }
  PP_FLUSH();
#ifdef FFDDP_PHASE_PROF
  if (b == 0 && l == 0) atomicAdd(&g_pp[28 + wv], dwave);
#endif
  if (tid == 0) {
    st->preg = preg;
    st->n_retries += retries;
    st->accepted = -1;
    if (fail_inst) {
      st->bw_ok = 0;
      st->iter = iter;
      st->done = 1;
      st->ok = 0;
      st->n_backward += retries;
    } else {
      st->dg = dg;
      st->dq = dq;
      st->stop = stop;
      st->ffeas = ffl;
      st->bw_ok = 1;
      st->n_backward += retries + 1;
      st->n_iters += 1;
    }
  }
}

// ---------------------------------------------------------------------------
// line search with an 8-lane group per (instance, step length): the rollout
// of one trial is still sequential over the nodes, but each node calc runs
// joint-parallel (node_calc_g8), which shortens the dependent chain that
// bounds this kernel.  Lane i < 7 carries joint i of x (q_i, v_i, FF tau_i).
// ---------------------------------------------------------------------------
// SolverFDDP::solve acceptance of trial tr (tryStep + expectedImprovement)
// for an instance in state s; dV / dVexp / d1 of the trial out (trace)
// the line search's results of instance b, trials 0..n-1, loaded at once
// (n is NTRIALS or the first pass's width): the acceptance loop below exits
// at the first accepted trial, and with the loads inside it every trial
// cost a dependent global-memory round trip
struct TrialRes {
  double cost[NTRIALS], dv[NTRIALS];
  bool fail[NTRIALS];
};
__device__ __forceinline__ void load_trials(const Dev& d, int b, int n, TrialRes& T) {
  const double* tb = d.trial + (long)b * NTRIALS * 2;
  const int* fb = d.trial_fail + (long)b * NTRIALS;
#pragma unroll
  for (int tr = 0; tr < NTRIALS; ++tr) {
    const bool in = tr < n;
    T.cost[tr] = in ? tb[2 * tr] : 0.0;
    T.dv[tr] = in ? tb[2 * tr + 1] : 0.0;
    T.fail[tr] = in ? fb[tr] != 0 : true;
  }
}

__device__ __forceinline__ bool trial_accepted(const DevConsts& C, const InstState& s, const TrialRes& T, int tr,
                                               double* o_dV = nullptr, double* o_dVexp = nullptr,
                                               double* o_d1 = nullptr) {
  if (T.fail[tr]) return false;
  const double a = C.alphas[tr];
  const double cost_try = T.cost[tr];
  const double dv = s.is_feasible ? 0.0 : T.dv[tr];
  const double dV = s.cost - cost_try;
  const double d0 = s.dg + dv, d1 = s.dq - 2.0 * dv;
  const double dVexp = a * (d0 + 0.5 * a * d1);
  if (o_dV) {
    *o_dV = dV;
    *o_dVexp = dVexp;
    *o_d1 = d1;
  }
  if (dVexp >= 0) return fabs(d0) < C.th_grad || dV > C.th_acceptstep * dVexp;
  // ascent direction (closing the gaps may raise the cost): only while
  // infeasible.  Crocoddyl's comparator is dV < th_acceptnegstep dVexp; the
  // alternative accepts a rise of at most th_acceptnegstep x the predicted
  // one (include/ffddp.h FFDDP_NEGSTEP_*)
  if (s.is_feasible) return false;
  return C.neg_rule == FFDDP_NEGSTEP_CROCODDYL ? dV < C.th_acceptnegstep * dVexp
                                               : dV > C.th_acceptnegstep * dVexp;
}

// Width of the line search's first pass, decided on the device: every step
// length at once while the slice's active instances fit the threshold
// wide_max and the previous iteration had an instance that needed more than
// the host's width n1 (then the second pass, a whole extra rollout on the
// iteration's chain, would likely run again), else n1.  The first pass, the
// second pass and k_accept read the same two values.  Which trials run in
// which pass changes no result (each trial is evaluated alone).
__device__ __forceinline__ int first_width(int n1, const Dev& d, int cur, int wide_max) {
  return (d.acnt[cur] <= wide_max && d.acnt[2 + cur] != 0) ? NTRIALS : n1;
}

// one wave per SIMD: the register budget holds the next node's K row,
// prefetched one node ahead (a 2-waves/SIMD variant without the prefetch
// measured slower in every iteration).
// ROW (ffddp_rollout.hpp): one trial group per 16-lane DPP row (latency
// layout) instead of two (throughput layout).  Both instantiations are
// launched for a pass whose layout the host cannot know; each reads the
// slice's active count and returns at once unless it is the chosen one:
// ROW while the pass's trial groups fit row_max (one wave per SIMD share at
// four groups per wave).  The two give the same bits, so the choice never
// makes a result depend on the batch.  The node loop is written with
// explicit fma under fp contract(off) for that reason.
__device__ __forceinline__ int ls_row_bcast0(int v) {  // lane 0 of the row into every lane of it
  return __builtin_amdgcn_update_dpp(v, v, 0x150, 0xf, 0xf, false);
}
#pragma clang fp contract(off)
#ifndef FW_WPE
#define FW_WPE 1  // waves per SIMD of the two-groups-per-row layout's register budget
#endif
// FR: d.fref[b][t] is the node's force reference, prefetched with its
// position / velocity references one node ahead.
// CW: the scalar cost weights are the instance's row d.cw[b].  A lane needs
// only its role's block of the row (joint lanes the state / control weights,
// the EE lane the frame / contact ones: LS_CW registers shared by both roles),
// loaded once before the node loop: the row does not depend on the node.
// UL: the BoxQP clamp, the torque soft-limit bounds and the w soft limit are
// the lane's three entries of the instance's row d.ul[b], held in registers
// next to W in place of LaneK's (per block, while a block's groups belong to
// different instances).  The EE lane takes joint 6's, as LaneK gives it.
// MD: the link's mass, centre of mass and rotational inertia are the joint
// lane's 13 entries of the instance's row d.md[b], held in registers next to W
// and L in place of LaneK's for the same reason (the kernel runs one wave per
// SIMD, so the registers are there: DESIGN.md §21).  The EE lane and the ROW
// layout's phantom lanes hold zeros, as LaneK gives them.
// MT: the base placement and the gravity vector are those of the instance's
// row d.mt[b], held in registers next to M for the same reason (LsT: lane 0 of
// the real and of the phantom group takes base_R / base_p, finite in both, the
// other lanes copy LaneK's placement once; every lane takes the gravity).
template <int NC, bool FF, bool ROW, bool FR = false, bool CW = false, bool UL = false, bool MD = false,
          bool MT = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ROW ? 1 : FW_WPE))) void k_forward_g8(const DevConsts* __restrict__ Cg, Dev d,
                                                   const double* __restrict__ x0,
                                                   const double* __restrict__ node_ref,
                                                   const double* __restrict__ inst_ref,
                                                   const uint8_t* __restrict__ surface, int tr0, int ntr,
                                                   int only_more, int cur, int wide_max, int row_max) {
  const DevConsts& C = *Cg;
  const int N = C.N;
  constexpr int nx = FF ? 21 : 14;
  constexpr int GL = ROW ? 16 : G8;  // lanes per trial group slot
  // host: first pass (0, n1), second pass (n1, NTRIALS - n1); the device may
  // widen the first pass to all step lengths (first_width)
  {
    const int n1 = first_width(only_more ? tr0 : ntr, d, cur, wide_max);
    tr0 = only_more ? n1 : 0;
    ntr = only_more ? NTRIALS - n1 : n1;
    if (ntr == 0) return;
    // the layout of this pass (same decision in both instantiations)
    if (((long)d.acnt[cur] * ntr <= (long)row_max) != ROW) return;
  }
  const long blk = xcd_block(blockIdx.x, ((long)d.acnt[cur] * ntr * GL + 63) / 64);
  const long gid = (blk * (long)blockDim.x + threadIdx.x) / GL;
  const int li = g8_lane();
  const bool J = li < NQ;
  const int ji = J ? li : 0;
  const bool real = !ROW || (threadIdx.x & 8) == 0;  // ROW: lanes 8..15 of a row are the phantom group
  const bool Js = J && real;                          // stores
  const int slot = (int)(gid / ntr), tr = tr0 + (int)(gid % ntr);
  __shared__ LaneK LKs[ROW ? 16 : G8];
  lane_consts_fill(C, LKs, (int)threadIdx.x);
  if (ROW) lane_consts_fill_phantom(C, LKs, (int)threadIdx.x);
  __syncthreads();
  const LaneK& K = LKs[ROW ? (threadIdx.x & 15) : li];
  const unsigned fl = ls_flags(C);
  const ActiveList al = active_list(d, cur);
  if (slot >= al.n) return;
  const int b = al.list[slot];
  const InstState* st = d.st + b;
  if (st->done) return;
  if (only_more) {
    // second pass of the line search: only instances none of whose first
    // tr0 trials was accepted (the first pass's results are complete: same stream)
    const InstState sv = *st;
    TrialRes T;
    load_trials(d, b, tr0, T);
    bool any = false;
    // constant trip count: T stays in registers (a runtime bound indexes
    // it dynamically, i.e. through scratch memory)
#pragma unroll
    for (int t2 = 0; t2 < NTRIALS; ++t2) any = any || (t2 < tr0 && trial_accepted(C, sv, T, t2));
    if (any) return;
  }
#ifdef FFDDP_PHASE_PROF
  const bool pp_on = (b == 0 && tr == 0);
#endif
  PP_INIT();
  const double alpha = C.alphas[tr];
  const bool feas = st->is_feasible != 0;
  const bool gap = !(feas || alpha == 1.0);
  const bool surf = surface[b] != 0;
  const double* xreg = inst_ref + (long)b * 21;
  const double xq = xreg[ji], xv = xreg[7 + ji], tref = xreg[14 + ji];
  // FF: y reference (= y0) of this lane's joint, loaded once
  double yq = 0.0, yv = 0.0, yt = 0.0;
  if (FF) {
    yq = x0[(long)b * nx + ji];
    yv = x0[(long)b * nx + 7 + ji];
    yt = x0[(long)b * nx + 14 + ji];
  }
  // predicted state (lane-local joint components)
  double hq = J ? x0[(long)b * nx + ji] : 0.0;
  double hv = J ? x0[(long)b * nx + 7 + ji] : 0.0;
  double ht = (FF && J) ? x0[(long)b * nx + 14 + ji] : 0.0;
  double cost = 0.0, dvp = 0.0;
  bool fail = false, fail_l = false;
  double* xtr = d.xs_try + ((long)b * NTRIALS + tr) * (N + 1) * nx;
  double* utr = d.us_try + ((long)b * NTRIALS + tr) * N * NU;
  // node inputs of the rollout, prefetched one node ahead (joint lane ji)
  constexpr int NCX = FF ? 3 : 2;  // state components per joint lane
  double pxs[3] = {0, 0, 0}, pfs[3] = {0, 0, 0}, pw[3] = {0, 0, 0}, pK[21], pus = 0.0, pk = 0.0, pref[6];
  double pfr = 0.0;
  LsW W;
  if constexpr (CW) {
    const double* cwr = d.cw + (long)b * FFDDP_COST_W + (J ? FFDDP_CW_JOINT0 : 0);
#pragma unroll
    for (int k = 0; k < LS_CW; ++k) W.w[k] = cwr[k];
  }
  LsL L;
  if constexpr (UL) {
    // a term the handle does not build never reads its entry
    const double* ulr = d.ul + (long)b * FFDDP_TAU_LIM_W + 4 * (J ? li : NQ - 1);
    L.uub = (fl & RF_BOX) ? ulr[0] : 0.0;
    L.tsub = (fl & RF_TSOFT) ? ulr[1] : 0.0;
    L.wslim = (FF && C.w_ws > 0.0) ? ulr[2] : K.wslim;
  }
  LsM M;
  if constexpr (MD) {
    // the EE lane and the phantom group: exact zeros (the unmasked suffix sums rely on it)
    const bool lnk = J && real;
    const double* mdr = d.md + (long)b * FFDDP_LINK_W + 16 * ji;
    M.m = lnk ? mdr[0] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) M.com[k] = lnk ? mdr[1 + k] : 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) M.I[k] = lnk ? mdr[4 + k] : 0.0;
  }
  LsT Tm;
  if constexpr (MT) {
    const double* mtr = d.mt + (long)b * FFDDP_MOUNT_W;
    const bool base = li == 0;  // the real group's joint 0 and (ROW) the phantom group's
#pragma unroll
    for (int k = 0; k < 9; ++k) Tm.R[k] = base ? mtr[k] : K.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Tm.p[k] = base ? mtr[9 + k] : K.p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Tm.g[k] = mtr[12 + k];
  }
  // FF augmentation weights (joint lanes) at their use: a term the handle does not build keeps C's zero
  auto w_y = [&]() { return (CW && C.w_y > 0.0) ? W.w[FFDDP_CW_Y - FFDDP_CW_JOINT0] : C.w_y; };
  auto w_w = [&]() { return (CW && C.w_w > 0.0) ? W.w[FFDDP_CW_W - FFDDP_CW_JOINT0] : C.w_w; };
  auto w_ws = [&]() { return (CW && C.w_ws > 0.0) ? W.w[FFDDP_CW_W_SOFT_LIMITS - FFDDP_CW_JOINT0] : C.w_ws; };
  auto fetch = [&](int t) {
    const long nb = (long)b * (N + 1) + t;
#pragma unroll
    for (int c = 0; c < 6; ++c) pref[c] = node_ref[nb * 6 + c];
    if constexpr (FR) pfr = d.fref[nb];
#pragma unroll
    for (int c = 0; c < NCX; ++c) {
      pxs[c] = J ? d.xs[nb * nx + 7 * c + ji] : 0.0;
      pfs[c] = (J && gap) ? d.fs[nb * nx + 7 * c + ji] : 0.0;
      pw[c] = (J && !feas) ? d.w[nb * nx + 7 * c + ji] : 0.0;
    }
    if (t < N) {
      const long ub = (long)b * N + t;
      pus = J ? d.us[ub * NU + ji] : 0.0;
      pk = J ? d.k[ub * NU + ji] : 0.0;
      const double* K_t = d.K + ub * NU * nx + (long)ji * nx;
#pragma unroll
      for (int m = 0; m < nx; ++m) pK[m] = J ? K_t[m] : 0.0;
    }
  };
  fetch(0);
  for (int t = 0; t <= N; ++t) {
    double xq_t = hq, xv_t = hv, xt_t = ht;
    const double sq = pxs[0], sv = pxs[1], stt = pxs[2];
    if (gap) {
      xq_t = fma(pfs[0], alpha - 1.0, hq);
      xv_t = fma(pfs[1], alpha - 1.0, hv);
      if (FF) xt_t = fma(pfs[2], alpha - 1.0, ht);
    }
    if (!feas) {
      dvp = fma(-pw[0], sq - xq_t, dvp);
      dvp = fma(-pw[1], sv - xv_t, dvp);
      if (FF) dvp = fma(-pw[2], stt - xt_t, dvp);
    }
    if (Js) {
      xtr[(long)t * nx + ji] = xq_t;
      xtr[(long)t * nx + 7 + ji] = xv_t;
      if (FF) xtr[(long)t * nx + 14 + ji] = xt_t;
    }
    double ref[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) ref[c] = pref[c];
    const double fnr = pfr;
    if (t < N) {
      // u_i = us_i - alpha k_i - K_i (x - xs)  (crocoddyl order: x components q, v, tau)
      double u = 0.0;
      {
        double acc = fma(-pk, alpha, pus);
        const double dq = xq_t - sq, dv = xv_t - sv, dtt = xt_t - stt;
#pragma unroll
        for (int m = 0; m < NQ; ++m) {
          const double dqm = ls_get<ROW>(dq, m), dvm = ls_get<ROW>(dv, m);
          acc = fma(-pK[m], dqm, acc);
          acc = fma(-pK[7 + m], dvm, acc);
          if (FF) acc = fma(-pK[14 + m], ls_get<ROW>(dtt, m), acc);
        }
        if (fl & RF_BOX) acc = UL ? fmin(fmax(acc, -L.uub), L.uub) : fmin(fmax(acc, K.ulb), K.uub);
        u = acc;
        if (Js) utr[(long)t * NU + ji] = u;
      }
      fetch(t + 1);
      double qn, vn, cp, lam[3];
      const double uin = FF ? xt_t : u;
      PP(8);
      ls_node_calc<NC, ROW, FR, CW, UL, MD, MT>(C, fl, K, W, L, M, Tm, MODE_RUNNING, surf, xq_t, xv_t, uin, xq, xv, tref, ref, fnr, qn, vn, cp, lam
#ifdef FFDDP_PHASE_PROF
                            , pp_acc, pp_last
#endif
      );
      double c = C.dt * cp;
      double tn = 0.0;
      if (FF) {
        tn = fma(C.beta, u, C.alpha * xt_t);
        if (J) {
          const double e1 = xq_t - yq, e2 = xv_t - yv, e3 = xt_t - yt;
          c = fma(0.5 * w_y(), fma(K.wy2t * e3, e3, fma(K.wy2v * e2, e2, (K.wy2q * e1) * e1)), c);
          c = fma(0.5 * w_w(), u * u, c);
          const double ov = fabs(u) - (UL ? L.wslim : K.wslim);
          const double oo = ov > 0.0 ? ov : 0.0;
          c = fma(w_ws(), 0.5 * (oo * oo), c);
        }
      }
      cost += g8_sum(c);
      // a non-finite or huge state or cost fails the trial (forwardPass's
      // raiseIfNaN); the test is lane-local here and reduced once after the
      // last node, so no cross-lane reduction or branch sits on each node's
      // chain.  A failed trial's remaining nodes run on garbage whose results
      // nothing reads (its cost and trajectory are never accepted), and a bad
      // cost stays bad to the end
      fail_l = fail_l || (J && (bad(fabs(qn)) || bad(fabs(vn)) || (FF && bad(fabs(tn)))));
      hq = qn;
      hv = vn;
      ht = tn;
    } else {
      double qn, vn, cp, lam[3];
      const int mode = FF ? MODE_TERMINAL_U : MODE_TERMINAL_X;
      PP(8);
      ls_node_calc<NC, ROW, FR, CW, UL, MD, MT>(C, fl, K, W, L, M, Tm, mode, surf, xq_t, xv_t, FF ? xt_t : 0.0, xq, xv, tref, ref, fnr, qn, vn, cp, lam
#ifdef FFDDP_PHASE_PROF
                            , pp_acc, pp_last
#endif
      );
      double c = FF ? C.dt * cp : cp;
      if (FF && J) {
        const double e1 = xq_t - yq, e2 = xv_t - yv, e3 = xt_t - yt;
        c = fma(0.5 * w_y(), fma(K.wy2t * e3, e3, fma(K.wy2v * e2, e2, (K.wy2q * e1) * e1)), c);
      }
      cost += g8_sum(c);
    }
  }
  {
    int f = (bad(cost) || g8_or(fail_l ? 1 : 0)) ? 1 : 0;
    if (ROW) f = ls_row_bcast0(f);  // the phantom group follows the real one
    fail = f != 0;
  }
  PP(9);
  PP_FLUSH_AT(16);
  const double dv = g8_sum(dvp);
  if (li == 0 && real) {
    d.trial[((long)b * NTRIALS + tr) * 2 + 0] = cost;
    d.trial[((long)b * NTRIALS + tr) * 2 + 1] = dv;
    d.trial_fail[(long)b * NTRIALS + tr] = fail ? 1 : 0;
  }
}
#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------
// acceptance / regularisation / stopping: one lane per instance
// ---------------------------------------------------------------------------
// SolverFDDP::solve after the line search for instance b: first accepted step
// length, regularisation update, stopping test.  Returns the accepted trial
// (-1: none, or the instance is done).
__device__ int accept_instance(const DevConsts& C, Dev& d, int b, int iter, int n1) {
  InstState s = d.st[b];
  TrialRes T;  // issued with the state load (unused for a done instance)
  load_trials(d, b, NTRIALS, T);
  if (s.done) {
    d.st[b].accepted = -1;
    return -1;
  }
  s.iter = iter;
  int acc = -1;
  double steplength = C.alphas[NTRIALS - 1];
  int tried = NTRIALS;
  // dV, dVexp, d1 of the accepted (else the last finite) trial, for the trace
  double tdV = __builtin_nan(""), tdVexp = __builtin_nan(""), td1 = __builtin_nan("");
  for (int tr = 0; tr < NTRIALS; ++tr) {
    const double a = C.alphas[tr];
    const double cost_try = T.cost[tr];
    double e0 = tdV, e1 = tdVexp, e2 = td1;
    const bool okt = trial_accepted(C, s, T, tr, &e0, &e1, &e2);
    tdV = e0;
    tdVexp = e1;
    td1 = e2;
    if (!T.fail[tr] && e1 < 0) {
      s.n_neg += 1;
      s.n_neg_acc += okt ? 1 : 0;
    }
    if (okt) {
      acc = tr;
      steplength = a;
      tried = tr + 1;
      s.was_feasible = s.is_feasible;
      s.is_feasible = (s.was_feasible || a == 1.0) ? 1 : 0;
      s.cost = cost_try;
      s.recalc = 1;
      break;
    }
  }
  if (acc < 0) s.recalc = 0;  // (xs, us) unchanged: node data stays valid
  // step lengths the line-search kernels evaluated (first pass: n1; second
  // pass: the rest, only when none of the first n1 was accepted)
  s.n_eval1 += n1;
  const bool second = n1 < NTRIALS && (acc < 0 || acc >= n1);  // the second pass evaluated this instance
  if (second) s.n_eval2 += NTRIALS - n1;
  s.n_trials += tried;
  s.n_forward += second ? 2 : 1;  // line-search launches that processed it
  s.accepted = acc;
  if (steplength > C.th_stepdec) s.preg = fmax(s.preg / C.reg_dec, C.reg_min);
  if (steplength <= C.th_stepinc) {
    s.preg = fmin(s.preg * C.reg_inc, C.reg_max);
    if (s.preg == C.reg_max) {
      s.done = 1;
      s.ok = 0;
    }
  }
  // CallbackVerbose record of this iteration (before the stopping test, as
  // the callbacks run in SolverFDDP::solve; none when preg reached reg_max)
  if (d.trace && iter < d.trace_it && !s.done) {
    double* r = d.trace + ((long)b * d.trace_it + iter) * FFDDP_TRACE_W;
    r[0] = (double)iter;
    r[1] = s.cost;
    r[2] = s.stop;
    r[3] = -td1;
    r[4] = s.preg;
    r[5] = s.preg;
    r[6] = steplength;
    r[7] = s.ffeas;
    r[8] = tdV;
    r[9] = tdVexp;
  }
  if (!s.done && s.was_feasible && s.stop < C.th_stop) {
    s.done = 1;
    s.ok = 1;
  }
  d.st[b] = s;
  return acc;
}

// acceptance / regularisation / stopping, one lane per instance; the
// continuing instances are appended to the next active list with one atomic
// per wave.  The accepted trial is not copied here: the next iteration's
// k_node reads it in place and writes it into (xs, us) node by node, and
// k_commit does it for the instances no further k_node visits.
__global__ __launch_bounds__(64) void k_accept(const DevConsts* __restrict__ Cg, Dev d, int iter, int n1, int cur,
                                               int wide_max) {
  const DevConsts& C = *Cg;
  const ActiveList al = active_list(d, cur);
  const int n1h = n1;
  n1 = first_width(n1, d, cur, wide_max);
  if ((int)blockIdx.x * 64 >= al.n) return;
  const int slot = (int)blockIdx.x * 64 + (int)threadIdx.x;
  const bool has = slot < al.n;
  const int b = has ? al.list[slot] : 0;
  bool cont = false;
  int acc = -1;
  if (has) {
    acc = accept_instance(C, d, b, iter, n1);
    cont = d.st[b].done == 0;
  }
  // a continuing instance needed more step lengths than the host's first pass:
  // the next iteration's first pass may take them all (first_width)
  if (cont && (acc < 0 || acc >= n1h)) d.acnt[2 + (cur ^ 1)] = 1;
  const unsigned long long m = __ballot(cont);
  int base = 0;
  if (threadIdx.x == 0 && m != 0ull) base = atomicAdd(d.acnt + (cur ^ 1), __popcll(m));
  base = __builtin_amdgcn_readfirstlane(base);
  if (cont) d.alist[(long)(cur ^ 1) * d.B + base + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = b;
}

// end of solve: the accepted trial of every instance whose last iteration
// accepted one and that no k_node visited since becomes (xs, us); 16 lanes
// per instance, a chunk's loads all in flight before its stores
constexpr int COMMIT_IPB = 4;
__global__ __launch_bounds__(64) void k_commit(const DevConsts* __restrict__ Cg, Dev d) {
  const DevConsts& C = *Cg;
  const int q = threadIdx.x / 16, l = threadIdx.x % 16;
  const int b = (int)blockIdx.x * COMMIT_IPB + q;
  if (b >= d.B) return;
  const int acc = d.st[b].accepted;
  if (acc < 0) return;
  const int N = C.N, nx = C.nx;
  const long perX = (long)(N + 1) * nx, perU = (long)N * NU;
  const double* sx = d.xs_try + ((long)b * NTRIALS + acc) * perX;
  const double* su = d.us_try + ((long)b * NTRIALS + acc) * perU;
  double* dx = d.xs + (long)b * perX;
  double* du = d.us + (long)b * perU;
  constexpr int CH = 16;
  for (long base = l; base < perX + perU; base += 16 * CH) {
    double v[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const long i = base + 16 * u;
      v[u] = i < perX ? sx[i] : (i < perX + perU ? su[i - perX] : 0.0);
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const long i = base + 16 * u;
      if (i < perX)
        dx[i] = v[u];
      else if (i < perX + perU)
        du[i - perX] = v[u];
    }
  }
}

// solution read-back helpers: iter/ok, contact force at knots 0 and 1
// MD: the predicted contact force is computed under the instance's own link model, its row d.md[b] (a solve with
// link_rows), which rb_pass reads in place of C.rb's inertial parameters; MD = false is the kernel as it was.
// MT: and under its own base placement and gravity, its row d.mt[b] (a solve with mount_rows), which rb_pass reads
// likewise; instantiated with MD only.
template <int NC, bool FF, bool MD = false, bool MT = false>
__global__ __launch_bounds__(64) void k_finalize(const DevConsts* __restrict__ Cg, Dev d, int maxiter, const double* __restrict__ x0,
                           const double* __restrict__ node_ref, const double* __restrict__ inst_ref,
                           const uint8_t* __restrict__ surface, double* cost, int32_t* iters, uint8_t* ok,
                           double* fn_pred, int32_t* stats, const uint8_t* __restrict__ active) {
  const DevConsts& C = *Cg;
  const int N = C.N;
  constexpr int nx = FF ? 21 : 14;
  const long gid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int b = (int)(gid / 2), knot = (int)(gid % 2);
  if (b >= d.B) return;
  if (active && active[b] == 0) return;  // not selected: its output rows stay as they are
  const InstState s = d.st[b];
  if (knot == 0) {
    cost[b] = s.cost;
    iters[b] = s.done ? s.iter : maxiter;
    ok[b] = (s.done && s.ok) ? 1 : 0;
    if (stats) {
      stats[(long)b * FFDDP_NSTATS + 0] = s.n_iters;
      stats[(long)b * FFDDP_NSTATS + 1] = s.n_trials;
      stats[(long)b * FFDDP_NSTATS + 2] = s.n_retries;
      stats[(long)b * FFDDP_NSTATS + 3] = s.n_backward;
      stats[(long)b * FFDDP_NSTATS + 4] = s.n_calc;
      stats[(long)b * FFDDP_NSTATS + 5] = s.n_forward;
      stats[(long)b * FFDDP_NSTATS + 6] = s.n_eval1;
      stats[(long)b * FFDDP_NSTATS + 7] = s.n_eval2;
      stats[(long)b * FFDDP_NSTATS + 8] = s.n_neg;
      stats[(long)b * FFDDP_NSTATS + 9] = s.n_neg_acc;
    }
  }
  if (fn_pred == nullptr) return;
  const int t = knot < N ? knot : N - 1;
  if (!surface[b]) {
    fn_pred[(long)b * 2 + knot] = __builtin_nan("");
    return;
  }
  const double* y = d.xs + ((long)b * (N + 1) + t) * nx;
  const double* u = d.us + ((long)b * N + t) * NU;
  const double* ref = node_ref + ((long)b * (N + 1) + t) * 6;
  const double* xreg = inst_ref + (long)b * 21;
  Primal P;
  double yn[21], c;
  if constexpr (MT) {
    node_calc<NC, FF, true>(C, false, true, y, u, ref, xreg, xreg + 14, x0 + (long)b * nx, P, yn, c, nullptr,
                      d.md + (long)b * FFDDP_LINK_W, d.mt + (long)b * FFDDP_MOUNT_W);
  } else if constexpr (MD) {
    node_calc<NC, FF>(C, false, true, y, u, ref, xreg, xreg + 14, x0 + (long)b * nx, P, yn, c, nullptr,
                      d.md + (long)b * FFDDP_LINK_W);
  } else {
    node_calc<NC, FF>(C, false, true, y, u, ref, xreg, xreg + 14, x0 + (long)b * nx, P, yn, c);
  }
  fn_pred[(long)b * 2 + knot] = (NC == 1) ? P.lam[0] : P.lam[2];
}

// A lane's physics row (ffddp_plant_set_instance_params) over a copy of the handle's struct: rows is field-major
// [FFDDP_PLANT_ROW_W][ld], so the wave's loads of one field are consecutive doubles.
__device__ __forceinline__ void plant_load_row(ffddp_plant_params& P, int b, const double* __restrict__ rows, long ld) {
  const double* r = rows + b;
  for (int i = 0; i < NQ; ++i) {
    P.armature[i] = r[(FFDDP_PLANT_ROW_ARMATURE + i) * ld];
    P.damping[i] = r[(FFDDP_PLANT_ROW_DAMPING + i) * ld];
  }
  P.r_tool = r[FFDDP_PLANT_ROW_R_TOOL * ld];
  P.margin = r[FFDDP_PLANT_ROW_MARGIN * ld];
  for (int i = 0; i < 2; ++i) P.solref[i] = r[(FFDDP_PLANT_ROW_SOLREF + i) * ld];
  for (int i = 0; i < 5; ++i) P.solimp[i] = r[(FFDDP_PLANT_ROW_SOLIMP + i) * ld];
}

// The handle's device copy of the link-model rows (ffddp_plant_set_instance_links): field-major over the
// PLANT_LINK_USED entries a row holds apart from padding, [PLANT_LINK_USED][ld], field 13 j + k being the row's
// entry 16 j + k, so the wave's loads of one field are consecutive doubles.
constexpr int PLANT_LINK_PER_JOINT = 13;                   // mass, com (3), inertia (9)
constexpr int PLANT_LINK_USED = NQ * PLANT_LINK_PER_JOINT;  // 91
constexpr int PLANT_LINK_LOCAL = 16 * (NQ - 1) + PLANT_LINK_PER_JOINT;  // a lane's row up to its last used entry
struct PlantLinks {
  const double* rows;
  long ld;
};

// A lane's link-model row in rb_pass's 16 j + k indexing; the padding entries of L are neither written nor read.
__device__ __forceinline__ void plant_load_links(double* L, int b, PlantLinks lk) {
  const double* __restrict__ r = lk.rows + b;
#pragma unroll
  for (int j = 0; j < NQ; ++j)
#pragma unroll
    for (int k = 0; k < PLANT_LINK_PER_JOINT; ++k) L[16 * j + k] = r[(PLANT_LINK_PER_JOINT * j + k) * lk.ld];
}
__device__ __forceinline__ PlantLinks plant_links_of(PlantLinks lk) { return lk; }
__device__ __forceinline__ PlantLinks plant_links_of(const double*, long, PlantLinks lk) { return lk; }
__device__ __forceinline__ void plant_load_row(ffddp_plant_params& P, int b, const double* __restrict__ rows, long ld,
                                               PlantLinks) {
  plant_load_row(P, b, rows, ld);
}

// closed-loop plant stand-in: one thread per instance (ffddp_plant.hpp).  k_plant<false>: every lane steps with
// the handle's struct; k_plant<true, const double*, long>: the trailing arguments are (rows, ld) and the lane
// steps with its own row.  The pack keeps the first instantiation's arguments, and so its code, what they were.
// A PlantLinks at the end of the pack (k_plant<false, PlantLinks>, k_plant<true, const double*, long, PlantLinks>):
// the lane integrates with its own link-model row, loaded once before the substep loop, in place of rb's masses,
// centres of mass and inertias.
template <bool ROWS, class... RowArgs>
__global__ __launch_bounds__(64) void k_plant(const ffddp_robot* __restrict__ rb, const ffddp_plant_params* __restrict__ pp,
                                              int B, double* __restrict__ q, double* __restrict__ v,
                                              const double* __restrict__ tau, const double* __restrict__ plane,
                                              int integrate, double* __restrict__ obs, int32_t* __restrict__ fail,
                                              RowArgs... row_args) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double qb[NQ], vb[NQ], tb[NQ], ob[PO_WORDS];
  for (int i = 0; i < NQ; ++i) {
    qb[i] = q[(long)b * NQ + i];
    vb[i] = v[(long)b * NQ + i];
    tb[i] = tau[(long)b * NQ + i];
  }
  const double* pl = plane + (long)b * 6;
  bool ok;
  if constexpr ((std::is_same_v<RowArgs, PlantLinks> || ...)) {
    double L[PLANT_LINK_LOCAL];
    plant_load_links(L, b, plant_links_of(row_args...));
    if constexpr (ROWS) {
      ffddp_plant_params P = *pp;
      plant_load_row(P, b, row_args...);
      ok = plant_step(*rb, P, qb, vb, tb, pl, pl + 3, integrate, ob, L);
    } else {
      ok = plant_step(*rb, *pp, qb, vb, tb, pl, pl + 3, integrate, ob, L);
    }
  } else if constexpr (ROWS) {
    ffddp_plant_params P = *pp;  // timestep, n_substeps and site_R stay the handle's
    plant_load_row(P, b, row_args...);
    ok = plant_step(*rb, P, qb, vb, tb, pl, pl + 3, integrate, ob);
  } else {
    ok = plant_step(*rb, *pp, qb, vb, tb, pl, pl + 3, integrate, ob);
  }
  for (int i = 0; i < NQ; ++i) {
    q[(long)b * NQ + i] = qb[i];
    v[(long)b * NQ + i] = vb[i];
  }
  for (int e = 0; e < PO_WORDS; ++e) obs[(long)b * PO_WORDS + e] = ob[e];
  if (fail) fail[b] = ok ? 0 : 1;
}

__global__ __launch_bounds__(64) void k_gravity(const ffddp_robot* __restrict__ rb, int B, const double* __restrict__ q,
                          double* __restrict__ tau) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  gravity_torque(*rb, q + (long)b * NQ, tau + (long)b * NQ);
}

// ffddp_gravity_torque_mdl_dev: k_gravity with each instance's own link-model row
__global__ __launch_bounds__(64) void k_gravity_mdl(const ffddp_robot* __restrict__ rb, int B, const double* __restrict__ q,
                                                    const double* __restrict__ link, double* __restrict__ tau) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  gravity_torque(*rb, q + (long)b * NQ, tau + (long)b * NQ, link + (long)b * FFDDP_LINK_W);
}

// ffddp_gravity_torque_mnt_dev: k_gravity with each instance's own mount row and, unless null, link-model row
__global__ __launch_bounds__(64) void k_gravity_mnt(const ffddp_robot* __restrict__ rb, int B, const double* __restrict__ q,
                                                    const double* __restrict__ link, const double* __restrict__ mount,
                                                    double* __restrict__ tau) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  gravity_torque<true>(*rb, q + (long)b * NQ, tau + (long)b * NQ, link ? link + (long)b * FFDDP_LINK_W : nullptr,
                       mount + (long)b * FFDDP_MOUNT_W);
}

// ffddp_fleet_obs_frame_dev: one lane per instance re-expresses its plant record (ffddp_plant.hpp PO_*) in the
// instance's planning frame (R, p in the MuJoCo world, frame row [FFDDP_FRAME_W]: R row-major, then p).  All PO_WORDS
// words are copied; positions become R^T (x - p), free vectors R^T x, the EE rotation and the site Jacobian R^T X
// column by column.  Each entry is (R[0][i] x0 + R[1][i] x1) + R[2][i] x2, evaluated left to right without
// contraction, so a restatement in numpy gives the same bits.  sel[b] == 0: the record is copied verbatim.
__global__ __launch_bounds__(64) void k_fleet_obs_frame(int B, const double* __restrict__ obs, long ld_obs,
                                                        const double* __restrict__ frame,
                                                        const uint8_t* __restrict__ sel, double* __restrict__ out,
                                                        long ld_out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* in = obs + (long)b * ld_obs;
  double* o = out + (long)b * ld_out;
  if (sel && !sel[b]) {
    for (int i = 0; i < PO_WORDS; ++i) o[i] = in[i];
    return;
  }
  double R[9], p[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = frame[(long)b * FFDDP_FRAME_W + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = frame[(long)b * FFDDP_FRAME_W + 9 + k];
  auto rt = [&](double x0, double x1, double x2, int i) { return (R[i] * x0 + R[3 + i] * x1) + R[6 + i] * x2; };
  for (int i = 0; i < PO_EE_P; ++i) o[i] = in[i];
  {
    const double d0 = in[PO_EE_P] - p[0], d1 = in[PO_EE_P + 1] - p[1], d2 = in[PO_EE_P + 2] - p[2];
    const double v0 = in[PO_EE_V], v1 = in[PO_EE_V + 1], v2 = in[PO_EE_V + 2];
    const double f0 = in[PO_FW], f1 = in[PO_FW + 1], f2 = in[PO_FW + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      o[PO_EE_P + i] = rt(d0, d1, d2, i);
      o[PO_EE_V + i] = rt(v0, v1, v2, i);
      o[PO_FW + i] = rt(f0, f1, f2, i);
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double x0 = in[PO_EE_R + j], x1 = in[PO_EE_R + 3 + j], x2 = in[PO_EE_R + 6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[PO_EE_R + 3 * i + j] = rt(x0, x1, x2, i);
  }
  o[PO_FN] = in[PO_FN];
  o[PO_NCON] = in[PO_NCON];
  for (int j = 0; j < NQ; ++j) {
    const double x0 = in[PO_J + j], x1 = in[PO_J + NQ + j], x2 = in[PO_J + 2 * NQ + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[PO_J + NQ * i + j] = rt(x0, x1, x2, i);
  }
}

// ---------------------------------------------------------------------------
// Problem builder (ffddp_build_problem_dev): one thread per (instance, knot).
// make_approach_then_circle (trajectories.py:8-93) + the benchmark hold
// (run_classical.py:256-264), MuJoCo -> Pinocchio (crocoddyl_classical.py:
// 250-258, R_MJ_FROM_PIN = diag(-1,-1,1)), references (:447-466).
// ---------------------------------------------------------------------------
struct TaskTraj {
  double center[3], radius, omega, z_contact, t_approach, t_pre, t_hold;
  double p_start[3], p_pre[3], p_cs[3];
};

__device__ __forceinline__ double smoothstep01(double s) {
  s = fmin(fmax(s, 0.0), 1.0);
  return s * s * (3.0 - 2.0 * s);
}

__device__ __forceinline__ double dsmoothstep01(double s) {
  s = fmin(fmax(s, 0.0), 1.0);
  return 6.0 * s * (1.0 - s);
}

// base(t) -> (p, v, surface) in the MuJoCo world
__device__ bool task_base(const TaskTraj& T, double t, double p[3], double v[3]) {
  const double* p0;
  const double* p1;
  double tau, dur;
  if (T.t_pre > 0.0 && t < T.t_pre) {
    p0 = T.p_start; p1 = T.p_pre; tau = t; dur = T.t_pre;
  } else if (t < T.t_pre + T.t_approach) {
    p0 = T.t_pre > 0.0 ? T.p_pre : T.p_start; p1 = T.p_cs; tau = t - T.t_pre; dur = T.t_approach;
  } else {
    const double th = T.omega * (t - (T.t_pre + T.t_approach));
    double sn, cs;
    sincos(th, &sn, &cs);
    p[0] = T.center[0] + T.radius * cs;
    p[1] = T.center[1] + T.radius * sn;
    p[2] = T.z_contact;
    v[0] = -T.radius * T.omega * sn;
    v[1] = T.radius * T.omega * cs;
    v[2] = 0.0;
    return true;
  }
  const double sl = tau / dur, s = smoothstep01(sl), dsdt = dsmoothstep01(sl) / dur;
  for (int i = 0; i < 3; ++i) {
    p[i] = (1.0 - s) * p0[i] + s * p1[i];
    v[i] = dsdt * (p1[i] - p0[i]);
  }
  return false;
}

__device__ bool task_eval(const TaskTraj& T, double t, double p[3], double v[3]) {
  const bool surf = task_base(T, t, p, v);
  const double tc = T.t_pre + T.t_approach;
  if (surf && t < tc + T.t_hold) {
    double vh[3];
    task_base(T, tc, p, vh);
    v[0] = v[1] = v[2] = 0.0;
  }
  return surf;
}

__global__ __launch_bounds__(64) void k_build(const ffddp_robot* __restrict__ rb, TaskTraj T, ffddp_task task, int B,
                                              int N, int nx, double dt, const double* __restrict__ t0,
                                              const double* __restrict__ x0, double* __restrict__ node_ref,
                                              double* __restrict__ inst_ref, uint8_t* __restrict__ surface) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long)B * (N + 1)) return;
  const int b = (int)(g / (N + 1)), k = (int)(g - (long)b * (N + 1));
  double p[3], v[3];
  task_eval(T, t0[b] + k * dt, p, v);
  double* o = node_ref + g * 6;
  o[0] = -p[0] - task.p_site_minus_frame[0];
  o[1] = -p[1] - task.p_site_minus_frame[1];
  o[2] = p[2] - task.p_site_minus_frame[2];
  o[3] = -v[0];
  o[4] = -v[1];
  o[5] = v[2];
  if (k != 0) return;
  double pp[3], vv[3];
  surface[b] = task_eval(T, t0[b], pp, vv) ? 1 : 0;
  const double* xb = x0 + (long)b * nx;
  double* ir = inst_ref + (long)b * 21;
  for (int i = 0; i < 7; ++i) {
    ir[i] = task.posture_mode ? task.q_nom[i] : xb[i];
    ir[7 + i] = task.posture_mode ? 0.0 : xb[7 + i];
  }
  if (task.torque_mode == 2) {
    for (int i = 0; i < 7; ++i) ir[14 + i] = 0.0;
  } else {
    gravity_torque(*rb, task.torque_mode == 1 ? task.q_nom : xb, ir + 14);
  }
}

// ---------------------------------------------------------------------------
// Fleet tick glue (ffddp_fleet_warm_start_dev / ffddp_fleet_keep_dev): pure
// data movement around the solve of a receding-horizon fleet.  An instance's
// arrays are contiguous blocks, indexed flat, so lanes touch consecutive
// doubles (8-byte accesses: with nx = 21 an instance's base is only 8-byte
// aligned).  Grid (B, FLEET_CHUNKS): the blocks of one instance stride over
// its flat index together, so valid[b] / fin are uniform in every wave.
// ---------------------------------------------------------------------------
constexpr int FLEET_BLOCK = 256;
constexpr int FLEET_CHUNKS = 4;

// _shift_guess (crocoddyl_classical.py:733-757): xs_init = [x0] + keep_xs[1:],
// us_init = keep_us[1:] + [keep_us[-1]]; cold: [x0] * (N+1), [u_cold] * N
__global__ __launch_bounds__(FLEET_BLOCK) void k_fleet_warm_start(
    int N, int nx, const double* __restrict__ x0, const double* __restrict__ u_cold,
    const uint8_t* __restrict__ valid, const double* __restrict__ keep_xs, const double* __restrict__ keep_us,
    double* __restrict__ xs_init, double* __restrict__ us_init) {
  const long b = blockIdx.x;
  const int t0 = blockIdx.y * FLEET_BLOCK + threadIdx.x, step = FLEET_CHUNKS * FLEET_BLOCK;
  const bool warm = valid[b] != 0;
  const int nxs = (N + 1) * nx, nus = N * NU;
  const double* xb = x0 + b * nx;
  const double* kx = keep_xs + b * nxs;
  double* xo = xs_init + b * nxs;
  for (int i = t0; i < nxs; i += step) xo[i] = (warm && i >= nx) ? kx[i] : xb[i % nx];
  const double* ub = u_cold + b * NU;
  const double* ku = keep_us + b * nus;
  double* uo = us_init + b * nus;
  // knot min(k+1, N-1) of keep_us, flat: i + 7 except in the last knot
  for (int i = t0; i < nus; i += step) uo[i] = warm ? ku[i + NU < nus ? i + NU : i] : ub[i % NU];
}

// keep the new solution iff its us[0] is finite (crocoddyl_classical.py:378-384),
// then pack the first-knot record from the kept arrays (layout: include/ffddp.h)
__global__ __launch_bounds__(FLEET_BLOCK) void k_fleet_keep(
    int N, int nx, const double* __restrict__ xs, const double* __restrict__ us, const double* __restrict__ K,
    const double* __restrict__ cost, const int32_t* __restrict__ iters, const uint8_t* __restrict__ ok,
    const double* __restrict__ fn_pred, const int32_t* __restrict__ stats, double* __restrict__ keep_xs,
    double* __restrict__ keep_us, double* __restrict__ keep_K, double* __restrict__ first) {
  const long b = blockIdx.x;
  const int t0 = blockIdx.y * FLEET_BLOCK + threadIdx.x, step = FLEET_CHUNKS * FLEET_BLOCK;
  const long nxs = (long)(N + 1) * nx, nus = (long)N * NU, nK = (long)N * NU * nx;
  const double *xn = xs + b * nxs, *un = us + b * nus, *Kn = K + b * nK;
  double *xk = keep_xs + b * nxs, *uk = keep_us + b * nus, *Kk = keep_K + b * nK;
  // fin: every wave tests the seven entries of us[b][0] itself (lanes 0-6, one ballot)
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(lane < NU ? (isfinite(un[lane]) ? 1 : 0) : 1);
  const bool fin = m == ~0ull;
  if (fin) {
    for (int i = t0; i < nxs; i += step) xk[i] = xn[i];
    for (int i = t0; i < nus; i += step) uk[i] = un[i];
    for (int i = t0; i < nK; i += step) Kk[i] = Kn[i];
  }
  if (blockIdx.y != 0) return;
  // the record comes from the kept arrays; when fin those equal the new
  // solution, which is read here instead (the copy above is other waves' work)
  const double *xr = fin ? xn : xk, *ur = fin ? un : uk, *Kr = fin ? Kn : Kk;
  const int W = FFDDP_FLEET_FIRST_W(nx), oK = 8 + 2 * nx, oS = 8 + 9 * nx;
  double* f = first + b * W;
  for (int j = threadIdx.x; j < W; j += FLEET_BLOCK) {
    double val;
    if (j == 0) val = fin ? 1.0 : 0.0;
    else if (j < 8) val = ur[j - 1];
    else if (j < oK) val = xr[j - 8];  // knots 0 and 1 are adjacent
    else if (j < oS) val = Kr[j - oK];
    else if (j == oS) val = cost[b];
    else if (j == oS + 1) val = (double)iters[b];
    else if (j == oS + 2) val = (double)ok[b];
    else if (j == oS + 3) val = (double)stats[b * FFDDP_NSTATS + 9];
    else val = fn_pred[b * 2 + (j - oS - 4)];
    f[j] = val;
  }
}

// ---------------------------------------------------------------------------
// Fleet closed loop on the device (ffddp_fleet_pre_dev / ffddp_fleet_post_dev):
// what FleetClassicalMPC / FleetForceFeedbackMPC.compute_control do on the host
// around the solve, per instance, from the caller's device-resident state.
// ---------------------------------------------------------------------------

// Everything before the solve.  One block per instance: every wave derives the
// instance's decisions (latch, mode change, warm / cold) from the old state
// itself, so they are uniform; the state is rewritten by thread 0 after a
// barrier, which is why the instance is not split over several blocks as in
// k_fleet_warm_start (another block could read valid[b] after the rewrite).
//
// SCHED (ffddp_fleet_pre_sched_dev): the instance solves this tick (Q.need[b],
// the solve's `active`) iff it has no warm start or its period has run out.
// The kept solution is never moved between solves: Q.age[b] counts the
// receding-horizon shifts since it was kept (_rollout_shift, pure copying), so
// knot i of the shifted lists is knot min(i + age, N) of keep_xs and knot
// min(i + age, N - 1) of keep_us / keep_K.  Only solving instances get a warm
// start.  SCHED = false is ffddp_fleet_pre_dev's kernel, unchanged (Q unused).
//
// TASK (ffddp_fleet_pre_task_dev): the instance's references and hint come
// from its own record (ffddp_task.hpp) at the task time T.t - delay instead of
// node1 / hint1.  The flag is two comparisons, so every wave derives it with
// the rest of the old state; the knots are spread over the threads.  TASK =
// false compiles the code as it was (T, dt_ocp unused).
//
// link (ffddp_fleet_pre_mdl_dev): the gravity torque reference is computed with
// the instance's own mass / com / inertia, its link-model row; null: *rb's.
// mount (ffddp_fleet_pre_mnt_dev): and under the instance's own base placement
// and gravity, its mount row; null: *rb's.
template <bool SCHED, bool TASK>
__global__ __launch_bounds__(FLEET_BLOCK) void k_fleet_pre(
    const ffddp_robot* __restrict__ rb, int N, int nx, ffddp_fleet_params P, ffddp_fleet_state S, ffddp_fleet_sched Q,
    const double* __restrict__ q, const double* __restrict__ v, const double* __restrict__ fn_meas,
    const double* __restrict__ contact, const double* __restrict__ ee_z, long ld, long ld1,
    const double* __restrict__ tau_hat, long ld_th, const double* __restrict__ q_nom, const double* __restrict__ node1, int hint1,
    double* __restrict__ x0, uint8_t* __restrict__ surface, double* __restrict__ inst_ref,
    double* __restrict__ node_ref, double* __restrict__ xs_init, double* __restrict__ us_init, ffddp_fleet_tasks T,
    double dt_ocp, const double* __restrict__ link, const double* __restrict__ mount) {
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const bool ff = nx == 21;
  const double* rec = TASK ? T.rec + b * FFDDP_FLEET_TASK_W : nullptr;
  const double t_task = TASK ? T.t - rec[FFDDP_FLEET_TASK_DELAY] : 0.0;
  const int hint = TASK ? (fleet_task_surface(rec, t_task) ? 1 : 0) : hint1;
  const bool latched0 = S.latched[b] != 0, valid0 = S.valid[b] != 0;
  const int cnt0 = S.loss_count[b], pm = S.prev_mode[b];
  // _surface (fleet.py; crocoddyl_classical.py:286-303)
  bool latched = latched0, surf = hint != 0;
  int cnt = cnt0;
  if (P.phase_source == 1) {
    double fn = fn_meas[b * ld1];
    if (contact) fn = fn * (contact[b * ld1] > 0.5 ? 1.0 : 0.0);
    const double ez = ee_z[b * ld1];
    const bool near = isfinite(ez) && ez <= P.z_contact + P.z_contact_band;
    const bool lost = fn < P.fn_contact_off;
    const int c = latched0 ? (lost ? cnt0 + 1 : 0) : 0;
    const bool release = latched0 && c >= P.contact_release_steps;
    const bool engage = !latched0 && (fn > P.fn_contact_on || (hint != 0 && near));
    latched = (latched0 && !release) || engage;
    cnt = (release || engage) ? 0 : c;
    surf = latched;
  }
  // _phase: a mode switch drops the warm start
  const bool changed = pm >= 0 && (surf != (pm == 1));
  const bool warm = valid0 && !changed;
  // _need_solve (since / age are written by the post kernel only)
  const bool need = !SCHED || !warm || Q.since[b] + 1 >= Q.period;
  const int age = SCHED ? (Q.age[b] < N ? Q.age[b] : N) : 0;  // every index below saturates at N
  __syncthreads();  // every wave holds the old state
  if (tid == 0) {
    S.valid[b] = warm ? 1 : 0;
    S.latched[b] = latched ? 1 : 0;
    S.loss_count[b] = cnt;
    S.prev_mode[b] = surf ? 1 : 0;
    surface[b] = surf ? 1 : 0;
    if (SCHED) Q.need[b] = need ? 1 : 0;
  }
  const double *qb = q + b * ld, *vb = v + b * ld, *th = ff ? tau_hat + b * ld_th : nullptr, *qn = q_nom + b * NQ;
  auto x0at = [&](int j) -> double { return j < 7 ? qb[j] : (j < 14 ? vb[j - 7] : th[j - 14]); };
  if (tid < nx) x0[b * nx + tid] = x0at(tid);
  // problem references (_problem_arrays, crocoddyl_classical.py:521-556; _tau_ref)
  double* ir = inst_ref + b * 21;
  if (tid < 14) ir[tid] = P.posture_mode ? (tid < 7 ? qn[tid] : 0.0) : x0at(tid);
  if (P.torque_mode == 2) {
    if (tid >= 64 && tid < 64 + NQ) ir[14 + tid - 64] = 0.0;
  } else if (tid == 64) {  // wave 1, so wave 0's lanes go on with the copies
    double qq[NQ], g[NQ];
    for (int i = 0; i < NQ; ++i) qq[i] = P.torque_mode == 1 ? qn[i] : qb[i];
    if (mount) {
      gravity_torque<true>(*rb, qq, g, link ? link + b * FFDDP_LINK_W : nullptr, mount + b * FFDDP_MOUNT_W);
    } else if (link) {
      gravity_torque(*rb, qq, g, link + b * FFDDP_LINK_W);
    } else {
      gravity_torque(*rb, qq, g);
    }
    for (int i = 0; i < NQ; ++i) ir[14 + i] = g[i];
  }
  const int nref = (N + 1) * 6, nxs = (N + 1) * nx, nus = N * NU;
  double* nr = node_ref + b * nref;
  if (TASK) {
    for (int k = tid; k <= N; k += FLEET_BLOCK) fleet_task_ref(rec, T.p_site_minus_frame, t_task, k, dt_ocp, nr + k * 6);
  } else {
    for (int i = tid; i < nref; i += FLEET_BLOCK) nr[i] = node1[i];
  }
  // _shift_guess, as k_fleet_warm_start
  const double* kx = S.keep_xs + b * nxs;
  double* xo = xs_init + b * nxs;
  const double* ub = ff ? th : S.tau_prev + b * NU;
  const double* ku = S.keep_us + b * nus;
  double* uo = us_init + b * nus;
  if (!SCHED) {
    for (int i = tid; i < nxs; i += FLEET_BLOCK) xo[i] = (warm && i >= nx) ? kx[i] : x0at(i % nx);
    for (int i = tid; i < nus; i += FLEET_BLOCK) uo[i] = warm ? ku[i + NU < nus ? i + NU : i] : ub[i % NU];
  } else if (need) {
    // _shift_guess of the lists shifted `age` times: xs knot min(k + age, N), us knot min(k + 1 + age, N - 1)
    for (int i = tid; i < nxs; i += FLEET_BLOCK) {
      const int k = i / nx, j = i - k * nx, ks = k + age < N ? k + age : N;
      xo[i] = (warm && k >= 1) ? kx[ks * nx + j] : x0at(j);
    }
    for (int i = tid; i < nus; i += FLEET_BLOCK) {
      const int k = i / NU, j = i - k * NU, ks = k + 1 + age < N - 1 ? k + 1 + age : N - 1;
      uo[i] = warm ? ku[ks * NU + j] : ub[j];
    }
  }
}

// max |x| over lanes 0..6 of the wave; a NaN propagates, as in np.max(np.abs(.))
__device__ __forceinline__ double fleet_absmax7(double x) {
  double m = 0.0;
  bool nan = false;
  for (int i = 0; i < NU; ++i) {
    const double y = fabs(__shfl(x, i));
    nan |= y != y;
    m = fmax(m, y);
  }
  return nan ? __builtin_nan("") : m;
}

// Row i of the torque policy from the kept first knot, in the fleets' order of
// operations (no contraction: only the order inside the dot products differs
// from numpy's).  Classical (_policy_control, crocoddyl_classical.py:759-779):
// us0 + s K0 (x0 - xs0); force feedback (Eq. 14-18, crocoddyl_force_feedback.py:
// 1041-1093) -> tau_des, then the inverse actuation map -> the return value.
template <bool FF>
__device__ __forceinline__ double fleet_policy_row(const ffddp_fleet_params& P, int i, bool valid, const double* ur,
                                                   const double* xr, const double* xr1, const double* Kr,
                                                   const double* x0b, const double* tau_prev, double& tau_des) {
#pragma clang fp contract(off)
  if (!FF) {
    double t = valid ? ur[i] : tau_prev[i];
    if (P.use_feedback_policy && valid) {
      double acc = 0.0;
      for (int j = 0; j < 14; ++j) acc += Kr[i * 14 + j] * (x0b[j] - xr[j]);
      t = t + P.feedback_gain_scale * acc;
    }
    tau_des = __builtin_nan("");
    return t;
  }
  const double eps = P.ff_use_tau_interpolation ? P.eps_pol : 0.0;
  const double tau0 = xr[14 + i], tau1 = xr1[14 + i], th = x0b[14 + i];  // xr1: the knot after xr
  double tp = tau0 + eps * (tau1 - tau0);
  if (P.use_feedback_policy) {
    const double c = eps * (1.0 - P.alpha_ocp);
    double ax = 0.0, at = 0.0;
    for (int j = 0; j < 14; ++j) ax += (c * Kr[i * 21 + j]) * (xr[j] - x0b[j]);
    for (int j = 0; j < 7; ++j) {
      const double I = i == j ? 1.0 : 0.0;
      at += (I + c * (Kr[i * 21 + 14 + j] - I)) * (xr[14 + j] - x0b[14 + j]);
    }
    tp = tp + P.feedback_gain_scale * (ax + at);
  }
  tau_des = valid ? tp : th;
  double t = tau_des;
  if (P.ff_inverse_actuation_model) t = (t - P.alpha_ctrl * th) / fmax(1.0e-6, 1.0 - P.alpha_ctrl);
  return t;
}

// np.clip(x, lo, hi): a NaN propagates
__device__ __forceinline__ double fleet_clip(double x, double lo, double hi) {
  return x != x ? x : fmin(fmax(x, lo), hi);
}

// Everything after the solve: k_fleet_keep's keep, then (wave 0 of the
// instance's first block, lanes 0-6 = the seven joints) the policy, _command,
// the info record, and the sweep's actuation and log columns when asked for.
//
// tau_lim (ffddp_fleet_post_lim_dev): the clips use the instance's own limit,
// entry 4i of its torque-limit row; null: P.tau_limits.
//
// SCHED (ffddp_fleet_post_sched_dev): only the instances that solved this tick
// (Q.need) can be kept; the policy reads the kept solution through Q.age (see
// k_fleet_pre), _safe_tau's trust / rate / smoothing filter follows the clip
// when Q.apply_filter, and the policy wave updates since / age last (the
// instance's other blocks read only need).  SCHED = false is
// ffddp_fleet_post_dev's kernel, unchanged (Q unused).
template <bool SCHED>
__global__ __launch_bounds__(FLEET_BLOCK) void k_fleet_post(
    int N, int nx, ffddp_fleet_params P, ffddp_fleet_state S, ffddp_fleet_sched Q, const double* __restrict__ xs,
    const double* __restrict__ us, const double* __restrict__ K, const double* __restrict__ cost,
    const int32_t* __restrict__ iters, const uint8_t* __restrict__ ok, const double* __restrict__ fn_pred,
    const int32_t* __restrict__ stats, const double* __restrict__ x0, const uint8_t* __restrict__ surface,
    const double* __restrict__ tau_bias, long ld_bias, double* __restrict__ tau_cmd, double* __restrict__ info,
    const double* __restrict__ scale, double* __restrict__ tau_app, double* __restrict__ tau_filt, double lpf,
    const double* __restrict__ obs, long ld_obs, double* __restrict__ log_obs, const double* __restrict__ tau_lim) {
  const long b = blockIdx.x;
  const int t0 = blockIdx.y * FLEET_BLOCK + threadIdx.x, step = FLEET_CHUNKS * FLEET_BLOCK;
  const long nxs = (long)(N + 1) * nx, nus = (long)N * NU, nK = (long)N * NU * nx;
  const double *xn = xs + b * nxs, *un = us + b * nus, *Kn = K + b * nK;
  double *xk = S.keep_xs + b * nxs, *uk = S.keep_us + b * nus, *Kk = S.keep_K + b * nK;
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(lane < NU ? (isfinite(un[lane]) ? 1 : 0) : 1);
  // SCHED: an instance that did not solve keeps nothing (its us row is its last solve's)
  const bool need = !SCHED || Q.need[b] != 0;
  const bool fin = need && m == ~0ull;
  if (fin) {
    for (int i = t0; i < nxs; i += step) xk[i] = xn[i];
    for (int i = t0; i < nus; i += step) uk[i] = un[i];
    for (int i = t0; i < nK; i += step) Kk[i] = Kn[i];
  }
  if (blockIdx.y != 0 || threadIdx.x >= 64) return;
  // the kept first knot (when fin the new solution, read in place: the copy above is other waves' work)
  const double *xr = fin ? xn : xk, *ur = fin ? un : uk, *Kr = fin ? Kn : Kk;
  const double* xr1 = xr + nx;
  int age0 = 0;
  if (SCHED) {
    // knot 0 of the shifted lists: us / K knot min(age, N-1), xs knot min(age, N), the next xs knot min(age+1, N)
    age0 = fin ? 0 : Q.age[b];
    const int a = age0 < N ? age0 : N, au = a < N - 1 ? a : N - 1, a1 = a + 1 < N ? a + 1 : N;
    xr1 = xr + (long)a1 * nx;
    xr += (long)a * nx;
    ur += (long)au * NU;
    Kr += (long)au * NU * nx;
  }
  const bool ff = nx == 21, on = lane < NU;
  const int i = on ? lane : 0;  // lanes 7.. repeat joint 0 and write nothing
  const bool valid = S.valid[b] != 0 || fin;
  const double* x0b = x0 + b * nx;
  double* tprev = S.tau_prev + b * NU;
  const bool surf = surface[b] != 0;
  double tau_des;
  double traw = ff ? fleet_policy_row<true>(P, i, valid, ur, xr, xr1, Kr, x0b, tprev, tau_des)
                   : fleet_policy_row<false>(P, i, valid, ur, xr, xr1, Kr, x0b, tprev, tau_des);
  const double tau_des_inf = ff ? fleet_absmax7(tau_des) : __builtin_nan("");
  // _command: unstable fallback (crocoddyl_classical.py:392-404), _safe_tau (:260-284)
  const double tau_raw_inf = fleet_absmax7(traw), cb = cost[b];
  const bool unstable = !isfinite(cb) || cb > P.max_solver_cost || tau_raw_inf > P.max_tau_raw_inf;
  double tc;
  {
#pragma clang fp contract(off)
    if (unstable) traw = tau_bias[b * ld_bias + i] - P.fallback_dq_damping * x0b[7 + i];
    const bool bad = __ballot(on && !isfinite(traw)) != 0;
    // tau_lim (ffddp_fleet_post_lim_dev): the instance's own limit, entry 4i of its row
    const double lim = tau_lim ? tau_lim[b * FFDDP_TAU_LIM_W + 4 * i] : P.tau_limits[i], x = bad ? tprev[i] : traw;
    tc = x != x ? x : fmin(fmax(x, -lim), lim);
    if (SCHED && Q.apply_filter) {  // _safe_tau's filter (crocoddyl_classical.py:272-284), its order and grouping
      const double prev = tprev[i], al = Q.tau_smoothing_alpha, ms = Q.tau_rate_limit[i] * Q.dt;
      double d = fleet_clip(tc - prev, -Q.tau_trust_inf, Q.tau_trust_inf);
      d = fleet_clip(d, -ms, ms);
      tc = fleet_clip((1.0 - al) * prev + al * (prev + d), -lim, lim);
    }
  }
  const double tau_cmd_inf = fleet_absmax7(tc);
  if (on) {
    tprev[i] = tc;
    tau_cmd[b * NU + i] = tc;
    if (tau_app) {
#pragma clang fp contract(off)
      const double ta = scale ? tc * scale[b * NU + i] : tc;
      tau_app[b * NU + i] = ta;
      if (tau_filt) tau_filt[b * NU + i] = (1.0 - lpf) * tau_filt[b * NU + i] + lpf * ta;
    }
  }
  if (log_obs && lane < FFDDP_FLEET_LOG_W)  // site position, normal force, contact flag
    log_obs[b * FFDDP_FLEET_LOG_W + lane] = obs[b * ld_obs + (lane < 3 ? 28 + lane : 43 + lane)];
  if (lane != 0) return;
  S.valid[b] = (valid && !unstable) ? 1 : 0;
  double* f = info + b * FFDDP_FLEET_INFO_W;
  f[0] = (double)ok[b];
  f[1] = cb;
  f[2] = (double)iters[b];
  f[3] = fin ? 1.0 : 0.0;
  f[4] = unstable ? 1.0 : 0.0;
  f[5] = surf ? 1.0 : 0.0;
  f[6] = valid ? 0.0 : -1.0;
  f[7] = need ? (double)stats[b * FFDDP_NSTATS + 9] : 0.0;
  f[8] = tau_raw_inf;
  f[9] = tau_cmd_inf;
  f[10] = tau_des_inf;
  // predicted normal force (classical: knot 0; force feedback: _predicted_normal_force_next_step, :1219-1243)
  const double fn0 = fn_pred[b * 2], fn1 = fn_pred[b * 2 + 1];
  double fp;
  if (!ff) {
    fp = surf ? fn0 : __builtin_nan("");
  } else {
#pragma clang fp contract(off)
    const double f0 = fabs(fn0), f1 = fabs(fn1);
    const double f01 = (N == 1 || !P.ff_dt_mpc_below_dt_ocp) ? f0 : (1.0 - P.eps_pol) * f0 + P.eps_pol * f1;
    const double fnx = N == 1 ? f0 : (!isfinite(f0) ? f1 : (!isfinite(f1) ? f0 : f01));
    fp = (surf && isfinite(fnx)) ? fnx : __builtin_nan("");
  }
  f[11] = fp;
  if (SCHED) {  // last: since / age belong to this lane
    Q.since[b] = need ? 0 : Q.since[b] + 1;
    Q.age[b] = need ? age0 : age0 + 1;
  }
}

}  // namespace

// ===========================================================================
// host side
// ===========================================================================
// copies of the host entry point, issued per slice by launch_solve_t: inputs
// host -> device before the slice's first kernel, outputs device -> host
// after its last; `done[k]` is recorded on slice k's stream after them
struct HostIO {
  struct In {
    void* dev;
    const void* host;
    size_t per_inst;
  } in[6];
  struct Out {
    void* host;
    const void* dev;
    size_t per_inst;
  } out[5];
  int n_in = 0, n_out = 0;
  hipEvent_t* done = nullptr;
  // filled by launch_solve_t: the slices [b0[k], b0[k] + bk[k])
  int ns = 0;
  int b0[8] = {0}, bk[8] = {0};
  // optional: called before slice k's input copies are enqueued (the host
  // stages that slice's pageable inputs); with it the slices are enqueued
  // one after the other instead of iteration by iteration
  std::function<int(int)> stage;
};

struct ffddp_handle {
  int device = 0;
  int max_batch = 0;
  DevConsts hc{};
  DevConsts* dc = nullptr;
  ffddp_robot* drb = nullptr;
  Dev d{};
  // staging for host-pointer API
  double *in_x0 = nullptr, *in_nref = nullptr, *in_iref = nullptr, *in_xs = nullptr, *in_us = nullptr;
  uint8_t* in_surf = nullptr;
  double *out_xs = nullptr, *out_us = nullptr, *out_K = nullptr, *out_cost = nullptr, *out_fn = nullptr;
  int32_t *out_iters = nullptr, *out_stats = nullptr;
  uint8_t* out_ok = nullptr;
  std::string err;
  // host entry point: page-locked staging (inputs + outputs, max_batch)
  // and the per-slice completion events
  char* stage = nullptr;
  size_t stage_bytes = 0;
  std::vector<hipEvent_t> hdone;
  CopyPool* pool = nullptr;  // host copies of the host entry point (first host solve)
  // per-iteration trace (ffddp_trace_enable)
  double* trace = nullptr;
  int trace_it = 0;
  // live solve plans (their graphs captured this handle's workspace and
  // trace pointer): ffddp_trace_enable refuses while any is alive and
  // ffddp_destroy invalidates them; last_done marks the end of the last
  // solve_batch[_dev] call, which ffddp_plan_run waits for on the device
  std::vector<ffddp_plan*> plans;
  hipEvent_t last_done = nullptr;
  bool last_done_set = false;
  // [max_batch][N+1] filled with fn_des: the force reference of a solve with cost weights
  // and no force_ref of its own (first such solve)
  double* fref_const = nullptr;
  // [max_batch][FFDDP_COST_W] rows of the configuration's weights: the cost weights of a solve with torque
  // limits and no cost_w of its own (first such solve)
  double* cw_const = nullptr;
  // [max_batch][FFDDP_TAU_LIM_W] rows of the configuration's limits: the torque limits of a solve with link
  // rows and no tau_lim of its own (first such solve)
  double* ul_const = nullptr;
  // [max_batch][FFDDP_LINK_W] rows of the handle's robot: the link model of a solve with mount rows and no
  // link_rows of its own (first such solve)
  double* md_const = nullptr;
  // sub-batch streams: the batch is split into nstreams slices solved on their
  // own HIP streams, so latency-bound phases of one slice overlap with the
  // throughput-bound phases of another (FFDDP_STREAMS, default 4: three
  // created streams plus the caller's stream, the 4 hardware queues a process
  // gets; FFDDP_CALLER_SLICE=0 puts every slice on a created stream)
  int nstreams = 4;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> sev;  // fork + per-stream join events
  std::vector<hipEvent_t> stg;  // start-stagger events (FFDDP_STAGGER)
  bool caller_slice = true;  // FFDDP_CALLER_SLICE
  // FFDDP_STAGGER: 0 off, 1 slice k's first node stage after slice k-1's,
  // 2 after its init; -1 (default) picks per solve: 1 when the slices exceed
  // one wave per SIMD share (throughput-bound first iterations: B=4096
  // +2.3 %, B=2048 +4 % over 2), else 0 (latency-bound: the stagger only
  // delays the last slice, B=512/1024 +1.2 % over 1)
  int stagger = -1;
  // FFDDP_NODE_REP=0: the first node stage evaluates every node of a uniform cold start instead of
  // node 0 and k_node_rep's copies (same results)
  bool node_rep = true;
  int fw_first = 4;  // trials evaluated before the fallback pass (FFDDP_FW_FIRST)
  // first-pass trial counts of the first iterations (FFDDP_FW_SCHED="2,2,2,2"):
  // while every instance is active the line search is throughput-bound, so a
  // 2-trial first pass (alpha 1, 1/2 cover ~90 % of the instances) halves its
  // work and the second pass, needed there anyway, covers the rest; once most
  // instances are done the pass is latency-bound and 4 trials in one pass win
  std::vector<int> fw_sched{2, 2, 2, 2};
  int bw_late_max = -1;  // active instances up to which a slice's backward pass uses the latency variant
                         // (FFDDP_BW_LATE_MAX; -1: SIMDs / slices)
  int bw_w2_max = -1;    // ... and the two-wave variant (FFDDP_BW_W2_MAX; -1: SIMDs / (2 slices); 0: never)
  int n_simd = 1024;     // SIMDs of the device (4 per CU)
  bool fw_fill = true;   // widen the first line-search pass to fill the SIMDs (FFDDP_FW_FILL=0: off)
  // horizon from which an 8-wide first pass takes all ten (FFDDP_FW_LONG;
  // 0: never, the default since round 5: C5 tracking 64.0k-64.8k -> 65.7k-66.1k,
  // random x0 29.3k -> 28.9k; round 3 measured +4.5 % for it)
  int fw_long = 0;
  int fw_wide_max = -1;  // active instances per slice up to which the first pass takes every step length
                         // (decided on the device; FFDDP_FW_WIDE_MAX; -1: SIMDs / slices; 0: never)
  int ls_row_max = -1;   // trial groups of a line-search pass up to which it runs one group per DPP row
                         // (decided on the device; FFDDP_LS_ROW_MAX; -1: 4 SIMDs / slices, one wave
                         // per SIMD share; 0: never)
  // optional per-kernel timing
  bool prof = false;
  int prof_mask = 0;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<int> ev_class;  // class per event pair
  double prof_ms[FFDDP_NKERNELS] = {0};
  int64_t prof_n[FFDDP_NKERNELS] = {0};
};

namespace {

bool stream_pool_acquire(int device, int n, std::vector<hipStream_t>& out);
void stream_pool_release(int device, int n);


int fail(ffddp_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

#define HIPCHK(h, expr)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(h, FFDDP_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

template <class T> int dalloc(ffddp_handle* h, T** p, size_t n) {
  if (hipMalloc((void**)p, n * sizeof(T) + 64) != hipSuccess) {
    *p = nullptr;
    return fail(h, FFDDP_E_OOM, "hipMalloc failed");
  }
  return 0;
}

void free_all(ffddp_handle* h) {
  void* ps[] = {h->dc, h->drb, h->d.alist, h->d.acnt, h->d.rec_buf, h->d.fs, h->d.xs, h->d.us, h->d.K, h->d.k, h->d.w, h->d.xs_try,
                h->d.us_try, h->d.trial, h->d.trial_fail, h->d.st, h->d.uni0, h->d.rep, h->in_x0, h->in_nref, h->in_iref, h->in_xs,
                h->in_us, h->in_surf, h->out_xs, h->out_us, h->out_K, h->out_cost, h->out_fn, h->out_iters,
                h->out_stats, h->out_ok};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  if (h->trace) (void)hipFree(h->trace);
  if (h->fref_const) (void)hipFree(h->fref_const);
  if (h->cw_const) (void)hipFree(h->cw_const);
  if (h->ul_const) (void)hipFree(h->ul_const);
  if (h->md_const) (void)hipFree(h->md_const);
  if (h->stage) (void)hipHostFree(h->stage);
}

// event pair around a launch (only when profiling is enabled)
struct ProfScope {
  ffddp_handle* h;
  hipStream_t s;
  bool on;
  ProfScope(ffddp_handle* h_, hipStream_t s_, int cls) : h(h_), s(s_), on(h_->prof && ((h_->prof_mask >> cls) & 1)) {
    if (!on) return;
    if (h->ev_used + 2 > h->ev_pool.size()) {
      for (int i = 0; i < 256; ++i) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        h->ev_pool.push_back(e);
      }
    }
    h->ev_class.push_back(cls);
    (void)hipEventRecord(h->ev_pool[h->ev_used], s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(h->ev_pool[h->ev_used + 1], s);
    h->ev_used += 2;
  }
};

// profiling classes: one kernel per class (KC_COMMIT: the end-of-solve k_commit)
enum { KC_INIT = 0, KC_NODE, KC_BACKWARD, KC_FORWARD, KC_ACCEPT, KC_COMMIT, KC_FINALIZE, KC_FORWARD2 };

// the per-instance slice [b0, b0 + Bk) of the handle workspace
Dev dev_slice(const Dev& d0, int b0, int Bk, int k) {
  Dev d = d0;
  const long N = d0.N, nx = d0.nx;
  d.B = Bk;
  d.rec_buf += (long)b0 * (N + 1) * d0.rec;
  d.fs += (long)b0 * (N + 1) * nx;
  d.xs += (long)b0 * (N + 1) * nx;
  d.us += (long)b0 * N * NU;
  d.K += (long)b0 * N * NU * nx;
  d.k += (long)b0 * N * NU;
  d.w += (long)b0 * (N + 1) * nx;
  d.xs_try += (long)b0 * NTRIALS * (N + 1) * nx;
  d.us_try += (long)b0 * NTRIALS * N * NU;
  d.trial += (long)b0 * NTRIALS * 2;
  d.trial_fail += (long)b0 * NTRIALS;
  d.st += b0;
  d.alist += 2L * b0;
  d.uni0 += b0;
  d.rep += (long)b0 * REP_W;
  d.acnt += 4 * k;
  if (d.trace) d.trace += (long)b0 * d0.trace_it * FFDDP_TRACE_W;
  if (d.fref) d.fref += (long)b0 * (N + 1);
  if (d.cw) d.cw += (long)b0 * FFDDP_COST_W;
  if (d.ul) d.ul += (long)b0 * FFDDP_TAU_LIM_W;
  if (d.md) d.md += (long)b0 * FFDDP_LINK_W;
  if (d.mt) d.mt += (long)b0 * FFDDP_MOUNT_W;
  return d;
}

// What a solve takes, in the C ABI's order (include/ffddp.h: ffddp_solve_batch_wts_dev): the host entry
// point, the device entry points and the plan capture fill one and hand it down to launch_solve_t.
struct SolveArgs {
  int B;
  const double *x0, *nref, *iref;
  const uint8_t* surf;
  const double *xs_init, *us_init;
  int maxiter, is_feasible;
  double *xs, *us, *K, *cost;
  int32_t* iters;
  uint8_t* ok;
  double* fn_pred;
  int32_t* stats;
  const uint8_t* active;
  const double *fref, *cw, *ul, *md, *mt;
};

template <int NC, bool FF, bool FR, bool CW, bool UL, bool MD, bool MT>
int launch_solve_t(ffddp_handle* h, const SolveArgs& a, hipStream_t s, HostIO* io) {
  const int B = a.B, maxiter = a.maxiter;
  const int N = h->hc.N, nx = h->hc.nx;
  int S = h->nstreams;
  if (B < 64 * S) S = 1;
  if (S > 1) {
    // the streams normally come with the handle (ffddp_create); the fork /
    // join and stagger events on first use
    if ((int)h->streams.size() < S && !stream_pool_acquire(h->device, S, h->streams))
      return fail(h, FFDDP_E_DEVICE, "hipStreamCreate failed");
    while ((int)h->sev.size() < S + 1) {
      hipEvent_t e;
      HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      h->sev.push_back(e);
    }
    while ((int)h->stg.size() < S) {
      hipEvent_t e;
      HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      h->stg.push_back(e);
    }
  }
  const int Bs = (B + S - 1) / S;
  const int stagger = S == 1 ? 0 : (h->stagger >= 0 ? h->stagger : (Bs > h->n_simd / S ? 1 : 0));
  struct Slice {
    Dev d;
    hipStream_t s;
    int b0, B;
  };
  Slice sl[8];
  // device entry point: the solve iterates in the caller's xs / us / K
  // (same [B][N+1][nx] / [B][N][7] / [B][N][7][nx] layout as the handle's
  // buffers), so no copy of the solution follows the last kernel; the host
  // entry point keeps the handle's buffers (its outputs are host memory)
  Dev dbase = h->d;
  dbase.fref = FR ? a.fref : nullptr;
  dbase.cw = CW ? a.cw : nullptr;
  dbase.ul = UL ? a.ul : nullptr;
  dbase.md = MD ? a.md : nullptr;
  dbase.mt = MT ? a.mt : nullptr;
  if (!io) {
    dbase.xs = a.xs;
    dbase.us = a.us;
    dbase.K = a.K;
  }
  for (int k = 0; k < S; ++k) {
    sl[k].b0 = k * Bs;
    sl[k].B = (B - sl[k].b0) < Bs ? (B - sl[k].b0) : Bs;
    sl[k].d = dev_slice(dbase, sl[k].b0, sl[k].B, k);
    // FFDDP_CALLER_SLICE: the last slice runs on the caller's stream (its
    // hardware queue is otherwise idle during the solve)
    sl[k].s = (S > 1 && !(h->caller_slice && k == S - 1)) ? h->streams[k] : s;
  }
  if (S > 1) {
    HIPCHK(h, hipEventRecord(h->sev[0], s));
    for (int k = 0; k < S; ++k)
      if (sl[k].s != s) HIPCHK(h, hipStreamWaitEvent(sl[k].s, h->sev[0], 0));
  }
  const long nxl = nx, N1 = N + 1;
  // the uniform-start replication (k_node_rep): the plain classical kernels only, N >= 2
  constexpr bool REP = !FF && !FR && !CW && !UL && !MD && !MT;
  const bool node_rep = REP && h->node_rep && N >= 2;
  if (io) {
    io->ns = S;
    for (int k = 0; k < S; ++k) {
      io->b0[k] = sl[k].b0;
      io->bk[k] = sl[k].B;
    }
  }
  // host entry point: slice k's inputs go up on its own stream, so its
  // copies overlap the other slices' kernels
  auto enqueue_in = [&](int k) -> int {
    for (int i = 0; i < io->n_in; ++i) {
      const size_t o = (size_t)sl[k].b0 * io->in[i].per_inst;
      HIPCHK(h, hipMemcpyAsync((char*)io->in[i].dev + o, (const char*)io->in[i].host + o,
                               (size_t)sl[k].B * io->in[i].per_inst, hipMemcpyHostToDevice, sl[k].s));
    }
    return 0;
  };
  auto enqueue_init = [&](int k) {
    ProfScope p(h, sl[k].s, KC_INIT);
    const long b0 = sl[k].b0;
    // null: no instance of the slice is flagged as a uniform start
    auto rep_ref = [&](long b) { return node_rep ? a.nref + b * N1 * 6 : nullptr; };
    if (a.active)
      hipLaunchKernelGGL(k_init<true>, dim3(1024), dim3(INIT_BLOCK), 0, sl[k].s, h->dc, sl[k].d,
                         a.xs_init + b0 * N1 * nxl, a.us_init + b0 * (long)N * NU, a.is_feasible, a.active + b0, rep_ref(b0),
                         a.surf + b0, NC);
    else
      hipLaunchKernelGGL(k_init<false>, dim3(1024), dim3(INIT_BLOCK), 0, sl[k].s, h->dc, sl[k].d,
                         a.xs_init + b0 * N1 * nxl, a.us_init + b0 * (long)N * NU, a.is_feasible, nullptr, rep_ref(b0),
                         a.surf + b0, NC);
  };
  // one FDDP iteration of slice k: node stage, backward pass, line search, step decision
  auto enqueue_iter = [&](int k, int it) -> int {
    const Dev& d = sl[k].d;
    const hipStream_t ss = sl[k].s;
    const int Bk = sl[k].B;
    const long b0 = sl[k].b0;
    const double* x0k = a.x0 + b0 * nxl;
    const double* nrefk = a.nref + b0 * N1 * 6;
    const double* irefk = a.iref + b0 * 21;
    const uint8_t* surfk = a.surf + b0;
    const long nodes = (long)Bk * (N + 1);
    // optional start stagger: slice k's first node stage waits for slice
    // k-1's, so the throughput-bound node stages do not all collide
    if (it == 0 && k > 0 && stagger) HIPCHK(h, hipStreamWaitEvent(ss, h->stg[k - 1], 0));
    if (it == 0 && stagger == 2 && k + 1 < S) HIPCHK(h, hipEventRecord(h->stg[k], ss));
    {
      ProfScope p(h, ss, KC_NODE);
      hipLaunchKernelGGL((k_node<NC, FF, FR, CW, UL, MD, MT>), dim3((int)((nodes + NODE_GPB - 1) / NODE_GPB)), dim3(NODE_BLOCK), 0, ss,
                         h->dc, d, x0k, nrefk, irefk, surfk, 0, it & 1, (it == 0 && node_rep) ? 1 : 0);
      if constexpr (REP) {
        if (it == 0 && node_rep)
          hipLaunchKernelGGL((k_node_rep<NC>), dim3((unsigned)(((long)Bk * (N - 1) + NODE_GPB - 1) / NODE_GPB)), dim3(NODE_BLOCK),
                             0, ss, h->dc, d, nrefk, surfk);
      }
    }
    if (it == 0 && stagger == 1 && k + 1 < S) HIPCHK(h, hipEventRecord(h->stg[k], ss));
    {
      ProfScope p(h, ss, KC_BACKWARD);
      const int lmax = h->bw_late_max >= 0 ? h->bw_late_max : h->n_simd / S;
      // two-wave variant: for slices no larger than one wave per SIMD share
      // (small per-GPU batches, where the whole solve is latency-bound) at
      // one wave per SIMD; in the tails of large slices (active count up to
      // lmax) at two waves per SIMD, so its blocks need not wait for the
      // other slices' kernels to free whole SIMDs (the one-wave kernel there:
      // B = 4096 -1.7 %; this one +2 % over LATE).  FF's
      // two-wave pass spills too much at two waves per SIMD: LATE there.
      const bool small = Bk <= h->n_simd / S;
      const int w2auto = small ? h->n_simd / (2 * S) : (FF ? 0 : lmax);
      const int w2max = std::min(lmax, h->bw_w2_max >= 0 ? h->bw_w2_max : w2auto);
      if (lmax < Bk)
        hipLaunchKernelGGL((k_backward_w<FF>), dim3(Bk), dim3(64), 0, ss, h->dc, d, it, it & 1, lmax, w2max);
      if (lmax > w2max && w2max < Bk)
        hipLaunchKernelGGL((k_backward_w<FF, true>), dim3(lmax < Bk ? lmax : Bk), dim3(64), 0, ss, h->dc, d, it, it & 1,
                           lmax, w2max);
      if (w2max > 0) {
        const dim3 g2(w2max < Bk ? w2max : Bk);
        if constexpr (!FF) {
          if (!small) {
            hipLaunchKernelGGL((k_backward_w2<FF, 2>), g2, dim3(128), 0, ss, h->dc, d, it, it & 1, w2max);
          } else {
            hipLaunchKernelGGL((k_backward_w2<FF, 1>), g2, dim3(128), 0, ss, h->dc, d, it, it & 1, w2max);
          }
        } else {
          hipLaunchKernelGGL((k_backward_w2<FF, 1>), g2, dim3(128), 0, ss, h->dc, d, it, it & 1, w2max);
        }
      }
    }
    int n1 = NTRIALS;
    {
      // first pass: trials 0..n1-1, per-iteration schedule (fw_sched) then
      // fw_first; the second pass evaluates the rest for the instances that
      // accepted none of them
      n1 = it < (int)h->fw_sched.size() ? h->fw_sched[it] : h->fw_first;
      // a small batch leaves SIMDs idle: evaluate as many step lengths in
      // the first pass as one wave per SIMD holds (8 groups per wave), so
      // the second pass (a whole extra rollout on the chain) is rarely needed
      if (h->fw_fill) n1 = std::max(n1, std::min(NTRIALS, 8 * h->n_simd / std::max(B, 1)));
      // long horizons (FFDDP_FW_LONG, off by default): a second pass is a
      // rollout ~N node-calcs long, so once the first pass is 8 wide it
      // could take all ten (N=100 point3d, B=1024: +4.5 % in round 3; on
      // the round-5 kernels -2.3 % in the tracking regime, +1.4 % random)
      if (h->fw_fill && h->fw_long > 0 && N >= h->fw_long && n1 >= 8) n1 = NTRIALS;
      // device-side widening of the first pass: while a slice's active
      // instances fit one wave per SIMD share at every step length, all ten
      // run at once (random x0 at B=1024: the second pass ran in every
      // iteration)
      const int wide = h->fw_wide_max >= 0 ? h->fw_wide_max : h->n_simd / S;
      const long g1 = std::max((long)Bk * n1, (long)std::min(Bk, wide) * NTRIALS);  // first-pass groups
      // layout of each pass (ffddp_rollout.hpp): one trial group per DPP
      // row while the pass's groups fit row_max, two otherwise, decided on
      // the device from the active count.  Only slices that fit one wave
      // per SIMD share take the row layout at all: a large slice's late
      // passes would gain it, but launching both layouts every pass (the
      // unchosen one exits at once) cost more than that at B = 4096
      // (507.9k vs 512.4k solves/s).  When every possible
      // pass of the slice fits, only the row layout is launched.
      const int row_max = (h->ls_row_max >= 0 ? h->ls_row_max : 4 * h->n_simd / S) *
                          (h->ls_row_max < 0 && Bk > h->n_simd / S ? 0 : 1);
      const bool row_only = row_max > 0 && (long)Bk * NTRIALS <= (long)row_max;
      auto fw = [&](int tr0, int ntr, int more) {
        const long groups = more ? (long)Bk * ntr : g1;
        if (!row_only) {
          const dim3 grid((unsigned)((groups * G8 + 63) / 64));
          hipLaunchKernelGGL((k_forward_g8<NC, FF, false, FR, CW, UL, MD, MT>), grid, dim3(64), 0, ss, h->dc, d, x0k, nrefk, irefk,
                             surfk, tr0, ntr, more, it & 1, wide, row_max);
        }
        if (row_max > 0) {
          const long rg = std::min(groups, (long)row_max);  // the row layout runs only when they fit
          const dim3 grid((unsigned)((rg * 16 + 63) / 64));
          hipLaunchKernelGGL((k_forward_g8<NC, FF, true, FR, CW, UL, MD, MT>), grid, dim3(64), 0, ss, h->dc, d, x0k, nrefk, irefk,
                             surfk, tr0, ntr, more, it & 1, wide, row_max);
        }
      };
      {
        ProfScope p(h, ss, KC_FORWARD);
        fw(0, n1, 0);
      }
      if (n1 < NTRIALS) {
        ProfScope p(h, ss, KC_FORWARD2);
        fw(n1, NTRIALS - n1, 1);
      }
    }
    {
      ProfScope p(h, ss, KC_ACCEPT);
      hipLaunchKernelGGL(k_accept, dim3((Bk + 63) / 64), dim3(64), 0, ss, h->dc, d, it, n1, it & 1,
                         h->fw_wide_max >= 0 ? h->fw_wide_max : h->n_simd / S);
    }
    return 0;
  };
  const size_t bxs = (size_t)(N + 1) * nx * sizeof(double);
  const size_t bus = (size_t)N * NU * sizeof(double);
  const size_t bks = (size_t)N * NU * nx * sizeof(double);
  // the end of slice k's solve: accepted trials committed, results, and
  // (host entry point) its outputs down and its completion event
  auto enqueue_tail = [&](int k) -> int {
    const Dev& d = sl[k].d;
    const hipStream_t ss = sl[k].s;
    const long b0 = sl[k].b0;
    const int Bk = sl[k].B;
    {
      ProfScope p(h, ss, KC_COMMIT);
      hipLaunchKernelGGL(k_commit, dim3((Bk + COMMIT_IPB - 1) / COMMIT_IPB), dim3(64), 0, ss, h->dc, d);
    }
    {
      ProfScope p(h, ss, KC_FINALIZE);
      hipLaunchKernelGGL((k_finalize<NC, FF, MD, MT>), dim3((2 * Bk + 63) / 64), dim3(64), 0, ss, h->dc, d, maxiter,
                         a.x0 + b0 * nxl, a.nref + b0 * N1 * 6, a.iref + b0 * 21, a.surf + b0, a.cost + b0, a.iters + b0,
                         a.ok + b0, a.fn_pred ? a.fn_pred + 2 * b0 : nullptr,
                         a.stats ? a.stats + b0 * FFDDP_NSTATS : nullptr, a.active ? a.active + b0 : nullptr);
    }
    // host entry point: page-locked host memory, the slice's results go
    // down as soon as it finishes (the device entry point solved in place)
    if (io) {
      HIPCHK(h, hipMemcpyAsync(a.xs + b0 * N1 * nxl, d.xs, bxs * Bk, hipMemcpyDefault, ss));
      HIPCHK(h, hipMemcpyAsync(a.us + b0 * (long)N * NU, d.us, bus * Bk, hipMemcpyDefault, ss));
      HIPCHK(h, hipMemcpyAsync(a.K + b0 * (long)N * NU * nx, d.K, bks * Bk, hipMemcpyDefault, ss));
      for (int i = 0; i < io->n_out; ++i) {
        const size_t o = (size_t)b0 * io->out[i].per_inst;
        HIPCHK(h, hipMemcpyAsync((char*)io->out[i].host + o, (const char*)io->out[i].dev + o,
                                 (size_t)Bk * io->out[i].per_inst, hipMemcpyDeviceToHost, ss));
      }
      HIPCHK(h, hipEventRecord(io->done[k], ss));
    }
    return 0;
  };
  if (io && io->stage) {
    // host entry point with pageable inputs: slice by slice, the host stages
    // slice k's inputs into page-locked memory and enqueues its whole solve
    // before staging slice k+1, so the staging of the later slices overlaps
    // the earlier slices' copies and kernels
    for (int k = 0; k < S; ++k) {
      if (const int rc = io->stage(k)) return rc;
      if (const int rc = enqueue_in(k)) return rc;
      enqueue_init(k);
      for (int it = 0; it < maxiter; ++it)
        if (const int rc = enqueue_iter(k, it)) return rc;
      if (const int rc = enqueue_tail(k)) return rc;
    }
  } else {
    // iteration-major across the slices (the device entry point and solve
    // plans; the host entry point with page-locked inputs)
    if (io)
      for (int k = 0; k < S; ++k)
        if (const int rc = enqueue_in(k)) return rc;
    for (int k = 0; k < S; ++k) enqueue_init(k);
    for (int it = 0; it < maxiter; ++it)
      for (int k = 0; k < S; ++k)
        if (const int rc = enqueue_iter(k, it)) return rc;
    for (int k = 0; k < S; ++k)
      if (const int rc = enqueue_tail(k)) return rc;
  }
  if (hipGetLastError() != hipSuccess) return fail(h, FFDDP_E_DEVICE, "kernel launch failed");
  if (S > 1) {
    for (int k = 0; k < S; ++k) {
      if (sl[k].s == s) continue;
      HIPCHK(h, hipEventRecord(h->sev[1 + k], sl[k].s));
      HIPCHK(h, hipStreamWaitEvent(s, h->sev[1 + k], 0));
    }
  }
  return 0;
}

// The one (nc, variant, force reference, cost weights, torque limits, link model) -> template constants decision, for
// the solve and for ffddp_calc_diff_mdl: f(NC, FF, FR, CW, UL, MD) is called with std::integral_constant arguments.  fr: there is
// a force reference; without one the kernels are the FR = false instantiations.  cw: there are cost-weight rows.
// The CW kernels exist with FR only (the caller supplies a force reference of fn_des where the user gave none: the
// same bits), so the build does not double.  ul: there are torque-limit rows; the UL kernels exist with FR and CW
// only (the caller supplies rows of the configuration's weights likewise).  md: there are link-model rows; the MD
// kernels exist with FR, CW and UL only (the caller supplies rows of the configuration's limits likewise).  mt: there
// are mount rows; the MT kernels exist with FR, CW, UL and MD only (the caller supplies rows of the handle's robot
// likewise).
template <class F> int dispatch_variant(ffddp_handle* h, bool fr, bool cw, bool ul, bool md, bool mt, F&& f) {
  if (cw && !fr) return fail(h, FFDDP_E_INVALID, "cost weights without a force reference");
  if (ul && !cw) return fail(h, FFDDP_E_INVALID, "torque limits without cost weights");
  if (md && !ul) return fail(h, FFDDP_E_INVALID, "link model without torque limits");
  if (mt && !md) return fail(h, FFDDP_E_INVALID, "mount without a link model");
  using NC1 = std::integral_constant<int, 1>;
  using NC3 = std::integral_constant<int, 3>;
  const bool ff = h->hc.variant == FFDDP_FORCE_FEEDBACK;
  auto nc_ff = [&](auto FR, auto CW, auto UL, auto MD, auto MT) -> int {
    if (h->hc.nc == 1)
      return ff ? f(NC1{}, std::true_type{}, FR, CW, UL, MD, MT) : f(NC1{}, std::false_type{}, FR, CW, UL, MD, MT);
    return ff ? f(NC3{}, std::true_type{}, FR, CW, UL, MD, MT) : f(NC3{}, std::false_type{}, FR, CW, UL, MD, MT);
  };
  const std::true_type T{};
  const std::false_type F_{};
  if (mt) return nc_ff(T, T, T, T, T);
  if (md) return nc_ff(T, T, T, T, F_);
  if (ul) return nc_ff(T, T, T, F_, F_);
  if (cw) return nc_ff(T, T, F_, F_, F_);
  if (fr) return nc_ff(T, F_, F_, F_, F_);
  return nc_ff(F_, F_, F_, F_, F_);
}

// io: the host entry point's copies (nullptr: the device entry points and the plan capture)
int launch_solve(ffddp_handle* h, const SolveArgs& a, hipStream_t s, HostIO* io) {
  return dispatch_variant(h, a.fref != nullptr, a.cw != nullptr, a.ul != nullptr, a.md != nullptr, a.mt != nullptr,
                          [&](auto NC, auto FF, auto FR, auto CW, auto UL, auto MD, auto MT) {
                            return launch_solve_t<decltype(NC)::value, decltype(FF)::value, decltype(FR)::value,
                                                  decltype(CW)::value, decltype(UL)::value, decltype(MD)::value,
                                                  decltype(MT)::value>(h, a, s, io);
                          });
}

// The one argument check of ffddp_solve_batch and ffddp_solve_batch_wts_dev.  B == 0 passes without a look at
// the pointers: the caller returns 0 for it.
int solve_args_check(ffddp_handle* h, const SolveArgs& a) {
  if (!h) return FFDDP_E_INVALID;
  if (a.fref && !(h->hc.w_fn > 0.0))
    return fail(h, FFDDP_E_INVALID, "force_ref given but the handle has no fn_track cost (w_fn <= 0)");
  if (a.B < 0 || a.maxiter < 0) return fail(h, FFDDP_E_INVALID, "negative B or maxiter");
  if (a.B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (a.B > 0 && (!a.x0 || !a.nref || !a.iref || !a.surf || !a.xs_init || !a.us_init || !a.xs || !a.us || !a.K ||
                  !a.cost || !a.iters || !a.ok))
    return fail(h, FFDDP_E_INVALID, "null pointer");
  return 0;
}

// Slice streams shared by every handle of the process on a device: a
// process gets 4 hardware queues (GPU_MAX_HW_QUEUES), and every stream
// beyond them shares a queue with another, serialising two slices (a second
// handle's own 3 streams took a B = 4096 host-entry solve from 11.4 to
// 15.4 ms).  Handles are not thread-safe anyway; two handles used from one
// thread just queue their slices on the same streams.  Ref-counted: the last
// release destroys them.
struct StreamPool {
  std::vector<hipStream_t> s;
  int refs = 0;
};
std::mutex g_pool_mu;
StreamPool g_pool[64];

bool stream_pool_acquire(int device, int n, std::vector<hipStream_t>& out) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  StreamPool& p = g_pool[device & 63];
  while ((int)p.s.size() < n) {
    hipStream_t st;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return false;
    p.s.push_back(st);
  }
  const int had = (int)out.size();
  out.assign(p.s.begin(), p.s.begin() + n);
  p.refs += n - had;
  return true;
}

void stream_pool_release(int device, int n) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  StreamPool& p = g_pool[device & 63];
  p.refs -= n;
  if (p.refs <= 0) {
    for (hipStream_t st : p.s) (void)hipStreamDestroy(st);
    p.s.clear();
    p.refs = 0;
  }
}

// page-locked (hipHostMalloc'd / registered) host memory?
bool host_pinned(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

bool valid_cfg(const ffddp_ocp_config& c) {
  return (c.variant == FFDDP_CLASSICAL || c.variant == FFDDP_FORCE_FEEDBACK) && c.horizon >= 1 &&
         c.horizon <= 4096 && (c.nc == 1 || c.nc == 3) && c.dt > 0.0;
}

}  // namespace

extern "C" {

int ffddp_create(const ffddp_robot* robot, const ffddp_ocp_config* cfg, int device, int max_batch,
                 ffddp_handle** out) {
  if (!robot || !cfg || !out || max_batch < 1) return FFDDP_E_INVALID;
  *out = nullptr;
  if (!valid_cfg(*cfg)) return FFDDP_E_INVALID;
  ffddp_handle* h = new (std::nothrow) ffddp_handle();
  if (!h) return FFDDP_E_OOM;
  h->device = device;
  h->max_batch = max_batch;
  fill_consts(*robot, *cfg, h->hc);
  if (hipSetDevice(device) != hipSuccess) {
    delete h;
    return FFDDP_E_DEVICE;
  }
  const long B = max_batch, N = cfg->horizon, nx = h->hc.nx;
  Dev& d = h->d;
  d.N = (int)N;
  d.nx = (int)nx;
  d.rec = rec_size((int)nx);
  if (d.rec != rec_words((int)nx)) {
    delete h;
    return FFDDP_E_INVALID;
  }
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0)
      h->n_simd = 4 * cu;
    const char* ns = std::getenv("FFDDP_STREAMS");
    if (ns) {
      const int v = std::atoi(ns);
      h->nstreams = v < 1 ? 1 : (v > 8 ? 8 : v);
    }
    if (const char* bl = std::getenv("FFDDP_BW_LATE_MAX")) h->bw_late_max = std::atoi(bl);
    if (const char* bw2 = std::getenv("FFDDP_BW_W2_MAX")) h->bw_w2_max = std::atoi(bw2);
    if (const char* ff = std::getenv("FFDDP_FW_FILL")) h->fw_fill = std::atoi(ff) != 0;
    if (const char* fl = std::getenv("FFDDP_FW_LONG")) h->fw_long = std::atoi(fl);
    if (const char* fwm = std::getenv("FFDDP_FW_WIDE_MAX")) h->fw_wide_max = std::atoi(fwm);
    if (const char* lrm = std::getenv("FFDDP_LS_ROW_MAX")) h->ls_row_max = std::atoi(lrm);
    if (const char* fsch = std::getenv("FFDDP_FW_SCHED")) {
      h->fw_sched.clear();
      for (const char* p = fsch; *p;) {
        const int v = std::atoi(p);
        h->fw_sched.push_back(v < 1 ? 1 : (v > NTRIALS ? NTRIALS : v));
        while (*p && *p != ',') ++p;
        if (*p == ',') ++p;
      }
    }
    if (const char* sg = std::getenv("FFDDP_STAGGER")) h->stagger = std::atoi(sg);
    if (const char* nr = std::getenv("FFDDP_NODE_REP")) h->node_rep = std::atoi(nr) != 0;
    if (const char* cs = std::getenv("FFDDP_CALLER_SLICE")) h->caller_slice = std::atoi(cs) != 0;
    const char* f1 = std::getenv("FFDDP_FW_FIRST");
    if (f1) {
      const int v = std::atoi(f1);
      h->fw_first = v < 1 ? 1 : (v > NTRIALS ? NTRIALS : v);
    }
  }
  // the slice streams now, not at the first solve: a process's first
  // streams get hardware queues of their own (GPU_MAX_HW_QUEUES, 4), and a
  // communicator created before them (RCCL's streams) would leave the
  // slices sharing queues
  if (h->nstreams > 1 && !stream_pool_acquire(h->device, h->nstreams, h->streams)) {
    delete h;
    return FFDDP_E_DEVICE;
  }
  int rc = 0;
  rc |= dalloc(h, &h->dc, 1);
  rc |= dalloc(h, &h->drb, 1);
  rc |= dalloc(h, &d.rec_buf, (size_t)B * (N + 1) * d.rec);
  rc |= dalloc(h, &d.fs, (size_t)B * (N + 1) * nx);
  rc |= dalloc(h, &d.xs, (size_t)B * (N + 1) * nx);
  rc |= dalloc(h, &d.us, (size_t)B * N * NU);
  rc |= dalloc(h, &d.K, (size_t)B * N * NU * nx);
  rc |= dalloc(h, &d.k, (size_t)B * N * NU);
  rc |= dalloc(h, &d.w, (size_t)B * (N + 1) * nx);
  rc |= dalloc(h, &d.xs_try, (size_t)B * NTRIALS * (N + 1) * nx);
  rc |= dalloc(h, &d.us_try, (size_t)B * NTRIALS * N * NU);
  rc |= dalloc(h, &d.trial, (size_t)B * NTRIALS * 2);
  rc |= dalloc(h, &d.trial_fail, (size_t)B * NTRIALS);
  rc |= dalloc(h, &d.st, (size_t)B);
  rc |= dalloc(h, &d.alist, (size_t)B * 2);
  rc |= dalloc(h, &d.uni0, (size_t)B);
  rc |= dalloc(h, &d.rep, (size_t)B * REP_W);
  rc |= dalloc(h, &d.acnt, (size_t)4 * 8);
  rc |= dalloc(h, &h->in_x0, (size_t)B * nx);
  rc |= dalloc(h, &h->in_nref, (size_t)B * (N + 1) * 6);
  rc |= dalloc(h, &h->in_iref, (size_t)B * 21);
  rc |= dalloc(h, &h->in_xs, (size_t)B * (N + 1) * nx);
  rc |= dalloc(h, &h->in_us, (size_t)B * N * NU);
  rc |= dalloc(h, &h->in_surf, (size_t)B);
  rc |= dalloc(h, &h->out_xs, (size_t)B * (N + 1) * nx);
  rc |= dalloc(h, &h->out_us, (size_t)B * N * NU);
  rc |= dalloc(h, &h->out_K, (size_t)B * N * NU * nx);
  rc |= dalloc(h, &h->out_cost, (size_t)B);
  rc |= dalloc(h, &h->out_fn, (size_t)B * 2);
  rc |= dalloc(h, &h->out_iters, (size_t)B);
  rc |= dalloc(h, &h->out_stats, (size_t)B * FFDDP_NSTATS);
  rc |= dalloc(h, &h->out_ok, (size_t)B);
  if (rc) {
    if (!h->streams.empty()) stream_pool_release(h->device, (int)h->streams.size());
    free_all(h);
    delete h;
    return FFDDP_E_OOM;
  }
  if (hipMemcpy(h->dc, &h->hc, sizeof(DevConsts), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->drb, robot, sizeof(ffddp_robot), hipMemcpyHostToDevice) != hipSuccess) {
    if (!h->streams.empty()) stream_pool_release(h->device, (int)h->streams.size());
    free_all(h);
    delete h;
    return FFDDP_E_DEVICE;
  }
  *out = h;
  return 0;
}

#ifdef FFDDP_PHASE_PROF
extern "C" int ffddp_debug_phase_read(unsigned long long* out, int n, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ffddp::g_pp), sizeof(unsigned long long) * (n < 48 ? n : 48)) != hipSuccess) return -2;
  if (reset) {
    unsigned long long z[48] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(ffddp::g_pp), z, sizeof(z)) != hipSuccess) return -2;
  }
  return 0;
}
#endif

int ffddp_profile_enable(ffddp_handle* h, int classes) {
  if (!h) return FFDDP_E_INVALID;
  h->prof_mask = classes & FFDDP_PROFILE_ALL;
  h->prof = h->prof_mask != 0;
  return 0;
}

int ffddp_profile_read(ffddp_handle* h, double* ms, int64_t* launches, int reset) {
  if (!h) return FFDDP_E_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  for (size_t i = 0; i < h->ev_class.size(); ++i) {
    hipEvent_t a = h->ev_pool[2 * i], b = h->ev_pool[2 * i + 1];
    HIPCHK(h, hipEventSynchronize(b));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, a, b));
    h->prof_ms[h->ev_class[i]] += t;
    h->prof_n[h->ev_class[i]] += 1;
  }
  h->ev_class.clear();
  h->ev_used = 0;
  for (int k = 0; k < FFDDP_NKERNELS; ++k) {
    if (ms) ms[k] = h->prof_ms[k];
    if (launches) launches[k] = h->prof_n[k];
    if (reset) {
      h->prof_ms[k] = 0.0;
      h->prof_n[k] = 0;
    }
  }
  return 0;
}

static void plan_invalidate(ffddp_plan* p);

void ffddp_destroy(ffddp_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (ffddp_plan* p : h->plans) plan_invalidate(p);
  h->plans.clear();
  if (h->last_done) (void)hipEventDestroy(h->last_done);
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->sev) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->stg) (void)hipEventDestroy(e);
  if (!h->streams.empty()) stream_pool_release(h->device, (int)h->streams.size());
  for (hipEvent_t e : h->hdone) (void)hipEventDestroy(e);
  delete h->pool;
  free_all(h);
  delete h;
}

const char* ffddp_last_error(const ffddp_handle* h) { return h ? h->err.c_str() : "null handle"; }

// the end of the solve just enqueued on stream s (every slice has joined s),
// for ffddp_plan_run to wait on
static int mark_solve_done(ffddp_handle* h, hipStream_t s) {
  if (!h->last_done) HIPCHK(h, hipEventCreateWithFlags(&h->last_done, hipEventDisableTiming));
  HIPCHK(h, hipEventRecord(h->last_done, s));
  h->last_done_set = true;
  return 0;
}

// the handle's constant force reference (fn_des everywhere), made on first use: the CW kernels are
// instantiated with FR only, and an array of fn_des reproduces the scalar path's bits
static int const_force_ref(ffddp_handle* h) {
  if (h->fref_const) return 0;
  const size_t n = (size_t)h->max_batch * (h->hc.N + 1);
  const std::vector<double> v(n, h->hc.fn_ref[h->hc.nc - 1]);
  if (int rc = dalloc(h, &h->fref_const, n)) return rc;
  HIPCHK(h, hipMemcpy(h->fref_const, v.data(), n * 8, hipMemcpyHostToDevice));
  return 0;
}

// the handle's constant cost-weight rows (the configuration's weights in every row; config.cost_weight_row's
// entries), made on first use: the UL kernels are instantiated with CW only, and rows of the handle's weights
// reproduce the scalar path's bits
static int const_cost_rows(ffddp_handle* h) {
  if (h->cw_const) return 0;
  const DevConsts& c = h->hc;
  const bool ff = c.variant == FFDDP_FORCE_FEEDBACK;
  double row[FFDDP_COST_W] = {};
  row[FFDDP_CW_EE_ORI] = c.w_ori;
  row[FFDDP_CW_WDAMP] = c.w_wd;
  row[FFDDP_CW_EE_POS] = c.w_ee_pos;
  row[FFDDP_CW_TANGENT_POS] = c.w_tp;
  row[FFDDP_CW_TANGENT_VEL] = c.w_tv;
  row[FFDDP_CW_PLANE_Z] = c.w_pz;
  row[FFDDP_CW_VZ] = c.w_vz;
  row[FFDDP_CW_UNILATERAL] = c.w_uni;
  row[FFDDP_CW_FN] = c.w_fn;
  row[FFDDP_CW_FRICTION_CONE] = c.nc == 3 ? c.w_fc : 0.0;
  row[FFDDP_CW_POSTURE] = c.w_post;
  row[FFDDP_CW_V] = c.w_v;
  row[FFDDP_CW_Q_SOFT_LIMITS] = c.w_qs;
  row[FFDDP_CW_TAU] = c.w_tau;
  row[FFDDP_CW_TAU_SOFT_LIMITS] = c.w_ts;
  row[FFDDP_CW_Y] = ff ? c.w_y : 0.0;
  row[FFDDP_CW_W] = ff ? c.w_w : 0.0;
  row[FFDDP_CW_W_SOFT_LIMITS] = ff ? c.w_ws : 0.0;
  const size_t n = (size_t)h->max_batch * FFDDP_COST_W;
  std::vector<double> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = row[i % FFDDP_COST_W];
  if (int rc = dalloc(h, &h->cw_const, n)) return rc;
  HIPCHK(h, hipMemcpy(h->cw_const, v.data(), n * 8, hipMemcpyHostToDevice));
  return 0;
}

int ffddp_torque_limit_rows(const ffddp_ocp_config* cfg, int B, const double* tau_limits, double* rows) {
  if (!cfg || B < 0 || (B > 0 && (!tau_limits || !rows))) return FFDDP_E_INVALID;
  for (long i = 0; i < (long)B * 7; ++i)
    if (!(std::isfinite(tau_limits[i]) && tau_limits[i] > 0.0)) return FFDDP_E_INVALID;
  for (long b = 0; b < B; ++b)
    torque_limit_row(tau_limits + b * 7, cfg->tau_soft_limit_margin, rows + b * FFDDP_TAU_LIM_W);
  return 0;
}

// the handle's constant torque-limit rows (the configuration's limits in every row, packed by torque_limit_row's
// own code from the constants fill_consts derived), made on first use: the MD kernels are instantiated with UL only, and rows of the handle's limits reproduce the
// constants' bits (the lower bounds are the exact negations)
static int const_limit_rows(ffddp_handle* h) {
  if (h->ul_const) return 0;
  const DevConsts& c = h->hc;
  double row[FFDDP_TAU_LIM_W];
  torque_limit_row_pack(c.u_ub, c.ts_ub, c.ws_lim, row);
  const size_t n = (size_t)h->max_batch * FFDDP_TAU_LIM_W;
  std::vector<double> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = row[i % FFDDP_TAU_LIM_W];
  if (int rc = dalloc(h, &h->ul_const, n)) return rc;
  HIPCHK(h, hipMemcpy(h->ul_const, v.data(), n * 8, hipMemcpyHostToDevice));
  return 0;
}

int ffddp_link_model_rows(const ffddp_robot* robots, int B, double* rows) {
  if (B < 0 || (B > 0 && (!robots || !rows))) return FFDDP_E_INVALID;
  for (long b = 0; b < B; ++b) {
    const ffddp_robot& r = robots[b];
    for (int j = 0; j < 7; ++j) {
      if (!(std::isfinite(r.mass[j]) && r.mass[j] > 0.0)) return FFDDP_E_INVALID;
      for (int e = 0; e < 3; ++e)
        if (!std::isfinite(r.com[j][e])) return FFDDP_E_INVALID;
      for (int e = 0; e < 9; ++e)
        if (!std::isfinite(r.inertia[j][e])) return FFDDP_E_INVALID;
    }
  }
  for (long b = 0; b < B; ++b) link_model_row(robots[b], rows + b * FFDDP_LINK_W);
  return 0;
}

// the handle's constant link-model rows (the handle's robot in every row, link_model_row's plain copies), made on
// first use: the MT kernels are instantiated with MD only, and rows of the handle's robot reproduce its bits
static int const_link_rows(ffddp_handle* h) {
  if (h->md_const) return 0;
  double row[FFDDP_LINK_W];
  link_model_row(h->hc.rb, row);
  const size_t n = (size_t)h->max_batch * FFDDP_LINK_W;
  std::vector<double> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = row[i % FFDDP_LINK_W];
  if (int rc = dalloc(h, &h->md_const, n)) return rc;
  HIPCHK(h, hipMemcpy(h->md_const, v.data(), n * 8, hipMemcpyHostToDevice));
  return 0;
}

int ffddp_mount_rows(const ffddp_robot* robots, int B, double* rows) {
  if (B < 0 || (B > 0 && (!robots || !rows))) return FFDDP_E_INVALID;
  for (long b = 0; b < B; ++b) {
    const ffddp_robot& r = robots[b];
    for (int e = 0; e < 9; ++e)
      if (!std::isfinite(r.joint_R[0][e])) return FFDDP_E_INVALID;
    for (int e = 0; e < 3; ++e)
      if (!std::isfinite(r.joint_p[0][e]) || !std::isfinite(r.gravity[e])) return FFDDP_E_INVALID;
  }
  for (long b = 0; b < B; ++b) mount_row(robots[b], rows + b * FFDDP_MOUNT_W);
  return 0;
}

int ffddp_solve_batch_wts_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w, void* stream) {
  return ffddp_solve_batch_lim_dev(h, B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs,
                                   us, K, cost, iters, ok, fn_pred, stats, active, force_ref, cost_w, nullptr, stream);
}

int ffddp_solve_batch_lim_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w,
                              const double* tau_lim, void* stream) {
  return ffddp_solve_batch_mdl_dev(h, B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs,
                                   us, K, cost, iters, ok, fn_pred, stats, active, force_ref, cost_w, tau_lim, nullptr,
                                   stream);
}

int ffddp_solve_batch_mdl_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w,
                              const double* tau_lim, const double* link_rows, void* stream) {
  return ffddp_solve_batch_mnt_dev(h, B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs,
                                   us, K, cost, iters, ok, fn_pred, stats, active, force_ref, cost_w, tau_lim, link_rows,
                                   nullptr, stream);
}

int ffddp_solve_batch_mnt_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w,
                              const double* tau_lim, const double* link_rows, const double* mount_rows, void* stream) {
  SolveArgs a{B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs, us, K, cost, iters, ok,
              fn_pred, stats, active, force_ref, cost_w, tau_lim, link_rows, mount_rows};
  if (int rc = solve_args_check(h, a)) return rc;
  if (B == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  // the handle's workspace is shared by every solve: a solve enqueued on
  // another (possibly non-blocking) stream must finish before this one starts
  if (h->last_done_set) HIPCHK(h, hipStreamWaitEvent((hipStream_t)stream, h->last_done, 0));
  if (mount_rows && !link_rows) {
    if (int rc = const_link_rows(h)) return rc;
    a.md = h->md_const;
  }
  if (a.md && !tau_lim) {
    if (int rc = const_limit_rows(h)) return rc;
    a.ul = h->ul_const;
  }
  if (a.ul && !cost_w) {
    if (int rc = const_cost_rows(h)) return rc;
    a.cw = h->cw_const;
  }
  if (a.cw && !force_ref) {
    if (int rc = const_force_ref(h)) return rc;
    a.fref = h->fref_const;
  }
  if (int rc = launch_solve(h, a, (hipStream_t)stream, nullptr)) return rc;
  return mark_solve_done(h, (hipStream_t)stream);
}

int ffddp_solve_batch_fref_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                               const double* inst_ref, const uint8_t* surface, const double* xs_init,
                               const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                               double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                               const uint8_t* active, const double* force_ref, void* stream) {
  return ffddp_solve_batch_wts_dev(h, B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs,
                                   us, K, cost, iters, ok, fn_pred, stats, active, force_ref, nullptr, stream);
}

int ffddp_solve_batch_sel_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, void* stream) {
  return ffddp_solve_batch_fref_dev(h, B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs,
                                    us, K, cost, iters, ok, fn_pred, stats, active, nullptr, stream);
}

int ffddp_solve_batch_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                          const uint8_t* surface, const double* xs_init, const double* us_init, int maxiter,
                          int is_feasible, double* xs, double* us, double* K, double* cost, int32_t* iters,
                          uint8_t* ok, double* fn_pred, int32_t* stats, void* stream) {
  return ffddp_solve_batch_sel_dev(h, B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs,
                                   us, K, cost, iters, ok, fn_pred, stats, nullptr, stream);
}

// error exit of the host entry point after its first asynchronous copy: the
// slice streams may still be copying from the staging buffer or the caller's
// page-locked arrays, or into them; wait for all of them before returning
static int drain_host_solve(ffddp_handle* h, int rc) {
  for (hipStream_t st : h->streams) (void)hipStreamSynchronize(st);
  (void)hipStreamSynchronize(nullptr);
  (void)hipGetLastError();
  return rc;
}

int ffddp_solve_batch(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                      const uint8_t* surface, const double* xs_init, const double* us_init, int maxiter,
                      int is_feasible, double* xs, double* us, double* K, double* cost, int32_t* iters, uint8_t* ok,
                      double* fn_pred, int32_t* stats) {
  // the caller's host arrays; no active mask, force reference, cost weights, torque limits, link model or mount on this path
  const SolveArgs user{B, x0, node_ref, inst_ref, surface, xs_init, us_init, maxiter, is_feasible, xs, us, K, cost,
                       iters, ok, fn_pred, stats, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (int rc = solve_args_check(h, user)) return rc;
  if (B == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t N = (size_t)h->hc.N, nx = (size_t)h->hc.nx;
  // per-instance bytes: inputs x0, node_ref, inst_ref, surface, xs_init, us_init;
  // outputs xs, us, K, cost, iters, ok, fn_pred, stats
  const size_t per[14] = {nx * 8, (N + 1) * 6 * 8, 21 * 8, 1, (N + 1) * nx * 8, N * NU * 8,
                          (N + 1) * nx * 8, N * NU * 8, N * NU * nx * 8, 8, 4, 1, 16, FFDDP_NSTATS * 4};
  size_t off[14], tot = 0;
  for (int i = 0; i < 14; ++i) {
    off[i] = tot;
    tot += ((per[i] * (size_t)h->max_batch + 255) / 256) * 256;
  }
  if (!h->stage) {
    if (hipHostMalloc((void**)&h->stage, tot, hipHostMallocDefault) != hipSuccess) {
      h->stage = nullptr;
      (void)hipGetLastError();
      return fail(h, FFDDP_E_OOM, "hipHostMalloc (staging) failed");
    }
    h->stage_bytes = tot;
  }
  while (h->hdone.size() < 8) {
    hipEvent_t e;
    HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->hdone.push_back(e);
  }
  if (!h->pool) {
    try {
      h->pool = new CopyPool(copy_threads());
    } catch (...) {
      h->pool = nullptr;
    }
  }
  if (!h->pool) return fail(h, FFDDP_E_OOM, "copy pool");
  CopyPool& pool = *h->pool;
  HostIO io;
  io.done = h->hdone.data();
  const bool tm = std::getenv("FFDDP_HOSTIO_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = tm ? now() : 0.0;
  // inputs: page-locked caller memory goes up directly, pageable memory
  // through the staging buffer, slice by slice: the host stages slice k and
  // enqueues its whole solve, then stages slice k+1 while slice k runs
  const void* uin[6] = {x0, node_ref, inst_ref, surface, xs_init, us_init};
  void* din[6] = {h->in_x0, h->in_nref, h->in_iref, h->in_surf, h->in_xs, h->in_us};
  bool stin[6];
  bool any_in = false;
  for (int i = 0; i < 6; ++i) {
    stin[i] = !host_pinned(uin[i]);
    any_in |= stin[i];
    io.in[io.n_in++] = HostIO::In{din[i], stin[i] ? (const void*)(h->stage + off[i]) : uin[i], per[i]};
  }
  double tst[8] = {0};
  if (any_in)
    io.stage = [&](int k) {
      std::vector<CopyJob> jobs;
      for (int i = 0; i < 6; ++i)
        if (stin[i]) {
          const size_t o = (size_t)io.b0[k] * per[i];
          jobs.push_back(CopyJob{h->stage + off[i] + o, (const char*)uin[i] + o, (size_t)io.bk[k] * per[i]});
        }
      pool.run(jobs);
      if (tm) tst[k] = now();
      return 0;
    };
  // outputs: slice by slice into page-locked caller memory, else into the
  // staging buffer and from there into the caller's arrays as each slice ends
  void* uout[8] = {xs, us, K, cost, iters, ok, fn_pred, stats};
  void* hout[8];
  bool staged[8];
  for (int i = 0; i < 8; ++i) {
    staged[i] = uout[i] != nullptr && !host_pinned(uout[i]);
    hout[i] = uout[i] == nullptr ? nullptr : (staged[i] ? (void*)(h->stage + off[6 + i]) : uout[i]);
  }
  const void* dsmall[5] = {h->out_cost, h->out_iters, h->out_ok, h->out_fn, h->out_stats};
  for (int i = 0; i < 5; ++i)
    if (hout[3 + i]) io.out[io.n_out++] = HostIO::Out{hout[3 + i], dsmall[i], per[9 + i]};
  // the caller slice runs on the null stream: a created stream of its own
  // would be a fifth stream on the process's 4 hardware queues and share one
  // with a slice (measured: 15.3 vs 11.6 ms per B = 4096 solve)
  hipStream_t cs = nullptr;
  // after an asynchronous device-entry solve still running on a caller
  // stream (possibly non-blocking): this solve reuses its workspace
  if (h->last_done_set) {
    const hipError_t e = hipStreamWaitEvent(cs, h->last_done, 0);
    if (e != hipSuccess) return fail(h, FFDDP_E_DEVICE, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
  }
  // the solve itself works on the handle's device buffers; xs / us / K: where launch_solve_t copies them down to
  const SolveArgs a{B, h->in_x0, h->in_nref, h->in_iref, h->in_surf, h->in_xs, h->in_us, maxiter, is_feasible,
                    (double*)hout[0], (double*)hout[1], (double*)hout[2], h->out_cost, h->out_iters, h->out_ok,
                    h->out_fn, h->out_stats, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (int rc = launch_solve(h, a, cs, &io)) return drain_host_solve(h, rc);
  const double t2 = tm ? now() : 0.0;
  // while the device solves: the first touch of the caller's pageable output
  // arrays (fresh numpy arrays are unmapped pages; faulting them in during
  // the drain below would sit on the solve's tail), by the same threads
  {
    std::vector<CopyJob> jobs;
    for (int i = 0; i < 8; ++i)
      if (staged[i]) jobs.push_back(CopyJob{uout[i], nullptr, (size_t)B * per[6 + i]});
    pool.run(jobs);
  }
  const double t3 = tm ? now() : 0.0;
  // drain the slices in the order they finish
  double tw[8] = {0}, tc[8] = {0};
  bool drained[8] = {false};
  for (int left = io.ns; left > 0;) {
    int k = -1;
    for (int j = 0; j < io.ns && k < 0; ++j) {
      if (drained[j]) continue;
      const hipError_t e = hipEventQuery(io.done[j]);
      if (e == hipSuccess) k = j;
      else if (e != hipErrorNotReady)
        return drain_host_solve(h, fail(h, FFDDP_E_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(e)));
    }
    if (k < 0) {
      std::this_thread::yield();
      continue;
    }
    if (tm) tw[k] = now();
    std::vector<CopyJob> jobs;
    for (int i = 0; i < 8; ++i) {
      if (!staged[i]) continue;
      const size_t o = (size_t)io.b0[k] * per[6 + i];
      jobs.push_back(CopyJob{(char*)uout[i] + o, (const char*)hout[i] + o, (size_t)io.bk[k] * per[6 + i]});
    }
    pool.run(jobs);
    if (tm) tc[k] = now();
    drained[k] = true;
    --left;
  }
  {
    const hipError_t e = hipStreamSynchronize(cs);
    if (e != hipSuccess)
      return drain_host_solve(h, fail(h, FFDDP_E_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e)));
  }
  if (tm) {
    std::fprintf(stderr, "[ffddp host io] %d copy threads | enqueue+stage-in %.2f ms", pool.threads(), t2 - t0);
    for (int k = 0; k < io.ns; ++k) std::fprintf(stderr, " (slice %d staged +%.2f)", k, tst[k] - t0);
    std::fprintf(stderr, " | output first touch done +%.2f", t3 - t0);
    for (int k = 0; k < io.ns; ++k) std::fprintf(stderr, " | slice %d done +%.2f copied +%.2f", k, tw[k] - t0, tc[k] - t0);
    std::fprintf(stderr, " | total %.2f ms\n", now() - t0);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// solve plans: the whole host-array solve of a fixed batch captured once as a
// HIP graph (one input copy, every kernel, one output copy) and replayed per
// call -- the receding-horizon loop's one solve per control tick
// ---------------------------------------------------------------------------
struct ffddp_plan {
  ffddp_handle* h = nullptr;  // null once the handle is destroyed (plan_invalidate)
  int device = 0;
  int B = 0;
  hipStream_t s = nullptr;
  hipGraphExec_t ge = nullptr;
  char *hin = nullptr, *hout = nullptr;  // page-locked, packed
  char *din = nullptr, *dout = nullptr;  // device, same layouts
  size_t in_bytes = 0, out_bytes = 0;
};

namespace {
// packed layouts: 8-byte fields first, then int32, then bytes; each field
// starts on a 256-byte boundary
struct PlanLayout {
  size_t x0, nref, iref, xs_init, us_init, surf, in_bytes;
  size_t xs, us, K, cost, fn, iters, stats, ok, out_bytes;
};
static PlanLayout plan_layout(int B, int N, int nx) {
  PlanLayout L{};
  size_t o = 0;
  auto put = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  const size_t b = (size_t)B, n = (size_t)N, x = (size_t)nx;
  L.x0 = put(b * x * 8);
  L.nref = put(b * (n + 1) * 6 * 8);
  L.iref = put(b * 21 * 8);
  L.xs_init = put(b * (n + 1) * x * 8);
  L.us_init = put(b * n * NU * 8);
  L.surf = put(b);
  L.in_bytes = o;
  o = 0;
  L.xs = put(b * (n + 1) * x * 8);
  L.us = put(b * n * NU * 8);
  L.K = put(b * n * NU * x * 8);
  L.cost = put(b * 8);
  L.fn = put(b * 2 * 8);
  L.iters = put(b * 4);
  L.stats = put(b * FFDDP_NSTATS * 4);
  L.ok = put(b);
  L.out_bytes = o;
  return L;
}

static void plan_free(ffddp_plan* p) {
  if (p->ge) (void)hipGraphExecDestroy(p->ge);
  if (p->s) (void)hipStreamDestroy(p->s);
  if (p->din) (void)hipFree(p->din);
  if (p->dout) (void)hipFree(p->dout);
  if (p->hin) (void)hipHostFree(p->hin);
  if (p->hout) (void)hipHostFree(p->hout);
  delete p;
}
}  // namespace

int ffddp_plan_create(ffddp_handle* h, int B, int maxiter, int is_feasible, ffddp_plan** out, ffddp_plan_io* io) {
  if (!h) return FFDDP_E_INVALID;
  if (!out || !io) return fail(h, FFDDP_E_INVALID, "null pointer");
  *out = nullptr;
  if (B < 1 || maxiter < 0) return fail(h, FFDDP_E_INVALID, "plan needs B >= 1 and maxiter >= 0");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  HIPCHK(h, hipSetDevice(h->device));
  const int N = h->hc.N, nx = h->hc.nx;
  const PlanLayout L = plan_layout(B, N, nx);
  ffddp_plan* p = new (std::nothrow) ffddp_plan();
  if (!p) return fail(h, FFDDP_E_OOM, "plan allocation failed");
  p->h = h;
  p->device = h->device;
  p->B = B;
  p->in_bytes = L.in_bytes;
  p->out_bytes = L.out_bytes;
  if (hipHostMalloc((void**)&p->hin, L.in_bytes, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&p->hout, L.out_bytes, hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&p->din, L.in_bytes) != hipSuccess || hipMalloc((void**)&p->dout, L.out_bytes) != hipSuccess) {
    (void)hipGetLastError();
    plan_free(p);
    return fail(h, FFDDP_E_OOM, "plan buffers");
  }
  std::memset(p->hin, 0, L.in_bytes);
  std::memset(p->hout, 0, L.out_bytes);
  if (hipStreamCreateWithFlags(&p->s, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    plan_free(p);
    return fail(h, FFDDP_E_DEVICE, "hipStreamCreate (plan)");
  }
  // capture: inputs up, the device entry point's launch sequence iterating in
  // the plan's own output region, outputs down.  Per-kernel timing events are
  // not captured (profiling is off while capturing).
  const bool prof = h->prof;
  h->prof = false;
  char* di = p->din;
  char* dq = p->dout;
  const SolveArgs a{B, (const double*)(di + L.x0), (const double*)(di + L.nref), (const double*)(di + L.iref),
                    (const uint8_t*)(di + L.surf), (const double*)(di + L.xs_init), (const double*)(di + L.us_init),
                    maxiter, is_feasible, (double*)(dq + L.xs), (double*)(dq + L.us), (double*)(dq + L.K),
                    (double*)(dq + L.cost), (int32_t*)(dq + L.iters), (uint8_t*)(dq + L.ok), (double*)(dq + L.fn),
                    (int32_t*)(dq + L.stats), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = 0;
  hipError_t e = hipStreamBeginCapture(p->s, hipStreamCaptureModeThreadLocal);
  if (e == hipSuccess) {
    e = hipMemcpyAsync(p->din, p->hin, L.in_bytes, hipMemcpyHostToDevice, p->s);
    if (e == hipSuccess)
      rc = launch_solve(h, a, p->s, nullptr);
    if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(p->hout, p->dout, L.out_bytes, hipMemcpyDeviceToHost, p->s);
    hipGraph_t g = nullptr;
    const hipError_t e2 = hipStreamEndCapture(p->s, &g);
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess && rc == 0) e = hipGraphInstantiate(&p->ge, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
  }
  h->prof = prof;
  if (rc == 0 && e != hipSuccess) rc = fail(h, FFDDP_E_DEVICE, std::string("plan capture: ") + hipGetErrorString(e));
  if (rc) {
    (void)hipGetLastError();
    plan_free(p);
    return rc;
  }
  char* hi = p->hin;
  char* ho = p->hout;
  io->x0 = (double*)(hi + L.x0);
  io->node_ref = (double*)(hi + L.nref);
  io->inst_ref = (double*)(hi + L.iref);
  io->surface = (uint8_t*)(hi + L.surf);
  io->xs_init = (double*)(hi + L.xs_init);
  io->us_init = (double*)(hi + L.us_init);
  io->xs = (const double*)(ho + L.xs);
  io->us = (const double*)(ho + L.us);
  io->K = (const double*)(ho + L.K);
  io->cost = (const double*)(ho + L.cost);
  io->iters = (const int32_t*)(ho + L.iters);
  io->ok = (const uint8_t*)(ho + L.ok);
  io->fn_pred = (const double*)(ho + L.fn);
  io->stats = (const int32_t*)(ho + L.stats);
  h->plans.push_back(p);
  *out = p;
  return 0;
}

int ffddp_plan_run(ffddp_plan* p) {
  if (!p || !p->h || !p->ge) return FFDDP_E_INVALID;  // null, or its handle was destroyed
  ffddp_handle* h = p->h;
  HIPCHK(h, hipSetDevice(h->device));
  // the graph works in the handle's workspace: after a solve still running
  // on another stream (solve_batch_dev is asynchronous), never beside it
  if (h->last_done_set) HIPCHK(h, hipStreamWaitEvent(p->s, h->last_done, 0));
  HIPCHK(h, hipGraphLaunch(p->ge, p->s));
  HIPCHK(h, hipStreamSynchronize(p->s));
  return 0;
}

// the handle is going away: drop the graph (it references the handle's
// workspace); the page-locked io arrays and the device buffers stay until
// ffddp_plan_destroy
static void plan_invalidate(ffddp_plan* p) {
  (void)hipStreamSynchronize(p->s);
  if (p->ge) (void)hipGraphExecDestroy(p->ge);
  p->ge = nullptr;
  p->h = nullptr;
}

void ffddp_plan_destroy(ffddp_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->s);
  if (p->h) {
    std::vector<ffddp_plan*>& v = p->h->plans;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == p) {
        v.erase(v.begin() + (long)i);
        break;
      }
  }
  plan_free(p);
}

int ffddp_host_alloc(size_t bytes, void** p) {
  if (!p) return FFDDP_E_INVALID;
  *p = nullptr;
  if (hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return FFDDP_E_OOM;
  }
  return 0;
}

int ffddp_host_free(void* p) {
  if (!p) return 0;
  return hipHostFree(p) == hipSuccess ? 0 : FFDDP_E_DEVICE;
}

int ffddp_get_solver_params(const ffddp_handle* h, ffddp_solver_params* p) {
  if (!h || !p) return FFDDP_E_INVALID;
  const DevConsts& c = h->hc;
  *p = ffddp_solver_params{};
  p->th_stop = c.th_stop;
  p->th_grad = c.th_grad;
  p->th_acceptstep = c.th_acceptstep;
  p->th_acceptnegstep = c.th_acceptnegstep;
  p->th_stepdec = c.th_stepdec;
  p->th_stepinc = c.th_stepinc;
  p->reg_min = c.reg_min;
  p->reg_max = c.reg_max;
  p->reg_incfactor = c.reg_inc;
  p->reg_decfactor = c.reg_dec;
  p->neg_step_rule = c.neg_rule;
  return 0;
}

int ffddp_set_solver_params(ffddp_handle* h, const ffddp_solver_params* p) {
  if (!h || !p) return FFDDP_E_INVALID;
  const double v[10] = {p->th_stop, p->th_grad, p->th_acceptstep, p->th_acceptnegstep, p->th_stepdec,
                        p->th_stepinc, p->reg_min, p->reg_max, p->reg_incfactor, p->reg_decfactor};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) return fail(h, FFDDP_E_INVALID, "solver parameters must be finite and >= 0");
  if (!(p->reg_min > 0.0) || p->reg_max < p->reg_min || !(p->reg_incfactor > 1.0) || !(p->reg_decfactor > 1.0))
    return fail(h, FFDDP_E_INVALID, "need 0 < reg_min <= reg_max and reg factors > 1");
  if (p->neg_step_rule != FFDDP_NEGSTEP_CROCODDYL && p->neg_step_rule != FFDDP_NEGSTEP_BOUNDED_RISE)
    return fail(h, FFDDP_E_INVALID, "neg_step_rule must be FFDDP_NEGSTEP_CROCODDYL or FFDDP_NEGSTEP_BOUNDED_RISE");
  DevConsts c = h->hc;
  c.th_stop = p->th_stop;
  c.th_grad = p->th_grad;
  c.th_acceptstep = p->th_acceptstep;
  c.th_acceptnegstep = p->th_acceptnegstep;
  c.th_stepdec = p->th_stepdec;
  c.th_stepinc = p->th_stepinc;
  c.reg_min = p->reg_min;
  c.reg_max = p->reg_max;
  c.reg_inc = p->reg_incfactor;
  c.reg_dec = p->reg_decfactor;
  c.neg_rule = p->neg_step_rule;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());  // no solve in flight reads the constants while they change
  HIPCHK(h, hipMemcpy(h->dc, &c, sizeof(DevConsts), hipMemcpyHostToDevice));
  h->hc = c;
  return 0;
}

int ffddp_trace_enable(ffddp_handle* h, int max_iters) {
  if (!h || max_iters < 0) return FFDDP_E_INVALID;
  // a live plan's graph writes the trace buffer it captured (or none)
  if (!h->plans.empty())
    return fail(h, FFDDP_E_INVALID, "solve plans of this handle are alive: destroy them before ffddp_trace_enable");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->trace) {
    HIPCHK(h, hipDeviceSynchronize());
    (void)hipFree(h->trace);
  }
  h->trace = nullptr;
  h->trace_it = 0;
  h->d.trace = nullptr;
  h->d.trace_it = 0;
  if (max_iters == 0) return 0;
  if (int rc = dalloc(h, &h->trace, (size_t)h->max_batch * max_iters * FFDDP_TRACE_W)) return rc;
  h->trace_it = max_iters;
  h->d.trace = h->trace;
  h->d.trace_it = max_iters;
  return 0;
}

int ffddp_trace_read(ffddp_handle* h, int B, double* out) {
  if (!h || !out || B < 0 || B > h->max_batch) return FFDDP_E_INVALID;
  if (!h->trace) return fail(h, FFDDP_E_INVALID, "trace not enabled (ffddp_trace_enable)");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());  // diagnostic read: every stream's solve has finished
  HIPCHK(h, hipMemcpy(out, h->trace, (size_t)B * h->trace_it * FFDDP_TRACE_W * 8, hipMemcpyDeviceToHost));
  return 0;
}

int ffddp_calc_diff(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                    const uint8_t* surface, const double* xs, const double* us, double* Fx, double* Fu, double* Lx,
                    double* Lu, double* Lxx, double* Lxu, double* Luu, double* cost, double* xnext, double* lam) {
  return ffddp_calc_diff_wts(h, B, x0, node_ref, inst_ref, surface, xs, us, nullptr, nullptr, Fx, Fu, Lx, Lu, Lxx, Lxu,
                             Luu, cost, xnext, lam);
}

int ffddp_calc_diff_fref(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                         const uint8_t* surface, const double* xs, const double* us, const double* force_ref,
                         double* Fx, double* Fu, double* Lx, double* Lu, double* Lxx, double* Lxu, double* Luu,
                         double* cost, double* xnext, double* lam) {
  return ffddp_calc_diff_wts(h, B, x0, node_ref, inst_ref, surface, xs, us, force_ref, nullptr, Fx, Fu, Lx, Lu, Lxx,
                             Lxu, Luu, cost, xnext, lam);
}

int ffddp_calc_diff_wts(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                        const uint8_t* surface, const double* xs, const double* us, const double* force_ref,
                        const double* cost_w, double* Fx, double* Fu, double* Lx, double* Lu, double* Lxx, double* Lxu,
                        double* Luu, double* cost, double* xnext, double* lam) {
  return ffddp_calc_diff_lim(h, B, x0, node_ref, inst_ref, surface, xs, us, force_ref, cost_w, nullptr, Fx, Fu, Lx, Lu,
                             Lxx, Lxu, Luu, cost, xnext, lam);
}

int ffddp_calc_diff_lim(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                        const uint8_t* surface, const double* xs, const double* us, const double* force_ref,
                        const double* cost_w, const double* tau_lim, double* Fx, double* Fu, double* Lx, double* Lu,
                        double* Lxx, double* Lxu, double* Luu, double* cost, double* xnext, double* lam) {
  return ffddp_calc_diff_mdl(h, B, x0, node_ref, inst_ref, surface, xs, us, force_ref, cost_w, tau_lim, nullptr, Fx, Fu,
                             Lx, Lu, Lxx, Lxu, Luu, cost, xnext, lam);
}

int ffddp_calc_diff_mdl(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                        const uint8_t* surface, const double* xs, const double* us, const double* force_ref,
                        const double* cost_w, const double* tau_lim, const double* link_rows, double* Fx, double* Fu,
                        double* Lx, double* Lu, double* Lxx, double* Lxu, double* Luu, double* cost, double* xnext,
                        double* lam) {
  return ffddp_calc_diff_mnt(h, B, x0, node_ref, inst_ref, surface, xs, us, force_ref, cost_w, tau_lim, link_rows, nullptr,
                             Fx, Fu, Lx, Lu, Lxx, Lxu, Luu, cost, xnext, lam);
}

int ffddp_calc_diff_mnt(ffddp_handle* h, int B, const double* x0, const double* node_ref, const double* inst_ref,
                        const uint8_t* surface, const double* xs, const double* us, const double* force_ref,
                        const double* cost_w, const double* tau_lim, const double* link_rows, const double* mount_rows,
                        double* Fx, double* Fu, double* Lx, double* Lu, double* Lxx, double* Lxu, double* Luu,
                        double* cost, double* xnext, double* lam) {
  if (!h) return FFDDP_E_INVALID;
  if (B < 1 || B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "bad B");
  if (force_ref && !(h->hc.w_fn > 0.0))
    return fail(h, FFDDP_E_INVALID, "force_ref given but the handle has no fn_track cost (w_fn <= 0)");
  HIPCHK(h, hipSetDevice(h->device));
  // diagnostic call: the force reference lives in a buffer of its own for the call
  struct Tmp {
    double* p = nullptr;
    ~Tmp() {
      if (p) (void)hipFree(p);
    }
  } fref, cw, ul, md, mt;
  const bool with_md = link_rows || mount_rows;
  const bool with_ul = tau_lim || with_md;
  const bool with_cw = cost_w || with_ul;
  if (force_ref) {
    HIPCHK(h, hipMalloc((void**)&fref.p, (size_t)B * (h->hc.N + 1) * 8));
    HIPCHK(h, hipMemcpy(fref.p, force_ref, (size_t)B * (h->hc.N + 1) * 8, hipMemcpyHostToDevice));
  } else if (with_cw) {
    if (int rc = const_force_ref(h)) return rc;
  }
  if (with_ul && !cost_w)
    if (int rc = const_cost_rows(h)) return rc;
  if (tau_lim) {
    HIPCHK(h, hipMalloc((void**)&ul.p, (size_t)B * FFDDP_TAU_LIM_W * 8));
    HIPCHK(h, hipMemcpy(ul.p, tau_lim, (size_t)B * FFDDP_TAU_LIM_W * 8, hipMemcpyHostToDevice));
  } else if (with_md) {
    if (int rc = const_limit_rows(h)) return rc;
  }
  if (mount_rows) {
    if (!link_rows)
      if (int rc = const_link_rows(h)) return rc;
    HIPCHK(h, hipMalloc((void**)&mt.p, (size_t)B * FFDDP_MOUNT_W * 8));
    HIPCHK(h, hipMemcpy(mt.p, mount_rows, (size_t)B * FFDDP_MOUNT_W * 8, hipMemcpyHostToDevice));
  }
  if (link_rows) {
    HIPCHK(h, hipMalloc((void**)&md.p, (size_t)B * FFDDP_LINK_W * 8));
    HIPCHK(h, hipMemcpy(md.p, link_rows, (size_t)B * FFDDP_LINK_W * 8, hipMemcpyHostToDevice));
  }
  if (cost_w) {
    HIPCHK(h, hipMalloc((void**)&cw.p, (size_t)B * FFDDP_COST_W * 8));
    HIPCHK(h, hipMemcpy(cw.p, cost_w, (size_t)B * FFDDP_COST_W * 8, hipMemcpyHostToDevice));
  }
  const int N = h->hc.N, nx = h->hc.nx, R = h->d.rec;
  const bool ff = h->hc.variant == FFDDP_FORCE_FEEDBACK;
  Dev d = h->d;
  d.B = B;
  d.fref = fref.p ? fref.p : (with_cw ? h->fref_const : nullptr);
  d.cw = cw.p ? cw.p : (with_ul ? h->cw_const : nullptr);
  d.ul = ul.p ? ul.p : (with_md ? h->ul_const : nullptr);
  d.md = md.p ? md.p : (mount_rows ? h->md_const : nullptr);
  d.mt = mt.p;
  HIPCHK(h, hipMemcpy(h->in_x0, x0, (size_t)B * nx * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->in_nref, node_ref, (size_t)B * (N + 1) * 6 * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->in_iref, inst_ref, (size_t)B * 21 * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->in_surf, surface, (size_t)B, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->in_xs, xs, (size_t)B * (N + 1) * nx * 8, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->in_us, us, (size_t)B * N * NU * 8, hipMemcpyHostToDevice));
  // node kernel reads (xs, us) from the solver state: initialise it from the inputs
  hipLaunchKernelGGL(k_init<false>, dim3(1024), dim3(INIT_BLOCK), 0, nullptr, h->dc, d, h->in_xs, h->in_us, 0, nullptr, nullptr, nullptr, 0);
  const int rc = dispatch_variant(h, d.fref != nullptr, d.cw != nullptr, d.ul != nullptr, d.md != nullptr, d.mt != nullptr,
                                  [&](auto NC, auto FF, auto FR, auto CW, auto UL, auto MD, auto MT) {
    const long nodes = (long)B * (N + 1);
    hipLaunchKernelGGL((k_node<decltype(NC)::value, decltype(FF)::value, decltype(FR)::value, decltype(CW)::value,
                               decltype(UL)::value, decltype(MD)::value, decltype(MT)::value>),
                       dim3((int)((nodes + NODE_GPB - 1) / NODE_GPB)), dim3(NODE_BLOCK), 0, nullptr, h->dc, d, h->in_x0,
                       h->in_nref, h->in_iref, h->in_surf, 1, 0, 0);
    return 0;
  });
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipDeviceSynchronize());
  std::vector<double> rec((size_t)B * (N + 1) * R), fsv((size_t)B * (N + 1) * nx);
  HIPCHK(h, hipMemcpy(rec.data(), d.rec_buf, rec.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(fsv.data(), d.fs, fsv.size() * 8, hipMemcpyDeviceToHost));
  const double dt = h->hc.dt;
  for (int b = 0; b < B; ++b) {
    for (int t = 0; t <= N; ++t) {
      const double* r = rec.data() + ((size_t)b * (N + 1) + t) * R;
      const size_t nt = (size_t)b * (N + 1) + t;
      for (int i = 0; i < nx; ++i) Lx[nt * nx + i] = r[rec_off_Lx(nx) + i];
      for (int e = 0; e < nx * nx; ++e) Lxx[nt * nx * nx + e] = r[rec_off_Lxx(nx) + e];
      cost[nt] = r[rec_off_cost(nx)];
      for (int c = 0; c < 3; ++c) lam[nt * 3 + c] = r[rec_off_lam(nx) + c];
      if (t == N) continue;
      const size_t rt = (size_t)b * N + t;
      const double* A = r + rec_off_A();
      for (int i = 0; i < NU; ++i) Lu[rt * NU + i] = r[rec_off_Lu(nx) + i];
      for (int e = 0; e < nx * NU; ++e) Lxu[rt * nx * NU + e] = r[rec_off_Lxu(nx) + e];
      for (int e = 0; e < NU * NU; ++e) Luu[rt * NU * NU + e] = r[rec_off_Luu(nx) + e];
      for (int i = 0; i < nx; ++i) {
        for (int j = 0; j < nx; ++j) {
          double v = (i == j) ? 1.0 : 0.0;
          if (i < 14 && j < (ff ? 21 : 14)) {
            v += (i < 7 ? dt * dt : dt) * A[j * NQ + (i % 7)];
            if (i < 7 && j == i + 7) v += dt;
          }
          if (ff && i >= 14) v = (i == j) ? h->hc.alpha : 0.0;
          Fx[rt * nx * nx + i * nx + j] = v;
        }
        for (int kk = 0; kk < NU; ++kk) {
          double v;
          if (!ff)
            v = (i < 7 ? dt * dt : dt) * A[(14 + kk) * NQ + (i % 7)];
          else
            v = (i >= 14 && i - 14 == kk) ? h->hc.beta : 0.0;
          Fu[rt * nx * NU + i * NU + kk] = v;
        }
      }
      // xnext = xs[t+1] + fs[t+1]  (fs computed with is_feasible = 0)
      for (int i = 0; i < nx; ++i)
        xnext[rt * nx + i] = xs[((size_t)b * (N + 1) + t + 1) * nx + i] + fsv[((size_t)b * (N + 1) + t + 1) * nx + i];
    }
  }
  return 0;
}

int ffddp_frame_placement(const ffddp_robot* robot, const double* q, double* R, double* p) {
  if (!robot || !q || !R || !p) return FFDDP_E_INVALID;
  RBOut<double> o;
  const double zero[NQ] = {0, 0, 0, 0, 0, 0, 0};
  rb_pass<double, false, false>(*robot, q, zero, zero, nullptr, o, nullptr);
  for (int i = 0; i < 9; ++i) R[i] = o.Ree.m[i];
  p[0] = o.pee.x;
  p[1] = o.pee.y;
  p[2] = o.pee.z;
  return 0;
}

int ffddp_gravity_torque(const ffddp_robot* robot, int B, const double* q, double* tau) {
  if (!robot || !q || !tau || B < 0) return FFDDP_E_INVALID;
  for (int b = 0; b < B; ++b) gravity_torque(*robot, q + (size_t)b * NQ, tau + (size_t)b * NQ);
  return 0;
}

int ffddp_gravity_torque_dev(ffddp_handle* h, int B, const double* q, double* tau, void* stream) {
  if (!h || B < 0) return FFDDP_E_INVALID;
  if (B == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gravity, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->drb, B, q, tau);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_gravity_torque_mdl_dev(ffddp_handle* h, int B, const double* q, const double* link_rows, double* tau,
                                 void* stream) {
  if (!link_rows) return ffddp_gravity_torque_dev(h, B, q, tau, stream);
  if (!h || B < 0) return FFDDP_E_INVALID;
  if (B == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gravity_mdl, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->drb, B, q, link_rows, tau);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_gravity_torque_mnt_dev(ffddp_handle* h, int B, const double* q, const double* link_rows,
                                 const double* mount_rows, double* tau, void* stream) {
  if (!h || B < 0) return FFDDP_E_INVALID;
  if (B > 0 && (!q || !tau)) return fail(h, FFDDP_E_INVALID, "ffddp_gravity_torque_mnt_dev: null pointer");
  if (!mount_rows) return ffddp_gravity_torque_mdl_dev(h, B, q, link_rows, tau, stream);
  if (B == 0) return 0;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_gravity_mnt, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->drb, B, q, link_rows,
                     mount_rows, tau);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_build_problem_dev(ffddp_handle* h, int B, const ffddp_task* task, const double* t0, const double* x0,
                            double* node_ref, double* inst_ref, uint8_t* surface, void* stream) {
  if (!h || !task || B < 0) return FFDDP_E_INVALID;
  if (B == 0) return 0;
  if (!t0 || !x0 || !node_ref || !inst_ref || !surface) return FFDDP_E_INVALID;
  if (task->posture_mode < 0 || task->posture_mode > 1 || task->torque_mode < 0 || task->torque_mode > 2) {
    h->err = "ffddp_build_problem_dev: posture_mode must be 0/1 and torque_mode 0/1/2";
    return FFDDP_E_INVALID;
  }
  // make_approach_then_circle's closure constants (trajectories.py:36-60)
  TaskTraj T{};
  for (int i = 0; i < 3; ++i) T.center[i] = task->center[i];
  T.radius = task->radius;
  T.omega = task->omega;
  T.z_contact = task->z_contact;
  T.t_approach = std::max(task->t_approach, 1.0e-6);
  T.t_pre = std::max(task->t_pre, 0.0);
  T.t_hold = task->t_hold;
  for (int i = 0; i < 3; ++i) T.p_cs[i] = task->center[i];
  T.p_cs[0] += task->radius;
  T.p_cs[2] = task->z_contact;
  for (int i = 0; i < 3; ++i) T.p_start[i] = task->has_ee_start ? task->ee_start[i] : T.p_cs[i];
  if (!task->has_ee_start) T.p_start[2] += 0.08;
  const double z_pre = task->has_z_pre ? task->z_pre : std::max(task->z_contact + 0.05, T.p_start[2]);
  for (int i = 0; i < 3; ++i) T.p_pre[i] = T.p_cs[i];
  T.p_pre[2] = z_pre;
  const int N = h->hc.N;
  const long n = (long)B * (N + 1);
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_build, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, h->drb, T, *task, B, N,
                     h->hc.nx, h->hc.dt, t0, x0, node_ref, inst_ref, surface);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_fleet_warm_start_dev(ffddp_handle* h, int B, const double* x0, const double* u_cold, const uint8_t* valid,
                               const double* keep_xs, const double* keep_us, double* xs_init, double* us_init,
                               void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_warm_start_dev: B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!x0 || !u_cold || !valid || !keep_xs || !keep_us || !xs_init || !us_init)
    return fail(h, FFDDP_E_INVALID, "ffddp_fleet_warm_start_dev: null pointer");
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_fleet_warm_start, dim3(B, FLEET_CHUNKS), dim3(FLEET_BLOCK), 0, (hipStream_t)stream, h->hc.N,
                     h->hc.nx, x0, u_cold, valid, keep_xs, keep_us, xs_init, us_init);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_fleet_keep_dev(ffddp_handle* h, int B, const double* xs, const double* us, const double* K,
                         const double* cost, const int32_t* iters, const uint8_t* ok, const double* fn_pred,
                         const int32_t* stats, double* keep_xs, double* keep_us, double* keep_K, double* first,
                         void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_keep_dev: B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!xs || !us || !K || !cost || !iters || !ok || !fn_pred || !stats || !keep_xs || !keep_us || !keep_K || !first)
    return fail(h, FFDDP_E_INVALID, "ffddp_fleet_keep_dev: null pointer");
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_fleet_keep, dim3(B, FLEET_CHUNKS), dim3(FLEET_BLOCK), 0, (hipStream_t)stream, h->hc.N, h->hc.nx,
                     xs, us, K, cost, iters, ok, fn_pred, stats, keep_xs, keep_us, keep_K, first);
  HIPCHK(h, hipGetLastError());
  return 0;
}

static bool fleet_state_complete(const ffddp_fleet_state* s) {
  return s->valid && s->latched && s->loss_count && s->prev_mode && s->tau_prev && s->keep_xs && s->keep_us && s->keep_K;
}

static int fleet_sched_check(ffddp_handle* h, const ffddp_fleet_sched& c, const std::string& who) {
  if (!c.since || !c.age || !c.need) return fail(h, FFDDP_E_INVALID, who + ": null pointer");
  if (c.period < 1) return fail(h, FFDDP_E_INVALID, who + ": period must be at least 1");
  if (c.apply_filter && !(c.tau_smoothing_alpha >= 0.0 && c.tau_smoothing_alpha <= 1.0))
    return fail(h, FFDDP_E_INVALID, who + ": tau_smoothing_alpha outside [0, 1]");
  return 0;
}

// The body of ffddp_fleet_pre_dev, _pre_sched_dev, _pre_task_dev and _pre_mdl_dev; `name`: the entry point called,
// for the messages.  sched: the scheduled tick (the SCHED instantiations).  tasks: per-instance tasks (the TASK
// instantiations) in place of node_ref1 / contact_hint.  link: per-instance link-model rows or null.  mount:
// per-instance mount rows or null.
static int fleet_pre(ffddp_handle* h, const char* name, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                     const double* q, const double* v, const double* fn_meas, const double* contact,
                     const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                     const double* q_nom, const double* node_ref1, int contact_hint, double* x0, uint8_t* surface,
                     double* inst_ref, double* node_ref, double* xs_init, double* us_init,
                     const ffddp_fleet_sched* sched, const ffddp_fleet_tasks* tasks, const double* link,
                     const double* mount, void* stream) {
  if (!h) return FFDDP_E_INVALID;
  const std::string who(name);
  if (B <= 0) return fail(h, FFDDP_E_INVALID, who + ": B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  const bool ff = h->hc.nx == 21;
  if (!p || !s || !fleet_state_complete(s) || !q || !v || !fn_meas || !ee_z || (ff && !tau_hat) || !q_nom ||
      (tasks ? !tasks->rec : !node_ref1) || !x0 || !surface || !inst_ref || !node_ref || !xs_init || !us_init)
    return fail(h, FFDDP_E_INVALID, who + ": null pointer");
  if (ld_qv < NQ || ld_scalar < 1 || (ff && ld_tau_hat < NU) || p->phase_source < 0 || p->phase_source > 1 || p->torque_mode < 0 ||
      p->torque_mode > 2 || p->posture_mode < 0 || p->posture_mode > 1)
    return fail(h, FFDDP_E_INVALID, who + ": bad stride or mode");
  if (sched)
    if (const int rc = fleet_sched_check(h, *sched, who)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const auto kern = sched ? (tasks ? k_fleet_pre<true, true> : k_fleet_pre<true, false>)
                          : (tasks ? k_fleet_pre<false, true> : k_fleet_pre<false, false>);
  hipLaunchKernelGGL(kern, dim3(B), dim3(FLEET_BLOCK), 0, (hipStream_t)stream, h->drb, h->hc.N, h->hc.nx, *p, *s,
                     sched ? *sched : ffddp_fleet_sched{}, q, v, fn_meas, contact, ee_z, (long)ld_qv, (long)ld_scalar,
                     tau_hat, (long)ld_tau_hat, q_nom, node_ref1, contact_hint, x0, surface, inst_ref, node_ref, xs_init,
                     us_init, tasks ? *tasks : ffddp_fleet_tasks{}, tasks ? h->hc.dt : 0.0, link, mount);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_fleet_pre_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                        const double* q, const double* v, const double* fn_meas, const double* contact,
                        const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                        const double* q_nom,
                        const double* node_ref1, int contact_hint, double* x0, uint8_t* surface, double* inst_ref,
                        double* node_ref, double* xs_init, double* us_init, void* stream) {
  return fleet_pre(h, "ffddp_fleet_pre_dev", B, p, s, q, v, fn_meas, contact, ee_z, ld_qv, ld_scalar, tau_hat, ld_tau_hat,
                   q_nom, node_ref1, contact_hint, x0, surface, inst_ref, node_ref, xs_init, us_init, nullptr, nullptr,
                   nullptr, nullptr, stream);
}

int ffddp_fleet_pre_sched_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                              const double* q, const double* v, const double* fn_meas, const double* contact,
                              const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                              const double* q_nom, const double* node_ref1, int contact_hint, double* x0,
                              uint8_t* surface, double* inst_ref, double* node_ref, double* xs_init, double* us_init,
                              ffddp_fleet_sched sched, void* stream) {
  return fleet_pre(h, "ffddp_fleet_pre_sched_dev", B, p, s, q, v, fn_meas, contact, ee_z, ld_qv, ld_scalar, tau_hat,
                   ld_tau_hat, q_nom, node_ref1, contact_hint, x0, surface, inst_ref, node_ref, xs_init, us_init, &sched,
                   nullptr, nullptr, nullptr, stream);
}

// The body of ffddp_fleet_post_dev, _post_sched_dev and _post_lim_dev (sched: the scheduled tick, the SCHED
// instantiation; tau_lim: per-instance torque-limit rows or null)
static int fleet_post(ffddp_handle* h, const char* name, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                      const double* xs, const double* us, const double* K, const double* cost, const int32_t* iters,
                      const uint8_t* ok, const double* fn_pred, const int32_t* stats, const double* x0,
                      const uint8_t* surface, const double* tau_bias, int ld_tau_bias, double* tau_cmd, double* info,
                      const double* scale, double* tau_app, double* tau_filt, double lpf, const double* obs,
                      int ld_obs, double* log_obs, const ffddp_fleet_sched* sched, const double* tau_lim,
                      void* stream) {
  if (!h) return FFDDP_E_INVALID;
  const std::string who(name);
  if (B <= 0) return fail(h, FFDDP_E_INVALID, who + ": B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!p || !s || !fleet_state_complete(s) || !xs || !us || !K || !cost || !iters || !ok || !fn_pred || !stats ||
      !x0 || !surface || !tau_bias || !tau_cmd || !info)
    return fail(h, FFDDP_E_INVALID, who + ": null pointer");
  if (ld_tau_bias < NU || (log_obs && (!obs || ld_obs < FFDDP_PLANT_OBS)) || (tau_filt && !tau_app))
    return fail(h, FFDDP_E_INVALID, who + ": bad stride or optional arguments");
  if (sched)
    if (const int rc = fleet_sched_check(h, *sched, who)) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(sched ? k_fleet_post<true> : k_fleet_post<false>, dim3(B, FLEET_CHUNKS), dim3(FLEET_BLOCK), 0,
                     (hipStream_t)stream, h->hc.N, h->hc.nx, *p, *s, sched ? *sched : ffddp_fleet_sched{}, xs, us, K, cost,
                     iters, ok, fn_pred, stats, x0, surface, tau_bias, (long)ld_tau_bias, tau_cmd, info, scale, tau_app,
                     tau_filt, lpf, obs, (long)ld_obs, log_obs, tau_lim);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_fleet_post_lim_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                             const double* xs, const double* us, const double* K, const double* cost,
                             const int32_t* iters, const uint8_t* ok, const double* fn_pred, const int32_t* stats,
                             const double* x0, const uint8_t* surface, const double* tau_bias, int ld_tau_bias,
                             double* tau_cmd, double* info, const double* scale, double* tau_app, double* tau_filt,
                             double lpf, const double* obs, int ld_obs, double* log_obs,
                             const ffddp_fleet_sched* sched, const double* tau_lim, void* stream) {
  return fleet_post(h, "ffddp_fleet_post_lim_dev", B, p, s, xs, us, K, cost, iters, ok, fn_pred, stats, x0, surface,
                    tau_bias, ld_tau_bias, tau_cmd, info, scale, tau_app, tau_filt, lpf, obs, ld_obs, log_obs, sched,
                    tau_lim, stream);
}

int ffddp_fleet_post_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                         const double* xs, const double* us, const double* K, const double* cost,
                         const int32_t* iters, const uint8_t* ok, const double* fn_pred, const int32_t* stats,
                         const double* x0, const uint8_t* surface, const double* tau_bias, int ld_tau_bias,
                         double* tau_cmd, double* info, const double* scale, double* tau_app, double* tau_filt,
                         double lpf, const double* obs, int ld_obs, double* log_obs, void* stream) {
  return fleet_post(h, "ffddp_fleet_post_dev", B, p, s, xs, us, K, cost, iters, ok, fn_pred, stats, x0, surface, tau_bias,
                    ld_tau_bias, tau_cmd, info, scale, tau_app, tau_filt, lpf, obs, ld_obs, log_obs, nullptr, nullptr,
                    stream);
}

int ffddp_fleet_post_sched_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                               const double* xs, const double* us, const double* K, const double* cost,
                               const int32_t* iters, const uint8_t* ok, const double* fn_pred, const int32_t* stats,
                               const double* x0, const uint8_t* surface, const double* tau_bias, int ld_tau_bias,
                               double* tau_cmd, double* info, const double* scale, double* tau_app, double* tau_filt,
                               double lpf, const double* obs, int ld_obs, double* log_obs, ffddp_fleet_sched sched,
                               void* stream) {
  return fleet_post(h, "ffddp_fleet_post_sched_dev", B, p, s, xs, us, K, cost, iters, ok, fn_pred, stats, x0, surface,
                    tau_bias, ld_tau_bias, tau_cmd, info, scale, tau_app, tau_filt, lpf, obs, ld_obs, log_obs, &sched,
                    nullptr, stream);
}

// per-instance tasks (ffddp_task.hpp): the sampler alone, and pre with it in place of node_ref1 / contact_hint
int ffddp_fleet_task_refs_dev(ffddp_handle* h, int B, ffddp_fleet_tasks tasks, const double* t, double* node_ref,
                              uint8_t* hint, void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_task_refs_dev: B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!tasks.rec || !t || !node_ref || !hint) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_task_refs_dev: null pointer");
  HIPCHK(h, hipSetDevice(h->device));
  const long n = (long)B * (h->hc.N + 1);
  hipLaunchKernelGGL(k_fleet_task_refs, dim3((unsigned)((n + TASK_BLOCK - 1) / TASK_BLOCK)), dim3(TASK_BLOCK), 0,
                     (hipStream_t)stream, B, h->hc.N, h->hc.dt, tasks, t, node_ref, hint);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// per-instance force setpoint profiles (ffddp_force.hpp): the solve's force_ref for this tick
int ffddp_fleet_force_refs_dev(ffddp_handle* h, int B, ffddp_fleet_tasks tasks, const double* force, int rows,
                               double fn_default, double* force_ref, void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_force_refs_dev: B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!force || !force_ref) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_force_refs_dev: null pointer");
  if (rows < 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_force_refs_dev: rows below 0");
  HIPCHK(h, hipSetDevice(h->device));
  const long n = (long)B * (h->hc.N + 1);
  hipLaunchKernelGGL(k_fleet_force_refs, dim3((unsigned)((n + FORCE_BLOCK - 1) / FORCE_BLOCK)), dim3(FORCE_BLOCK), 0,
                     (hipStream_t)stream, B, h->hc.N, h->hc.dt, tasks, force, rows, fn_default, force_ref);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_fleet_pre_task_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                             const double* q, const double* v, const double* fn_meas, const double* contact,
                             const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                             const double* q_nom, ffddp_fleet_tasks tasks, double* x0, uint8_t* surface,
                             double* inst_ref, double* node_ref, double* xs_init, double* us_init,
                             const ffddp_fleet_sched* sched, void* stream) {
  return fleet_pre(h, "ffddp_fleet_pre_task_dev", B, p, s, q, v, fn_meas, contact, ee_z, ld_qv, ld_scalar, tau_hat,
                   ld_tau_hat, q_nom, nullptr, 0, x0, surface, inst_ref, node_ref, xs_init, us_init, sched, &tasks, nullptr,
                   nullptr, stream);
}

int ffddp_fleet_pre_mdl_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                            const double* q, const double* v, const double* fn_meas, const double* contact,
                            const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                            const double* q_nom, ffddp_fleet_tasks tasks, const double* node_ref1, int contact_hint,
                            double* x0, uint8_t* surface, double* inst_ref, double* node_ref, double* xs_init,
                            double* us_init, const ffddp_fleet_sched* sched, const double* link_rows, void* stream) {
  return fleet_pre(h, "ffddp_fleet_pre_mdl_dev", B, p, s, q, v, fn_meas, contact, ee_z, ld_qv, ld_scalar, tau_hat,
                   ld_tau_hat, q_nom, node_ref1, contact_hint, x0, surface, inst_ref, node_ref, xs_init, us_init, sched,
                   tasks.rec ? &tasks : nullptr, link_rows, nullptr, stream);
}

int ffddp_fleet_pre_mnt_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                            const double* q, const double* v, const double* fn_meas, const double* contact,
                            const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                            const double* q_nom, ffddp_fleet_tasks tasks, const double* node_ref1, int contact_hint,
                            double* x0, uint8_t* surface, double* inst_ref, double* node_ref, double* xs_init,
                            double* us_init, const ffddp_fleet_sched* sched, const double* link_rows,
                            const double* mount_rows, void* stream) {
  return fleet_pre(h, "ffddp_fleet_pre_mnt_dev", B, p, s, q, v, fn_meas, contact, ee_z, ld_qv, ld_scalar, tau_hat,
                   ld_tau_hat, q_nom, node_ref1, contact_hint, x0, surface, inst_ref, node_ref, xs_init, us_init, sched,
                   tasks.rec ? &tasks : nullptr, link_rows, mount_rows, stream);
}

// a plant record per instance re-expressed in the instance's planning frame (k_fleet_obs_frame)
int ffddp_fleet_obs_frame_dev(ffddp_handle* h, int B, const double* obs, int ld_obs, const double* frame,
                              const uint8_t* sel, double* obs_out, int ld_out, void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_obs_frame_dev: B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!obs || !frame || !obs_out) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_obs_frame_dev: null pointer");
  if (ld_obs < PO_WORDS || ld_out < PO_WORDS) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_obs_frame_dev: bad stride");
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_fleet_obs_frame, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, obs, (long)ld_obs,
                     frame, sel, obs_out, (long)ld_out);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// the sweep's task metrics (ffddp_metrics.hpp): one record per instance folded into acc [W][ld]
int ffddp_fleet_metrics_dev(ffddp_handle* h, int B, int ld, const double* obs, int ld_obs, ffddp_fleet_tasks tasks,
                            int rows, double dt, const double* p_ref, double ts, const double* t_phase, double fn_des,
                            const double* info, const uint8_t* need, const int32_t* plant_fail, double* acc, void* stream) {
  return ffddp_fleet_metrics_fref_dev(h, B, ld, obs, ld_obs, tasks, rows, dt, p_ref, ts, t_phase, fn_des, info, need,
                                      plant_fail, acc, nullptr, 0, stream);
}

int ffddp_fleet_metrics_fref_dev(ffddp_handle* h, int B, int ld, const double* obs, int ld_obs, ffddp_fleet_tasks tasks,
                                 int rows, double dt, const double* p_ref, double ts, const double* t_phase,
                                 double fn_des, const double* info, const uint8_t* need, const int32_t* plant_fail,
                                 double* acc, const double* force, int rows_force, void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_metrics_dev: B must be positive");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!obs || !t_phase || !acc || (!tasks.rec && !p_ref))
    return fail(h, FFDDP_E_INVALID, "ffddp_fleet_metrics_dev: null pointer");
  if (ld < B || ld_obs < 48 || (tasks.rec && rows < 0) || (force && rows_force < 0))
    return fail(h, FFDDP_E_INVALID, "ffddp_fleet_metrics_dev: bad stride or record count");
  HIPCHK(h, hipSetDevice(h->device));
  const dim3 grid((unsigned)((B + METRICS_BLOCK - 1) / METRICS_BLOCK)), block(METRICS_BLOCK);
  if (force && tasks.rec)
    hipLaunchKernelGGL((k_fleet_metrics<true, const double*, int>), grid, block, 0, (hipStream_t)stream, B, (long)ld, obs,
                       (long)ld_obs, tasks, rows, dt, p_ref, ts, t_phase, fn_des, info, need, plant_fail, acc, force,
                       rows_force);
  else if (force)
    hipLaunchKernelGGL((k_fleet_metrics<false, const double*, int>), grid, block, 0, (hipStream_t)stream, B, (long)ld, obs,
                       (long)ld_obs, tasks, 0, dt, p_ref, ts, t_phase, fn_des, info, need, plant_fail, acc, force,
                       rows_force);
  else if (tasks.rec)
    hipLaunchKernelGGL(k_fleet_metrics<true>, grid, block, 0, (hipStream_t)stream, B, (long)ld, obs, (long)ld_obs, tasks,
                       rows, dt, p_ref, ts, t_phase, fn_des, info, need, plant_fail, acc);
  else
    hipLaunchKernelGGL(k_fleet_metrics<false>, grid, block, 0, (hipStream_t)stream, B, (long)ld, obs, (long)ld_obs, tasks,
                       0, dt, p_ref, ts, t_phase, fn_des, info, need, plant_fail, acc);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// the uncertainty injector around the tick (ffddp_inject.hpp)
static int fleet_inject_check(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const char* who) {
  if (B <= 0 || k < 0) return fail(h, FFDDP_E_INVALID, std::string(who) + ": B must be positive and k >= 0");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!inj || !inj->row || !inj->a || !inj->b || !inj->obs_ring || !inj->cmd_ring || !inj->tau_hat_filt || !inj->z_cmd)
    return fail(h, FFDDP_E_INVALID, std::string(who) + ": null pointer");
  if (inj->d_obs < 0 || inj->d_cmd < 0 || inj->rows < 0)
    return fail(h, FFDDP_E_INVALID, std::string(who) + ": a delay below 0");
  if (inj->noise != FFDDP_INJECT_NOISE_TABLE && inj->noise != FFDDP_INJECT_NOISE_PHILOX)
    return fail(h, FFDDP_E_INVALID, std::string(who) + ": unknown noise mode");
  return 0;
}

// The body of ffddp_fleet_inject_obs_dev and _obs_rows_dev (`who`: the entry point called; rows: per-row delays
// and sigmas, the ROWS instantiation)
static int fleet_inject_obs(ffddp_handle* h, const char* who, int B, const ffddp_fleet_inject* inj, int k,
                            const double* z, const double* q, const double* v, int ld_qv, const double* tau_filt,
                            double* qv_ctrl, double* tau_hat, double* tau_ctrl, const ffddp_fleet_inject_rows* rows,
                            void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (int rc = fleet_inject_check(h, B, inj, k, who)) return rc;
  if (!q || !v || !qv_ctrl || (inj->noise == FFDDP_INJECT_NOISE_TABLE ? (inj->rows > 0 && !z) : !inj->seed))
    return fail(h, FFDDP_E_INVALID, std::string(who) + ": null pointer");
  if (ld_qv < NQ) return fail(h, FFDDP_E_INVALID, std::string(who) + ": bad stride");
  HIPCHK(h, hipSetDevice(h->device));
  const int nb = (int)(((long)B * NU + INJECT_BLOCK - 1) / INJECT_BLOCK);
  if (rows)
    hipLaunchKernelGGL((k_fleet_inject_obs<true, ffddp_fleet_inject_rows>), dim3(nb), dim3(INJECT_BLOCK), 0,
                       (hipStream_t)stream, B, *inj, k, z, q, v, (long)ld_qv, tau_filt, qv_ctrl, tau_hat, tau_ctrl, *rows);
  else
    hipLaunchKernelGGL(k_fleet_inject_obs<false>, dim3(nb), dim3(INJECT_BLOCK), 0, (hipStream_t)stream, B, *inj, k, z, q,
                       v, (long)ld_qv, tau_filt, qv_ctrl, tau_hat, tau_ctrl);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// The body of ffddp_fleet_inject_cmd_dev and _cmd_rows_dev
static int fleet_inject_cmd(ffddp_handle* h, const char* who, int B, const ffddp_fleet_inject* inj, int k,
                            const double* tau_cmd, double* tau_app, const ffddp_fleet_inject_rows* rows, void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (int rc = fleet_inject_check(h, B, inj, k, who)) return rc;
  if (!tau_cmd || !tau_app) return fail(h, FFDDP_E_INVALID, std::string(who) + ": null pointer");
  HIPCHK(h, hipSetDevice(h->device));
  const int nb = (int)(((long)B * NU + INJECT_BLOCK - 1) / INJECT_BLOCK);
  if (rows)
    hipLaunchKernelGGL((k_fleet_inject_cmd<true, ffddp_fleet_inject_rows>), dim3(nb), dim3(INJECT_BLOCK), 0,
                       (hipStream_t)stream, B, *inj, k, tau_cmd, tau_app, *rows);
  else
    hipLaunchKernelGGL(k_fleet_inject_cmd<false>, dim3(nb), dim3(INJECT_BLOCK), 0, (hipStream_t)stream, B, *inj, k,
                       tau_cmd, tau_app);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int ffddp_fleet_inject_obs_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const double* z,
                               const double* q, const double* v, int ld_qv, const double* tau_filt, double* qv_ctrl,
                               double* tau_hat, double* tau_ctrl, void* stream) {
  return fleet_inject_obs(h, "ffddp_fleet_inject_obs_dev", B, inj, k, z, q, v, ld_qv, tau_filt, qv_ctrl, tau_hat,
                          tau_ctrl, nullptr, stream);
}

int ffddp_fleet_inject_cmd_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const double* tau_cmd,
                               double* tau_app, void* stream) {
  return fleet_inject_cmd(h, "ffddp_fleet_inject_cmd_dev", B, inj, k, tau_cmd, tau_app, nullptr, stream);
}

// the same two calls with per-row delays and sigmas; without any row array they are the calls above
int ffddp_fleet_inject_obs_rows_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const double* z,
                                    const double* q, const double* v, int ld_qv, const double* tau_filt,
                                    double* qv_ctrl, double* tau_hat, double* tau_ctrl,
                                    const ffddp_fleet_inject_rows* rows, void* stream) {
  if (!rows || (!rows->d_obs && !rows->d_cmd && !rows->sigma))
    return ffddp_fleet_inject_obs_dev(h, B, inj, k, z, q, v, ld_qv, tau_filt, qv_ctrl, tau_hat, tau_ctrl, stream);
  return fleet_inject_obs(h, "ffddp_fleet_inject_obs_rows_dev", B, inj, k, z, q, v, ld_qv, tau_filt, qv_ctrl, tau_hat,
                          tau_ctrl, rows, stream);
}

int ffddp_fleet_inject_cmd_rows_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k,
                                    const double* tau_cmd, double* tau_app, const ffddp_fleet_inject_rows* rows,
                                    void* stream) {
  if (!rows || (!rows->d_obs && !rows->d_cmd && !rows->sigma))
    return ffddp_fleet_inject_cmd_dev(h, B, inj, k, tau_cmd, tau_app, stream);
  return fleet_inject_cmd(h, "ffddp_fleet_inject_cmd_rows_dev", B, inj, k, tau_cmd, tau_app, rows, stream);
}

int ffddp_fleet_noise_dev(ffddp_handle* h, int B, const uint64_t* seed, int k, double* z, uint64_t* words,
                          void* stream) {
  if (!h) return FFDDP_E_INVALID;
  if (B <= 0 || k < 0) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_noise_dev: B must be positive and k >= 0");
  if (B > h->max_batch) return fail(h, FFDDP_E_CAPACITY, "B exceeds max_batch");
  if (!seed || !z) return fail(h, FFDDP_E_INVALID, "ffddp_fleet_noise_dev: null pointer");
  HIPCHK(h, hipSetDevice(h->device));
  const int nb = (int)(((long)B * NU + INJECT_BLOCK - 1) / INJECT_BLOCK);
  hipLaunchKernelGGL(k_fleet_noise, dim3(nb), dim3(INJECT_BLOCK), 0, (hipStream_t)stream, B, seed, k, z, words);
  HIPCHK(h, hipGetLastError());
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// plant stand-in
// ---------------------------------------------------------------------------
struct ffddp_plant {
  int device = 0, max_batch = 0;
  ffddp_robot* drb = nullptr;
  ffddp_plant_params* dpp = nullptr;
  double *q = nullptr, *v = nullptr, *tau = nullptr, *plane = nullptr, *obs = nullptr;
  int32_t* fail = nullptr;
  // per-instance physics (ffddp_plant_set_instance_params): field-major [FFDDP_PLANT_ROW_W][max_batch], allocated
  // by the first call; n_rows > 0: the rows are in force
  double* rows = nullptr;
  int n_rows = 0;
  // per-instance link models (ffddp_plant_set_instance_links): field-major [PLANT_LINK_USED][max_batch], allocated
  // by the first call; n_links > 0: the rows are in force
  double* links = nullptr;
  int n_links = 0;
};

extern "C" {

int ffddp_plant_create(const ffddp_robot* robot, const ffddp_plant_params* p, int device, int max_batch,
                       ffddp_plant** out) {
  static_assert(PO_WORDS == FFDDP_PLANT_OBS, "plant observation layout");
  if (!robot || !p || !out || max_batch < 1 || p->timestep <= 0.0 || p->n_substeps < 1) return FFDDP_E_INVALID;
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return FFDDP_E_DEVICE;
  ffddp_plant* h = new (std::nothrow) ffddp_plant();
  if (!h) return FFDDP_E_OOM;
  h->device = device;
  h->max_batch = max_batch;
  const size_t B = (size_t)max_batch;
  bool bad_alloc = hipMalloc((void**)&h->drb, sizeof(ffddp_robot)) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->dpp, sizeof(ffddp_plant_params)) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->q, B * NQ * 8) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->v, B * NQ * 8) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->tau, B * NQ * 8) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->plane, B * 6 * 8) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->obs, B * PO_WORDS * 8) != hipSuccess;
  bad_alloc |= hipMalloc((void**)&h->fail, B * 4) != hipSuccess;
  if (bad_alloc || hipMemcpy(h->drb, robot, sizeof(ffddp_robot), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->dpp, p, sizeof(ffddp_plant_params), hipMemcpyHostToDevice) != hipSuccess) {
    ffddp_plant_destroy(h);
    return bad_alloc ? FFDDP_E_OOM : FFDDP_E_DEVICE;
  }
  *out = h;
  return 0;
}

void ffddp_plant_destroy(ffddp_plant* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  void* ps[] = {h->drb, h->dpp, h->q, h->v, h->tau, h->plane, h->obs, h->fail, h->rows, h->links};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  delete h;
}

int ffddp_plant_step_dev(ffddp_plant* h, int B, double* q, double* v, const double* tau, const double* plane,
                         int integrate, double* obs, int32_t* fail, void* stream) {
  if (!h || B < 0 || B > h->max_batch) return FFDDP_E_INVALID;
  if (B == 0) return 0;
  if (!q || !v || !tau || !plane || !obs) return FFDDP_E_INVALID;
  if (h->n_rows > 0 && B > h->n_rows) return FFDDP_E_INVALID;
  if (h->n_links > 0 && B > h->n_links) return FFDDP_E_INVALID;
  if (hipSetDevice(h->device) != hipSuccess) return FFDDP_E_DEVICE;
  const PlantLinks lk = {h->links, (long)h->max_batch};
  if (h->n_links > 0 && h->n_rows > 0)
    hipLaunchKernelGGL((k_plant<true, const double*, long, PlantLinks>), dim3((B + 63) / 64), dim3(64), 0,
                       (hipStream_t)stream, h->drb, h->dpp, B, q, v, tau, plane, integrate, obs, fail, h->rows,
                       (long)h->max_batch, lk);
  else if (h->n_links > 0)
    hipLaunchKernelGGL((k_plant<false, PlantLinks>), dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->drb,
                       h->dpp, B, q, v, tau, plane, integrate, obs, fail, lk);
  else if (h->n_rows > 0)
    hipLaunchKernelGGL((k_plant<true, const double*, long>), dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       h->drb, h->dpp, B, q, v, tau, plane, integrate, obs, fail, h->rows, (long)h->max_batch);
  else
    hipLaunchKernelGGL(k_plant<false>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->drb, h->dpp, B, q, v,
                       tau, plane, integrate, obs, fail);
  return hipGetLastError() == hipSuccess ? 0 : FFDDP_E_DEVICE;
}

// a physics row the plant can integrate with (include/ffddp.h: ffddp_plant_set_instance_params)
static bool plant_row_valid(const double* r) {
  for (int i = 0; i < FFDDP_PLANT_ROW_W; ++i)
    if (!std::isfinite(r[i])) return false;
  for (int i = 0; i < NQ; ++i)
    if (r[FFDDP_PLANT_ROW_ARMATURE + i] < 0.0 || r[FFDDP_PLANT_ROW_DAMPING + i] < 0.0) return false;
  const double* sr = r + FFDDP_PLANT_ROW_SOLREF;
  const double* si = r + FFDDP_PLANT_ROW_SOLIMP;
  if (r[FFDDP_PLANT_ROW_R_TOOL] <= 0.0 || sr[0] <= 0.0 || sr[1] <= 0.0) return false;
  if (si[0] <= 0.0 || si[0] >= 1.0 || si[1] <= 0.0 || si[1] >= 1.0 || si[1] < si[0]) return false;
  return si[3] > 0.0 && si[3] < 1.0 && si[4] >= 1.0;
}

int ffddp_plant_set_instance_params(ffddp_plant* h, int n, const double* rows) {
  static_assert(FFDDP_PLANT_ROW_SOLIMP + 5 == FFDDP_PLANT_ROW_W, "plant physics row layout");
  if (!h) return FFDDP_E_INVALID;
  if (!rows) {  // back to the handle's struct; steps already enqueued keep the copy they were launched with
    h->n_rows = 0;
    return 0;
  }
  if (n < 1 || n > h->max_batch) return FFDDP_E_INVALID;
  for (int b = 0; b < n; ++b)
    if (!plant_row_valid(rows + (size_t)b * FFDDP_PLANT_ROW_W)) return FFDDP_E_INVALID;
  const size_t ld = (size_t)h->max_batch;
  std::vector<double> t(ld * FFDDP_PLANT_ROW_W, 0.0);  // row-major -> field-major
  for (int b = 0; b < n; ++b)
    for (int f = 0; f < FFDDP_PLANT_ROW_W; ++f) t[(size_t)f * ld + b] = rows[(size_t)b * FFDDP_PLANT_ROW_W + f];
  if (hipSetDevice(h->device) != hipSuccess) return FFDDP_E_DEVICE;
  if (!h->rows && hipMalloc((void**)&h->rows, t.size() * 8) != hipSuccess) {
    h->rows = nullptr;
    return FFDDP_E_OOM;
  }
  // steps in flight read the copy: wait for them, then replace it
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(h->rows, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return FFDDP_E_DEVICE;
  h->n_rows = n;
  return 0;
}

int ffddp_plant_set_instance_links(ffddp_plant* h, int n, const double* link_rows) {
  if (!h) return FFDDP_E_INVALID;
  if (!link_rows) {  // back to the handle's robot; steps already enqueued keep the copy they were launched with
    h->n_links = 0;
    return 0;
  }
  if (n < 1 || n > h->max_batch) return FFDDP_E_INVALID;
  // what ffddp_link_model_rows refuses; the padding entries are not looked at
  for (int b = 0; b < n; ++b) {
    const double* r = link_rows + (size_t)b * FFDDP_LINK_W;
    for (int j = 0; j < NQ; ++j) {
      if (!(std::isfinite(r[16 * j]) && r[16 * j] > 0.0)) return FFDDP_E_INVALID;
      for (int k = 1; k < PLANT_LINK_PER_JOINT; ++k)
        if (!std::isfinite(r[16 * j + k])) return FFDDP_E_INVALID;
    }
  }
  const size_t ld = (size_t)h->max_batch;
  std::vector<double> t(ld * PLANT_LINK_USED, 0.0);  // row-major -> field-major over the used entries
  for (int b = 0; b < n; ++b)
    for (int j = 0; j < NQ; ++j)
      for (int k = 0; k < PLANT_LINK_PER_JOINT; ++k)
        t[(size_t)(PLANT_LINK_PER_JOINT * j + k) * ld + b] = link_rows[(size_t)b * FFDDP_LINK_W + 16 * j + k];
  if (hipSetDevice(h->device) != hipSuccess) return FFDDP_E_DEVICE;
  if (!h->links && hipMalloc((void**)&h->links, t.size() * 8) != hipSuccess) {
    h->links = nullptr;
    return FFDDP_E_OOM;
  }
  // steps in flight read the copy: wait for them, then replace it
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(h->links, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return FFDDP_E_DEVICE;
  h->n_links = n;
  return 0;
}

int ffddp_plant_step(ffddp_plant* h, int B, double* q, double* v, const double* tau, const double* plane,
                     int integrate, double* obs) {
  if (!h || B < 0 || B > h->max_batch) return FFDDP_E_INVALID;
  if (B == 0) return 0;
  if (!q || !v || !tau || !plane || !obs) return FFDDP_E_INVALID;
  if (hipSetDevice(h->device) != hipSuccess) return FFDDP_E_DEVICE;
  const size_t n7 = (size_t)B * NQ * 8;
  if (hipMemcpy(h->q, q, n7, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->v, v, n7, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->tau, tau, n7, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->plane, plane, (size_t)B * 6 * 8, hipMemcpyHostToDevice) != hipSuccess)
    return FFDDP_E_DEVICE;
  int rc = ffddp_plant_step_dev(h, B, h->q, h->v, h->tau, h->plane, integrate, h->obs, h->fail, nullptr);
  if (rc) return rc;
  std::vector<int32_t> fl((size_t)B);
  if (hipMemcpy(q, h->q, n7, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(v, h->v, n7, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(obs, h->obs, (size_t)B * PO_WORDS * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(fl.data(), h->fail, (size_t)B * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return FFDDP_E_DEVICE;
  for (int b = 0; b < B; ++b)
    if (fl[b]) return FFDDP_E_INVALID;
  return 0;
}

}  // extern "C"
