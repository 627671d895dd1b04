/*
 * ffddp.h — C-ABI of the MI355X-native batched (Box)FDDP solver.
 *
 * Drop-in boundary for the reference's hot path
 *     ok = solver.solve(xs_init, us_init, max_iters, False)
 * at src/mpc/crocoddyl_classical.py:367 (ClassicalCrocoddylMPC) and
 * src/mpc/crocoddyl_force_feedback.py:605 (ForceFeedbackCrocoddylMPC), where
 * `solver` is crocoddyl.SolverBoxFDDP(problem) (crocoddyl_classical.py:442-445)
 * over the ShootingProblem built by _build_problem (:521-556 / FF :776-836).
 * The reference binds Crocoddyl through boost-python; this library is bound
 * through ctypes (ffddp._abi) and through a pybind11 module over the same
 * entry points (csrc/ffddp_pybind.cpp).  Plain pointers
 * and sizes only.
 *
 * Conventions
 *   - fp64 everywhere; all matrices row-major.
 *   - One handle = one OCP definition (robot + weights + horizon + variant),
 *     bound to one HIP device.  A handle is not thread-safe.  Handles on the
 *     same device share one pool of slice streams (and the null stream), so
 *     solves of two handles driven from two threads are correct but
 *     serialise on the GPU rather than overlap.
 *   - Return 0 on success or a negative FFDDP_E* code for API / launch / OOM
 *     errors.  Per-instance numerical failure is reported in ok[b] = 0 (the
 *     cost may be NaN), exactly like Crocoddyl's solve() returning False.
 *   - No C++ exception crosses this boundary.
 */
#ifndef FFDDP_H_
#define FFDDP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFDDP_NQ 7      /* Panda arm joints (fingers locked, crocoddyl_classical.py:189-197) */
#define FFDDP_NU 7      /* ActuationModelFull: nu = nv (:147) */
#define FFDDP_MAX_NC 3  /* ContactModel1D (nc=1) or ContactModel3D (nc=3) */
#define FFDDP_NSTATS 10 /* per-instance counters returned by the solve */
#define FFDDP_NKERNELS 8 /* kernel classes reported by ffddp_profile_read */

enum {
  FFDDP_OK = 0,
  FFDDP_E_INVALID = -1,  /* bad argument (sizes, null pointers, config) */
  FFDDP_E_DEVICE = -2,   /* HIP runtime / launch error */
  FFDDP_E_OOM = -3,      /* device allocation failed */
  FFDDP_E_CAPACITY = -4  /* B larger than the handle's max_batch */
};

enum { FFDDP_CLASSICAL = 0, FFDDP_FORCE_FEEDBACK = 1 };

/* Rigid-body model of the 7-DoF arm: revolute-z joints in a serial chain.
 * Replaces example_robot_data.load("panda") + pin.buildReducedModel
 * (crocoddyl_classical.py:137-145, 189-197). */
typedef struct ffddp_robot {
  double joint_R[FFDDP_NQ][9]; /* placement of joint i in its parent (rotation) */
  double joint_p[FFDDP_NQ][3]; /* placement of joint i in its parent (translation) */
  double mass[FFDDP_NQ];
  double com[FFDDP_NQ][3];     /* COM in the link frame */
  double inertia[FFDDP_NQ][9]; /* rotational inertia about the COM, link frame */
  double ee_R[9];              /* EE frame ("panda_link8") in link 7 */
  double ee_p[3];
  double gravity[3];           /* world gravity, (0,0,-9.81) */
} ffddp_robot;

/* OCP definition: every field the reference's _build_problem/_make_dam reads
 * from ClassicalMPCConfig / ForceFeedbackMPCConfig
 * (crocoddyl_classical.py:12-110, 521-728; crocoddyl_force_feedback.py:12-146,
 * 149-290, 776-1009).  Costs with weight 0 are not added (as in the reference). */
typedef struct ffddp_ocp_config {
  int32_t variant;      /* FFDDP_CLASSICAL (nx=14) or FFDDP_FORCE_FEEDBACK (nx=21) */
  int32_t horizon;      /* N running nodes + 1 terminal node */
  int32_t nc;           /* 1 = ContactModel1D normal_1d, 3 = ContactModel3D point3d */
  int32_t use_box;      /* 1 = SolverBoxFDDP (default), 0 = SolverFDDP */
  double dt;            /* dt_ocp */
  double z_press;
  double w_ee_pos, w_ee_ori;
  double ori_weights[3];
  double w_posture, w_v;
  double v_damp_weights[7];
  double w_tau, w_tau_soft_limits, tau_soft_limit_margin;
  double w_q_soft_limits, q_soft_limit_margin;
  double q_lower[7], q_upper[7];
  double w_tangent_pos, w_tangent_vel, w_plane_z, w_vz;
  /* fn_des: the desired normal contact force of the fn_track cost (weight w_fn),
   * one scalar for every instance and node; ffddp_solve_batch_fref_dev replaces
   * it per instance and node with its force_ref array */
  double w_unilateral, friction_margin, w_fn, fn_des;
  double w_wdamp;
  double w_wdamp_weights[3];
  double contact_gains[2];   /* Baumgarte [Kp, Kd] */
  double contact_inv_damping;/* JMinvJt_damping */
  double tau_limits[7];      /* u_lb = -tau_limits, u_ub = +tau_limits */
  double R_des[9];           /* FrameRotation reference, Pinocchio world */
  /* force-feedback augmentation (_AugmentedLPFActionModel) */
  double ff_alpha;           /* tau_{k+1} = alpha tau_k + (1-alpha) w_k */
  double w_w, w_w_soft_limits, w_y;
  double y_weights[21];
  int32_t use_inner_state_reg, use_inner_tau_reg;
  /* friction cone, built only for nc = 3 (crocoddyl_classical.py:678-687; FF
   * crocoddyl_force_feedback.py:959-966): ResidualModelContactFrictionCone over
   * crocoddyl.FrictionCone(I, mu, nf = 4, inner = False)
   * (crocoddyl_classical.py:999-1018, crocoddyl_force_feedback.py:1428-1447)
   * with a QuadraticBarrier narrowed by friction_margin (:891-903), weight
   * w_friction_cone */
  double w_friction_cone, mu;
} ffddp_ocp_config;

/* Task description for the device-side problem builder:
 * the approach-then-circle EE reference of src/tasks/trajectories.py:8-93
 * with the benchmark runner's contact-onset hold (run_classical.py:221-264),
 * the MuJoCo->Pinocchio target mapping (crocoddyl_classical.py:250-258) and
 * the posture / torque reference modes (crocoddyl_classical.py:447-466). */
typedef struct ffddp_task {
  double center[3];   /* circle centre, MuJoCo world (z = contact height) */
  double radius, omega, z_contact, t_approach, t_pre;
  double z_pre;       /* used when has_z_pre, else max(z_contact + 0.05, ee_start z) */
  double t_hold;      /* benchmark hold at contact onset (0.2 s; 0 = none) */
  double ee_start[3]; /* used when has_ee_start, else contact start + (0, 0, 0.08) */
  int32_t has_ee_start, has_z_pre;
  double p_site_minus_frame[3]; /* _calibrate_site_position_offset (Pinocchio frame) */
  double q_nom[7];
  int32_t posture_mode; /* 0: x_reg_ref = x0[:14]; 1: [q_nom, 0] */
  int32_t torque_mode;  /* 0: gravity(x0 q); 1: gravity(q_nom); 2: zero */
} ffddp_task;

typedef struct ffddp_handle ffddp_handle;

/* crocoddyl.SolverBoxFDDP(problem) / setProblem (crocoddyl_classical.py:350-361):
 * allocates device workspace for up to max_batch instances. */
int ffddp_create(const ffddp_robot* robot, const ffddp_ocp_config* cfg, int device,
                 int max_batch, ffddp_handle** out);
void ffddp_destroy(ffddp_handle* h);
const char* ffddp_last_error(const ffddp_handle* h);

/* Batched solver.solve(xs_init, us_init, maxiter, is_feasible)
 * (crocoddyl_classical.py:365-388, crocoddyl_force_feedback.py:603-628).
 * Host pointers, row-major:
 *   x0       [B][nx]           problem.x0 (FF: y0 = [q, v, tau_hat])
 *   node_ref [B][N+1][6]       p_ref, v_ref per node, Pinocchio world (:526-546)
 *   inst_ref [B][21]           x_reg_ref (14), tau_ref (7)           (:523-524)
 *   surface  [B]               0 free-space DAM, 1 contact DAM       (:533, 614)
 *   xs_init  [B][N+1][nx], us_init [B][N][7]                         (:365)
 * Outputs (solver.xs, solver.us, solver.K, solver.cost, solver.iter, ok):
 *   xs [B][N+1][nx], us [B][N][7], K [B][N][7][nx], cost [B], iters [B], ok [B]
 *   fn_pred [B][2]   contact lambda_normal at knots 0 and 1 of the solution
 *                    (crocoddyl_classical.py:905-942, FF :1219-1299; NaN if free)
 *   stats  [B][FFDDP_NSTATS]  (optional, may be NULL) per instance:
 *                    [0] FDDP iterations with a successful backward pass,
 *                    [1] line-search trials a sequential solver executes,
 *                    [2] regularisation retries of the backward pass,
 *                    [3] backward passes run, [4] calcDiff evaluations,
 *                    [5] line-search kernel launches that processed the
 *                    instance (first pass + second pass when it ran),
 *                    [6] / [7] step lengths evaluated by the first / second
 *                    line-search pass — for the roofline byte count
 *                    (SURVEY.md §8(d)),
 *                    [8] / [9] line-search trials judged / accepted by the
 *                    ascent-direction branch (dVexp < 0, see
 *                    ffddp_solver_params.neg_step_rule). */
int ffddp_solve_batch(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                      const double* inst_ref, const uint8_t* surface, const double* xs_init,
                      const double* us_init, int maxiter, int is_feasible, double* xs, double* us,
                      double* K, double* cost, int32_t* iters, uint8_t* ok, double* fn_pred,
                      int32_t* stats);

/* Same with DEVICE pointers (inputs resident in HBM) on `stream` (hipStream_t,
 * NULL = default stream).  Asynchronous: the caller synchronises the stream.
 * xs / us / K are the solver's working storage during the solve (it iterates
 * in them; no copy follows the last kernel): they must not overlap the other
 * inputs, except xs_init == xs and us_init == us (warm start in place). */
int ffddp_solve_batch_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                          const double* inst_ref, const uint8_t* surface, const double* xs_init,
                          const double* us_init, int maxiter, int is_feasible, double* xs,
                          double* us, double* K, double* cost, int32_t* iters, uint8_t* ok,
                          double* fn_pred, int32_t* stats, void* stream);

/* ffddp_solve_batch_dev for a subset of the batch: `active` is [B] device
 * bytes, instance b solves iff active[b] != 0; NULL selects every instance
 * (ffddp_solve_batch_dev is this call with NULL: same launches, same bits).
 * For an unselected instance the solve reads none of its xs_init / us_init
 * rows and writes none of its rows of xs, us, K, cost, iters, ok, fn_pred,
 * stats (its x0, node_ref, inst_ref, surface rows are not read either); its
 * part of the handle's workspace is left stale.  A selected instance's
 * outputs are the bits the unmasked call gives it (stats [5..7] count
 * line-search passes, which follow the slice's active count as they do
 * across batch sizes; they agree whenever the first pass already takes
 * every step length, as it does for small batches).  The first active list is
 * the selected instances in ascending order, a function of the mask alone.
 * The grids stay sized by the batch: blocks beyond the selected count exit at
 * once, as in a late iteration.  An all-zero mask is legal (returns 0, writes
 * nothing).  Errors, the trace, the per-kernel profile and the in-place rule
 * (xs_init == xs, us_init == us) are ffddp_solve_batch_dev's.  The
 * host-pointer entry point and solve plans take no mask. */
int ffddp_solve_batch_sel_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, void* stream);

/* ffddp_solve_batch_sel_dev with a desired normal contact force per instance
 * and node: force_ref is [B][N+1] device doubles, entry [b][t] replaces the
 * configuration's scalar fn_des in the fn_track cost of instance b at node t
 * (the component r = 0 for normal_1d, r = 2 for point3d; the tangential
 * references stay 0), in the node stage and in the line-search rollout alike.
 * The classical terminal node, whose contact force is 0, keeps its constant
 * term with force_ref[b][N].  A free-space instance (surface[b] == 0) has no
 * such cost: its results do not depend on its row.  Rows of unselected
 * instances are not read; `active` may be NULL.  The arithmetic is the scalar
 * path's in order and grouping, so an array filled with fn_des gives the bits
 * of the call without one.  force_ref == NULL is ffddp_solve_batch_sel_dev:
 * same kernels, same bits.  FFDDP_E_INVALID (with a message) when force_ref is
 * given and the handle's w_fn <= 0, which has no fn_track cost to steer; the
 * other errors are ffddp_solve_batch_sel_dev's.  The host-pointer entry point
 * and solve plans take no force reference. */
int ffddp_solve_batch_fref_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                               const double* inst_ref, const uint8_t* surface, const double* xs_init,
                               const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                               double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                               const uint8_t* active, const double* force_ref, void* stream);

/* ffddp_solve_batch_fref_dev with the scalar cost weights per instance:
 * cost_w is [B][FFDDP_COST_W] device doubles, row b the weights of instance b,
 * one named entry per scalar cost weight of ffddp_ocp_config (FFDDP_CW_<NAME>
 * is the entry of w_<name>).  A row is 32 doubles (256 bytes), so with cost_w
 * on a 128-byte boundary every row starts on one and each of its two blocks
 * lies in one 128-byte line: entries 0..9 are the frame and contact weights
 * (read by a node's end-effector lane), entries FFDDP_CW_JOINT0.. the state,
 * control and force-feedback weights (read by its joint lanes); the remaining
 * entries are padding, which the library may load and never uses.
 *
 * Which terms exist stays the handle's: a row entry replaces the weight of a
 * term the configuration builds (weight > 0 there, and the free-space /
 * contact split, use_inner_state_reg / use_inner_tau_reg, nc as before); the
 * entry of a term it does not build never enters the arithmetic (the node
 * stage does not load it; the line search loads each block whole and ignores
 * it), so any value there, NaN included, changes nothing.  An entry of
 * 0 for an existing term is legal: the term contributes zeros.  Entries must
 * be finite and >= 0; the rows are device memory, which the library cannot
 * check.  The weight vectors (ori_weights, v_damp_weights, y_weights, ...),
 * the activation bounds and margins, fn_des (per node through force_ref), the
 * contact gains, tau_limits (per instance through ffddp_solve_batch_lim_dev)
 * and the solver constants stay the handle's.
 *
 * Only the source of each weight changes, not the order or grouping of the
 * arithmetic, and the terminal node uses the same row: rows that repeat the
 * handle's configuration give the bits of the call without cost_w.  Rows of
 * unselected instances are not read (NaN there is harmless).  `active` and
 * force_ref stay optional and combine freely with cost_w (without a
 * force_ref the solve reads an array of fn_des the handle keeps, allocated
 * by the first such call).  cost_w == NULL is ffddp_solve_batch_fref_dev:
 * same kernels, same bits.  Errors are ffddp_solve_batch_fref_dev's.  The
 * host-pointer entry point and solve plans take no cost weights. */
#define FFDDP_COST_W 32
#define FFDDP_CW_EE_ORI 0
#define FFDDP_CW_WDAMP 1
#define FFDDP_CW_EE_POS 2
#define FFDDP_CW_TANGENT_POS 3
#define FFDDP_CW_TANGENT_VEL 4
#define FFDDP_CW_PLANE_Z 5
#define FFDDP_CW_VZ 6
#define FFDDP_CW_UNILATERAL 7
#define FFDDP_CW_FN 8
#define FFDDP_CW_FRICTION_CONE 9
#define FFDDP_CW_JOINT0 16 /* first entry of the joint lanes' block */
#define FFDDP_CW_POSTURE 16
#define FFDDP_CW_V 17
#define FFDDP_CW_Q_SOFT_LIMITS 18
#define FFDDP_CW_TAU 19
#define FFDDP_CW_TAU_SOFT_LIMITS 20
#define FFDDP_CW_Y 21
#define FFDDP_CW_W 22
#define FFDDP_CW_W_SOFT_LIMITS 23
int ffddp_solve_batch_wts_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w, void* stream);

/* ffddp_solve_batch_wts_dev with the torque limits per instance: tau_lim is
 * [B][FFDDP_TAU_LIM_W] device doubles, row b what the OCP of instance b derives
 * from its own tau_limits.  A row is 32 doubles (256 bytes), joint-major, so
 * that joint j's values are one aligned 32-byte read of its lane:
 *     4j + 0   u_ub[j]   = tau_limits[j]         the BoxQP bound, the rollout's clamp
 *     4j + 1   ts_ub[j]  = tau_limits[j] - mg    the torque soft-limit barrier's bound
 *     4j + 2   ws_lim[j]                         the force-feedback w soft limit
 *     4j + 3, 28..31     padding, which the library may load and never uses
 * mg is the configuration's tau_soft_limit_margin clamped below the instance's
 * smallest limit.  The lower bounds are the exact negations and the kernels
 * form them so.  ffddp_torque_limit_rows builds rows on the host with the code
 * that fills the handle's constants, so rows of the configuration's limits
 * give the bits of the call without tau_lim.
 *
 * Which terms exist stays the handle's (use_box, w_tau_soft_limits > 0,
 * w_w_soft_limits > 0, the variant): the entry of a term the handle does not
 * build never enters the arithmetic, so any value there, NaN included, changes
 * nothing.  Rows of unselected instances are not read.  `active`, force_ref
 * and cost_w stay optional and combine freely with tau_lim (without cost_w the
 * solve reads rows of the configuration's weights that the handle keeps,
 * allocated by the first such call; likewise fn_des without a force_ref).
 * tau_lim == NULL is ffddp_solve_batch_wts_dev: same kernels, same bits.
 * Errors are ffddp_solve_batch_wts_dev's.  The bounds' margins, the weights
 * and the solver constants stay the handle's; the host-pointer entry point and
 * solve plans take no limits. */
#define FFDDP_TAU_LIM_W 32
int ffddp_solve_batch_lim_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w,
                              const double* tau_lim, void* stream);

/* Host function: rows [B][FFDDP_TAU_LIM_W] for ffddp_solve_batch_lim_dev /
 * ffddp_fleet_post_lim_dev from tau_limits [B][7] and cfg's
 * tau_soft_limit_margin (the only field read).  FFDDP_E_INVALID for a null
 * pointer, B < 0, or a limit that is not finite and > 0. */
int ffddp_torque_limit_rows(const ffddp_ocp_config* cfg, int B, const double* tau_limits, double* rows);

/* ffddp_solve_batch_lim_dev with the controller's rigid-body model per
 * instance: link_rows is [B][FFDDP_LINK_W] device doubles, row b the inertial
 * parameters instance b plans with.  A row is 128 doubles (1 KiB), joint-major,
 * so that the 13 values a joint lane needs sit in one 128-byte line:
 *     16j + 0          mass[j]
 *     16j + 1 .. 3     com[j]                 in the link frame
 *     16j + 4 .. 12    inertia[j], row-major  all nine entries, as ffddp_robot
 *                                             holds them (nothing is symmetrised)
 *     16j + 13 .. 15, 112 .. 127   padding, which the library never reads
 * ffddp_link_model_rows packs ffddp_robot structs into rows, so a row of the
 * handle's robot gives the bits of the call without link_rows.  The kinematic
 * parameters (joint placements, the EE offset, gravity) stay the handle's.
 *
 * Rows of unselected instances are not read.  `active`, force_ref, cost_w and
 * tau_lim stay optional and combine freely with link_rows (without tau_lim the
 * solve reads rows of the configuration's limits that the handle keeps,
 * allocated by the first such call; likewise the configuration's weights
 * without cost_w and fn_des without a force_ref).  link_rows == NULL is
 * ffddp_solve_batch_lim_dev: same kernels, same bits.  Errors are
 * ffddp_solve_batch_lim_dev's.  The torque reference inst_ref[14..20] is the
 * caller's: ffddp_gravity_torque_mdl_dev gives it under each instance's model.
 * The host-pointer entry point, solve plans and ffddp_build_problem_dev take no
 * rows. */
#define FFDDP_LINK_W 128
int ffddp_solve_batch_mdl_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w,
                              const double* tau_lim, const double* link_rows, void* stream);

/* Host function: rows [B][FFDDP_LINK_W] for ffddp_solve_batch_mdl_dev,
 * ffddp_calc_diff_mdl, ffddp_gravity_torque_mdl_dev and ffddp_fleet_pre_mdl_dev
 * from the mass, com and inertia of B robots (the only fields read); padding
 * is zero.  FFDDP_E_INVALID for a null pointer, B < 0, a mass that is not
 * finite and > 0, or a com or inertia entry that is not finite. */
int ffddp_link_model_rows(const ffddp_robot* robots, int B, double* rows);

/* ffddp_solve_batch_mdl_dev with the arm's base mounting and the gravity
 * vector per instance: mount_rows is [B][FFDDP_MOUNT_W] device doubles, row b
 * what instance b plans with, in the solve's (Pinocchio) world.  A row is 16
 * doubles (128 bytes, one cache line):
 *     0 .. 8     base_R, row-major   in place of ffddp_robot.joint_R[0]
 *     9 .. 11    base_p              in place of ffddp_robot.joint_p[0]
 *     12 .. 14   gravity             in place of ffddp_robot.gravity
 *     15         padding, which the library never reads
 * ffddp_mount_rows packs ffddp_robot structs into rows, so a row of the
 * handle's robot gives the bits of the call without mount_rows.  base_R must
 * be a rotation; the library does not check it.  Joint placements 1..6 and
 * the EE offset stay the handle's.
 *
 * Planning in a frame M with pose x_W = R x_M + p of the unchanged physical
 * system is the same problem with base_R = R^T joint_R[0], base_p =
 * R^T (joint_p[0] - p) and gravity = R^T gravity, and with the references in M
 * (the contact normal, the tangential and plane costs are M-aligned by
 * construction).  A physically re-mounted arm changes the placement and keeps
 * the gravity.
 *
 * Rows of unselected instances are not read.  `active`, force_ref, cost_w,
 * tau_lim and link_rows stay optional and combine freely with mount_rows
 * (without link_rows the solve reads rows of the handle's robot that the
 * handle keeps, allocated by the first such call; likewise the limits, weights
 * and fn_des).  mount_rows == NULL is ffddp_solve_batch_mdl_dev: same kernels,
 * same bits.  Errors are ffddp_solve_batch_mdl_dev's.  The torque reference
 * inst_ref[14..20] is the caller's: ffddp_gravity_torque_mnt_dev gives it under
 * each instance's mount.  The host-pointer entry point, solve plans and
 * ffddp_build_problem_dev take no rows. */
#define FFDDP_MOUNT_W 16
int ffddp_solve_batch_mnt_dev(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                              const double* inst_ref, const uint8_t* surface, const double* xs_init,
                              const double* us_init, int maxiter, int is_feasible, double* xs, double* us, double* K,
                              double* cost, int32_t* iters, uint8_t* ok, double* fn_pred, int32_t* stats,
                              const uint8_t* active, const double* force_ref, const double* cost_w,
                              const double* tau_lim, const double* link_rows, const double* mount_rows, void* stream);

/* Host function: rows [B][FFDDP_MOUNT_W] for ffddp_solve_batch_mnt_dev,
 * ffddp_calc_diff_mnt, ffddp_gravity_torque_mnt_dev and ffddp_fleet_pre_mnt_dev
 * from joint_R[0], joint_p[0] and gravity of B robots (the only fields read,
 * plain copies); padding is zero.  FFDDP_E_INVALID for B < 0, for a null
 * pointer with B > 0, or for an entry that is not finite; B == 0 reads and
 * writes nothing and returns 0 whatever the pointers are, as
 * ffddp_link_model_rows does. */
int ffddp_mount_rows(const ffddp_robot* robots, int B, double* rows);

/* Solve plan for a receding-horizon loop: one solve of a fixed batch per
 * control tick (crocoddyl_classical.py:367 called every tick at
 * run_classical.py:412).  ffddp_plan_create captures the whole host-array
 * solve once as a HIP graph -- one copy of the packed inputs up, every kernel
 * of maxiter iterations, one copy of the packed outputs down -- and
 * ffddp_plan_run replays it and waits: one graph launch per tick instead of
 * ~50 kernel launches and 14 copies.  The plan owns page-locked input and
 * output arrays (the ffddp_solve_batch arguments, same layouts), returned in
 * *io: refill the inputs in place before each run, read the outputs after it
 * (overwritten by the next run).  Results equal ffddp_solve_batch's bit for
 * bit.  The solver properties (ffddp_set_solver_params) apply to later runs;
 * tracing and per-kernel timing are fixed at creation (timing off):
 * ffddp_trace_enable returns FFDDP_E_INVALID while a plan of the handle is
 * alive.  A plan uses its handle's workspace.  ffddp_plan_run first waits (on
 * the device) for the handle's last solve_batch[_dev] call to finish, on
 * whatever stream it ran; do not run a plan from a second host thread while
 * another solve of the same handle is being enqueued.  ffddp_destroy
 * invalidates the handle's live plans: their ffddp_plan_run then returns
 * FFDDP_E_INVALID, and ffddp_plan_destroy still frees them (their io arrays
 * stay valid until then). */
typedef struct ffddp_plan ffddp_plan;
typedef struct ffddp_plan_io {
  double* x0;        /* [B][nx]        inputs, written by the caller */
  double* node_ref;  /* [B][N+1][6] */
  double* inst_ref;  /* [B][21] */
  uint8_t* surface;  /* [B] */
  double* xs_init;   /* [B][N+1][nx] */
  double* us_init;   /* [B][N][7] */
  const double* xs;  /* [B][N+1][nx]  outputs of the last run */
  const double* us;  /* [B][N][7] */
  const double* K;   /* [B][N][7][nx] */
  const double* cost;
  const int32_t* iters;
  const uint8_t* ok;
  const double* fn_pred; /* [B][2] */
  const int32_t* stats;  /* [B][FFDDP_NSTATS] */
} ffddp_plan_io;
int ffddp_plan_create(ffddp_handle* h, int B, int maxiter, int is_feasible, ffddp_plan** out, ffddp_plan_io* io);
int ffddp_plan_run(ffddp_plan* p);
void ffddp_plan_destroy(ffddp_plan* p);

/* problem.calcDiff(xs, us) on the device (ShootingProblem::calcDiff; used by
 * parity tests of the per-node models).  Host pointers.  Outputs per node in
 * Crocoddyl layout (running nodes t < N, terminal node t = N):
 *   Fx [B][N][nx][nx], Fu [B][N][nx][7], Lx [B][N+1][nx], Lu [B][N][7],
 *   Lxx [B][N+1][nx][nx], Lxu [B][N][nx][7], Luu [B][N][7][7],
 *   cost [B][N+1], xnext [B][N][nx], lam [B][N+1][3] (contact force, 0 if free). */
int ffddp_calc_diff(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                    const double* inst_ref, const uint8_t* surface, const double* xs,
                    const double* us, double* Fx, double* Fu, double* Lx, double* Lu, double* Lxx,
                    double* Lxu, double* Luu, double* cost, double* xnext, double* lam);
/* ffddp_calc_diff with a host force_ref [B][N+1] (ffddp_solve_batch_fref_dev's
 * array; NULL: ffddp_calc_diff).  FFDDP_E_INVALID when it is given and the
 * handle's w_fn <= 0. */
int ffddp_calc_diff_fref(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                         const double* inst_ref, const uint8_t* surface, const double* xs,
                         const double* us, const double* force_ref, double* Fx, double* Fu, double* Lx,
                         double* Lu, double* Lxx, double* Lxu, double* Luu, double* cost, double* xnext,
                         double* lam);

/* ffddp_calc_diff_fref with host cost-weight rows [B][FFDDP_COST_W]
 * (ffddp_solve_batch_wts_dev's array; NULL: ffddp_calc_diff_fref). */
int ffddp_calc_diff_wts(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                        const double* inst_ref, const uint8_t* surface, const double* xs,
                        const double* us, const double* force_ref, const double* cost_w, double* Fx,
                        double* Fu, double* Lx, double* Lu, double* Lxx, double* Lxu, double* Luu,
                        double* cost, double* xnext, double* lam);

/* ffddp_calc_diff_wts with host torque-limit rows [B][FFDDP_TAU_LIM_W]
 * (ffddp_solve_batch_lim_dev's array; NULL: ffddp_calc_diff_wts). */
int ffddp_calc_diff_lim(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                        const double* inst_ref, const uint8_t* surface, const double* xs,
                        const double* us, const double* force_ref, const double* cost_w, const double* tau_lim,
                        double* Fx, double* Fu, double* Lx, double* Lu, double* Lxx, double* Lxu, double* Luu,
                        double* cost, double* xnext, double* lam);

/* ffddp_calc_diff_lim with host link-model rows [B][FFDDP_LINK_W]
 * (ffddp_solve_batch_mdl_dev's array; NULL: ffddp_calc_diff_lim). */
int ffddp_calc_diff_mdl(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                        const double* inst_ref, const uint8_t* surface, const double* xs,
                        const double* us, const double* force_ref, const double* cost_w, const double* tau_lim,
                        const double* link_rows, double* Fx, double* Fu, double* Lx, double* Lu, double* Lxx,
                        double* Lxu, double* Luu, double* cost, double* xnext, double* lam);

/* ffddp_calc_diff_mdl with host mount rows [B][FFDDP_MOUNT_W]
 * (ffddp_solve_batch_mnt_dev's array; NULL: ffddp_calc_diff_mdl). */
int ffddp_calc_diff_mnt(ffddp_handle* h, int B, const double* x0, const double* node_ref,
                        const double* inst_ref, const uint8_t* surface, const double* xs,
                        const double* us, const double* force_ref, const double* cost_w, const double* tau_lim,
                        const double* link_rows, const double* mount_rows, double* Fx, double* Fu, double* Lx,
                        double* Lu, double* Lxx, double* Lxu, double* Luu, double* cost, double* xnext, double* lam);

/* Host-side setup helpers (CPU, same model code): frame placement of the EE
 * (pin.forwardKinematics + updateFramePlacements, crocoddyl_classical.py:199-225)
 * and gravity torque rnea(q, 0, 0) (_gravity_torque, :447-451) for B configurations. */
int ffddp_frame_placement(const ffddp_robot* robot, const double* q, double* R, double* p);
int ffddp_gravity_torque(const ffddp_robot* robot, int B, const double* q, double* tau);

/* Solver properties of crocoddyl.SolverBoxFDDP / SolverFDDP (the attributes
 * the reference leaves at their defaults: th_stop, th_grad, th_acceptstep,
 * th_acceptnegstep, th_stepdec, th_stepinc, reg_min/reg_max/reg_incfactor/
 * reg_decfactor; crocoddyl_classical.py:442-445 constructs the solver and
 * sets none of them).  neg_step_rule selects the comparator of the
 * ascent-direction acceptance (dVexp < 0, only while infeasible,
 * SolverFDDP::solve):
 *   FFDDP_NEGSTEP_CROCODDYL     accept iff dV < th_acceptnegstep * dVexp
 *                               (Crocoddyl's source; default)
 *   FFDDP_NEGSTEP_BOUNDED_RISE  accept iff dV > th_acceptnegstep * dVexp
 *                               (a rise of at most th_acceptnegstep x the
 *                               predicted one; accepts the exact LQR step)
 * Values set here apply to the following solves of the handle. */
enum { FFDDP_NEGSTEP_CROCODDYL = 0, FFDDP_NEGSTEP_BOUNDED_RISE = 1 };
typedef struct ffddp_solver_params {
  double th_stop;          /* SolverBoxFDDP 5e-5, SolverFDDP 1e-9 */
  double th_grad;          /* 1e-12 */
  double th_acceptstep;    /* 0.1 */
  double th_acceptnegstep; /* 2.0 */
  double th_stepdec;       /* 0.5 */
  double th_stepinc;       /* 0.01 */
  double reg_min, reg_max; /* 1e-9, 1e9 */
  double reg_incfactor, reg_decfactor; /* 10, 10 */
  int32_t neg_step_rule;   /* FFDDP_NEGSTEP_* */
  int32_t reserved;
} ffddp_solver_params;
int ffddp_get_solver_params(const ffddp_handle* h, ffddp_solver_params* p);
int ffddp_set_solver_params(ffddp_handle* h, const ffddp_solver_params* p);

/* Per-iteration solver trace: what crocoddyl.CallbackVerbose prints at the end
 * of every iteration (solver.setCallbacks([crocoddyl.CallbackVerbose()]),
 * crocoddyl_classical.py:352-353, 360-361; FF :588-599).  ffddp_trace_enable
 * (h, max_iters) keeps a record per instance and iteration for the next solves
 * (0 = off); ffddp_trace_read copies the last solve's records for its B
 * instances to out [B][max_iters][FFDDP_TRACE_W] (host pointer):
 *   [0] iter, [1] cost, [2] stop = sum ||Qu||^2, [3] grad = -d1 of the last
 *   tried step length, [4] preg, [5] dreg (= preg), [6] step length (the
 *   accepted one, else the smallest tried), [7] ||ffeas|| = max |fs| of the
 *   iteration's calcDiff, [8] dV, [9] dV_exp of that step length.
 * Iterations an instance did not reach (stopped earlier, failed backward
 * pass) hold NaN rows. */
#define FFDDP_TRACE_W 10
int ffddp_trace_enable(ffddp_handle* h, int max_iters);
int ffddp_trace_read(ffddp_handle* h, int B, double* out);

/* Page-locked host memory for the host-pointer entry points: arrays passed to
 * ffddp_solve_batch that live in such memory are copied by DMA on the slice
 * streams, overlapping the other slices' kernels; pageable arrays go through
 * the handle's own page-locked staging buffers. */
int ffddp_host_alloc(size_t bytes, void** p);
int ffddp_host_free(void* p);

/* Optional per-kernel device timing (HIP events recorded around every launch
 * on the launch stream), one kernel per class.  Classes, in order: init,
 * node (calc + calcDiff tangents + Gauss-Newton, one fused kernel), backward,
 * forward (line search, first pass), accept (acceptance test, regularisation,
 * stopping; no copy: the next node kernel reads the accepted trial in place),
 * commit (end of solve: accepted trials no node kernel consumed become
 * xs / us), finalize, forward2 (line search, second pass).
 * `classes` is a bit mask over those classes (bit i = class i; 0 = off,
 * FFDDP_PROFILE_ALL = every class).  Timing only the kernel of interest keeps
 * the event overhead out of the other launches.
 * ffddp_profile_read synchronises the recorded events and returns, per class,
 * the summed milliseconds and launch counts since the last reset. */
#define FFDDP_PROFILE_ALL 0xFF
int ffddp_profile_enable(ffddp_handle* h, int classes);
int ffddp_profile_read(ffddp_handle* h, double* ms, int64_t* launches, int reset);

/* Batched gravity torque on the device (tau_ref for B instances), device pointers. */
int ffddp_gravity_torque_dev(ffddp_handle* h, int B, const double* q, double* tau, void* stream);
/* The same under each instance's own model: link_rows [B][FFDDP_LINK_W] device
 * doubles (ffddp_solve_batch_mdl_dev), the kinematics and gravity the handle's.
 * Rows of the handle's robot give ffddp_gravity_torque_dev's bits; link_rows ==
 * NULL is that function. */
int ffddp_gravity_torque_mdl_dev(ffddp_handle* h, int B, const double* q, const double* link_rows, double* tau,
                                 void* stream);
/* The same under each instance's own mount as well: mount_rows
 * [B][FFDDP_MOUNT_W] device doubles (ffddp_solve_batch_mnt_dev).  Either array
 * may be NULL (the handle's robot supplies that part); both NULL is
 * ffddp_gravity_torque_dev.  Rows of the handle's robot give its bits.
 * FFDDP_E_INVALID for a null handle, B < 0, or a null q or tau with B > 0
 * (checked here, before any launch). */
int ffddp_gravity_torque_mnt_dev(ffddp_handle* h, int B, const double* q, const double* link_rows,
                                 const double* mount_rows, double* tau, void* stream);

/* Device-side problem builder: what _build_problem (crocoddyl_classical.py:
 * 521-556; FF :776-836) feeds the action models, for B instances at once,
 * as the solver's input arrays.  Instance b solves from time t0[b] and state
 * x0[b] (nx): knot k samples the task at t0 + k dt_ocp (k = 0..N) and maps
 * it to the Pinocchio frame; surface[b] = the task's contact flag at t0
 * (phase_source "trajectory"); inst_ref = posture and torque references.
 * Device pointers: t0[B], x0[B][nx] -> node_ref[B][N+1][6],
 * inst_ref[B][21], surface[B]. */
int ffddp_build_problem_dev(ffddp_handle* h, int B, const ffddp_task* task, const double* t0, const double* x0,
                            double* node_ref, double* inst_ref, uint8_t* surface, void* stream);

/* Per-tick glue of a receding-horizon fleet (B closed loops, one batched
 * solve per control tick) around ffddp_solve_batch_dev.  Device pointers,
 * asynchronous on `stream`; N and nx are the handle's.  Pure data movement
 * plus a finiteness test, so the results are exact.  Outputs must not
 * overlap inputs.  FFDDP_E_INVALID for a null handle or pointer or B <= 0,
 * FFDDP_E_CAPACITY for B > max_batch.
 *
 * ffddp_fleet_warm_start_dev: the controllers' _shift_guess
 * (crocoddyl_classical.py:733-757) from the kept solution:
 *   xs_init[b][0] = x0[b];  k >= 1: valid[b] ? keep_xs[b][k] : x0[b]
 *                           (the state index is not shifted, as in the reference)
 *   us_init[b][k] = valid[b] ? keep_us[b][min(k+1, N-1)] : u_cold[b]
 * x0 [B][nx], u_cold [B][7] (classical: the previous command; force feedback:
 * y0[14:21]), valid [B] (1 = a kept solution exists), keep_xs [B][N+1][nx],
 * keep_us [B][N][7] -> xs_init [B][N+1][nx], us_init [B][N][7].
 *
 * ffddp_fleet_keep_dev: after the solve.  Per instance fin = the seven
 * entries of us[b][0] are finite (only knot 0 is tested,
 * crocoddyl_classical.py:378-384); if fin the instance's whole xs, us, K are
 * copied to keep_xs, keep_us, keep_K, else those are left untouched.  Then
 * first[b] takes one packed record from the kept arrays,
 * FFDDP_FLEET_FIRST_W(nx) = 14 + 9 nx doubles, in this order:
 *   [0] fin (0 / 1), [1..7] keep_us[0], [8..] keep_xs[0] (nx), keep_xs[1] (nx),
 *   keep_K[0] (7 nx, row-major [7][nx]), cost, iters, ok, stats[9],
 *   fn_pred[0], fn_pred[1]
 * (integers converted to double), which is all a controller reads of a tick's
 * solve: one copy to the host per tick.  xs, us, K, cost, iters, ok, fn_pred,
 * stats are ffddp_solve_batch_dev's outputs (stats is required here). */
#define FFDDP_FLEET_FIRST_W(nx) (14 + 9 * (nx))
int ffddp_fleet_warm_start_dev(ffddp_handle* h, int B, const double* x0, const double* u_cold, const uint8_t* valid,
                               const double* keep_xs, const double* keep_us, double* xs_init, double* us_init,
                               void* stream);
int ffddp_fleet_keep_dev(ffddp_handle* h, int B, const double* xs, const double* us, const double* K,
                         const double* cost, const int32_t* iters, const uint8_t* ok, const double* fn_pred,
                         const int32_t* stats, double* keep_xs, double* keep_us, double* keep_K, double* first,
                         void* stream);

/* The fleet's closed loop on the device: everything a fleet tick does around
 * the solve besides the two kernels above, per instance exactly what
 * FleetClassicalMPC / FleetForceFeedbackMPC.compute_control do on the host
 * (ffddp/fleet.py), from controller state that stays in caller-owned device
 * arrays.  A tick is ffddp_fleet_pre_dev, ffddp_solve_batch_dev,
 * ffddp_fleet_post_dev on one stream; nothing crosses to the host.  Device
 * pointers, asynchronous on `stream`; N, nx and the variant are the handle's.
 * FFDDP_E_INVALID for a null handle, a null required pointer, a bad stride
 * or mode, or B <= 0; FFDDP_E_CAPACITY for B > max_batch. */
typedef struct ffddp_fleet_state {
  uint8_t* valid;      /* [B] 1 = a kept solution exists (warm start, policy) */
  uint8_t* latched;    /* [B] the surface latch (phase_source force_latch) */
  int32_t* loss_count; /* [B] consecutive ticks below fn_contact_off while latched */
  int8_t* prev_mode;   /* [B] last tick's surface flag, -1 before the first tick */
  double* tau_prev;    /* [B][7] the previous command */
  double* keep_xs;     /* [B][N+1][nx] the kept solution, as for ffddp_fleet_keep_dev */
  double* keep_us;     /* [B][N][7] */
  double* keep_K;      /* [B][N][7][nx] */
} ffddp_fleet_state;

/* The controller configuration's scalars (ClassicalMPCConfig /
 * ForceFeedbackMPCConfig); the ff_* fields, eps_pol and the alphas are read
 * by the force-feedback variant only. */
typedef struct ffddp_fleet_params {
  int32_t phase_source;          /* 0 "trajectory" (the contact hint), 1 "force_latch" */
  int32_t contact_release_steps;
  int32_t posture_mode;          /* 0: x_reg_ref = x0[:14]; 1: [q_nom, 0] */
  int32_t torque_mode;           /* 0: gravity(q); 1: gravity(q_nom); 2: zero */
  int32_t use_feedback_policy;
  int32_t ff_use_tau_interpolation;
  int32_t ff_inverse_actuation_model;
  int32_t ff_dt_mpc_below_dt_ocp; /* dt_mpc < dt_ocp - 1e-9 */
  double z_contact, z_contact_band, fn_contact_on, fn_contact_off;
  double feedback_gain_scale, max_solver_cost, max_tau_raw_inf, fallback_dq_damping;
  double tau_limits[7];
  double eps_pol;    /* clip(dt_mpc / dt_ocp, 0, 1) */
  double alpha_ocp;  /* the torque filter's pole at dt_ocp */
  double alpha_ctrl; /* the torque filter's pole at the control period */
} ffddp_fleet_params;

/* ffddp_fleet_pre_dev: everything before the solve.
 * Inputs: q, v (rows of 7, row stride ld_qv doubles), fn_meas, ee_z (one value
 * per instance, stride ld_scalar), tau_hat (rows of 7, stride ld_tau_hat; force
 * feedback only, else may be NULL) -- so they may be views into the plant's
 * FFDDP_PLANT_OBS records (q = obs, v = obs + 7, fn_meas = obs + 46, ee_z =
 * obs + 30, strides FFDDP_PLANT_OBS).  contact (stride ld_scalar, may be
 * NULL): when given, the force used is fn_meas * (contact > 0.5), the plant
 * record's obs[46] * (obs[47] > 0.5).  q_nom [B][7]; node_ref1 [N+1][6] this
 * tick's node references, shared by the instances; contact_hint the
 * trajectory's contact flag at this tick.
 * Per instance: the surface latch (_surface; a non-finite ee_z is not near),
 * the mode-switch drop of `valid` and prev_mode (_phase) -> state, surface[b];
 * x0[b] = [q, v] (force feedback [q, v, tau_hat]); inst_ref[b] = posture
 * reference per posture_mode, gravity torque per torque_mode (the device
 * gravity_torque, as ffddp_gravity_torque_dev); node_ref[b] = node_ref1;
 * xs_init / us_init by ffddp_fleet_warm_start_dev's rule with the updated
 * valid and u_cold = tau_prev (classical) or tau_hat (force feedback).
 *
 * ffddp_fleet_post_dev: everything after the solve.  xs .. stats are the
 * solve's outputs, x0 and surface what pre wrote, tau_bias rows of 7 with
 * stride ld_tau_bias (the plant's obs + 14).  fin and keep as
 * ffddp_fleet_keep_dev, valid |= fin; the torque policy from the kept first
 * knot (classical us0 + s K0 (x0 - xs0); force feedback Eq. 14-18 and the
 * inverse actuation map) in the fleets' order of operations, only the order
 * of summation inside the dot products differs from numpy's; then _command:
 * tau_raw_inf, unstable (fallback tau_bias - damping v, valid &= ~unstable),
 * non-finite rows -> tau_prev, clip to tau_limits, tau_prev = tau_cmd.
 * Outputs tau_cmd [B][7] and info [B][FFDDP_FLEET_INFO_W]:
 *   [0] ok, [1] cost, [2] iters, [3] fin, [4] unstable, [5] surface,
 *   [6] policy_idx (0 / -1), [7] neg_accepted (stats[9]), [8] tau_raw_inf,
 *   [9] tau_cmd_inf, [10] tau_des_inf (NaN for classical), [11] fn_pred
 *   (classical: knot 0; force feedback: the knot-0/1 interpolation; NaN when free).
 * Optional (NULL = off), the closed-loop sweep's actuation and logging:
 *   tau_app [B][7] = scale [B][7] * tau_cmd, per joint (scale NULL = 1);
 *   tau_filt [B][7] (needs tau_app) <- (1 - lpf) tau_filt + lpf tau_app, the
 *     next tick's tau_hat of the force-feedback sweep;
 *   log_obs [B][FFDDP_FLEET_LOG_W] <- obs[b][28..30, 46, 47] (site position,
 *     normal force, contact flag) of obs [B] rows with stride ld_obs. */
#define FFDDP_FLEET_INFO_W 12
#define FFDDP_FLEET_LOG_W 5
int ffddp_fleet_pre_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                        const double* q, const double* v, const double* fn_meas, const double* contact,
                        const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                        const double* q_nom, const double* node_ref1, int contact_hint, double* x0, uint8_t* surface,
                        double* inst_ref, double* node_ref, double* xs_init, double* us_init, void* stream);
int ffddp_fleet_post_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                         const double* xs, const double* us, const double* K, const double* cost,
                         const int32_t* iters, const uint8_t* ok, const double* fn_pred, const int32_t* stats,
                         const double* x0, const uint8_t* surface, const double* tau_bias, int ld_tau_bias,
                         double* tau_cmd, double* info, const double* scale, double* tau_app, double* tau_filt,
                         double lpf, const double* obs, int ld_obs, double* log_obs, void* stream);

/* The scheduled tick: the controllers' mpc_update_steps (solve every
 * period-th tick, the Riccati feedback policy on the receding plan in
 * between; crocoddyl_classical.py:430-438, _need_solve) and
 * apply_command_filter (_safe_tau's trust / rate / smoothing filter, :272-284).
 * A tick is ffddp_fleet_pre_sched_dev, ffddp_solve_batch_sel_dev with
 * active = need, ffddp_fleet_post_sched_dev on one stream.  The arguments are
 * the unscheduled entry points' plus this struct by value; those entry points
 * themselves are unchanged.
 *
 * Instances do not solve in lockstep: a mode switch, an unstable tick or a
 * non-finite solve drops an instance's plan (valid = 0) and it solves on its
 * next tick whatever the period says.  pre:  need[b] = !warm || since[b] + 1
 * >= period, with warm = valid && no mode change, after the unchanged latch
 * and mode logic.
 *
 * The kept solution is never moved.  The reference shifts its lists by one
 * knot per tick without a solve (us, xs, Ks -> [1:] + [last]), which is pure
 * copying: after age[b] shifts, knot i of the shifted lists is knot
 * min(i + age, N - 1) of keep_us / keep_K and knot min(i + age, N) of
 * keep_xs, and every reader indexes through age.
 *   pre   x0, surface, inst_ref, node_ref and the state for every instance, as
 *         ffddp_fleet_pre_dev; for need instances the warm start of the
 *         shifted lists, xs_init[k >= 1] = keep_xs[min(k + age, N)], us_init[k]
 *         = keep_us[min(k + 1 + age, N - 1)] (cold start as before); the
 *         xs_init / us_init rows of the others are not written.
 *   post  fin = need && us[b][0] finite; a keep sets age = 0.  The policy
 *         reads knot min(age, N - 1) of keep_us / keep_K, knot min(age, N) of
 *         keep_xs and (force feedback, tau1) knot min(age + 1, N).  info's
 *         cost, ok, iters, fn_pred come from the solve's output rows, which
 *         for an instance that did not solve still hold its last solve's
 *         values (the controllers' _last_solve_* and carried fn_pred);
 *         neg_accepted is 0 for it.  With apply_filter, after the non-finite
 *         row substitution and the clip to tau_limits:
 *             d   = clip(target - prev, +-tau_trust_inf)
 *             d   = clip(d, +-tau_rate_limit[i] * dt)
 *             cmd = clip((1 - a) prev + a (prev + d), +-tau_limits[i])
 *         without contraction, a NaN propagating as in numpy.clip; tau_prev =
 *         cmd.  Last: since = solved ? 0 : since + 1, age += 1 unless solved.
 * With period = 1, apply_filter = 0 and age = 0 both give the unscheduled
 * entry points' bits.  FFDDP_E_INVALID also for a null since / age / need,
 * period < 1, or (apply_filter) tau_smoothing_alpha outside [0, 1]. */
typedef struct ffddp_fleet_sched {
  int32_t period;             /* mpc_update_steps, >= 1 */
  int32_t apply_filter;       /* apply_command_filter */
  double tau_trust_inf;
  double tau_smoothing_alpha; /* already clipped to [0, 1] */
  double dt;                  /* the control period */
  double tau_rate_limit[7];
  int32_t* since;             /* [B] state: ticks since the instance's last solve */
  int32_t* age;               /* [B] state: shifts of the kept solution since it was kept */
  uint8_t* need;              /* [B] written by pre: 1 = the instance solves this tick */
} ffddp_fleet_sched;
int ffddp_fleet_pre_sched_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                              const double* q, const double* v, const double* fn_meas, const double* contact,
                              const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                              const double* q_nom, const double* node_ref1, int contact_hint, double* x0,
                              uint8_t* surface, double* inst_ref, double* node_ref, double* xs_init, double* us_init,
                              ffddp_fleet_sched sched, void* stream);
int ffddp_fleet_post_sched_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                               const double* xs, const double* us, const double* K, const double* cost,
                               const int32_t* iters, const uint8_t* ok, const double* fn_pred, const int32_t* stats,
                               const double* x0, const uint8_t* surface, const double* tau_bias, int ld_tau_bias,
                               double* tau_cmd, double* info, const double* scale, double* tau_app, double* tau_filt,
                               double lpf, const double* obs, int ld_obs, double* log_obs, ffddp_fleet_sched sched,
                               void* stream);
/* The post stage with each instance's own torque limit: tau_lim is the solve's
 * [B][FFDDP_TAU_LIM_W] rows (ffddp_solve_batch_lim_dev), of which entry 4i of
 * row b replaces p->tau_limits[i] in _command's clip and in the filter's final
 * clip, so a derated instance is never commanded beyond what its solver
 * planned for.  sched as in ffddp_fleet_pre_task_dev: NULL is the unscheduled
 * tick.  tau_lim == NULL gives ffddp_fleet_post_dev's / _post_sched_dev's bits.
 * Errors are theirs, under this function's name. */
int ffddp_fleet_post_lim_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                             const double* xs, const double* us, const double* K, const double* cost,
                             const int32_t* iters, const uint8_t* ok, const double* fn_pred, const int32_t* stats,
                             const double* x0, const uint8_t* surface, const double* tau_bias, int ld_tau_bias,
                             double* tau_cmd, double* info, const double* scale, double* tau_app, double* tau_filt,
                             double lpf, const double* obs, int ld_obs, double* log_obs,
                             const ffddp_fleet_sched* sched, const double* tau_lim, void* stream);

/* The closed-loop sweep's actuation-uncertainty injector on the device
 * (ffddp/uncertainty.py BatchedUncertaintyInjector, bit for bit): two more
 * launches per tick around the three above.  Tick k of an injected fleet is
 *   plant step, ffddp_fleet_inject_obs_dev, ffddp_fleet_pre_dev, the solve,
 *   ffddp_fleet_post_dev, ffddp_fleet_inject_cmd_dev
 * on one stream.  The scalars travel by value; the arrays are caller-owned
 * device memory.  row[b] >= 0 is instance b's row in a, b, seed and the noise
 * table; row[b] = -1 marks an instance without an injector (both kinds share
 * one fleet).  The rings, the filter and z_cmd are indexed by the instance.
 * The ring slots are functions of the tick number k alone (no device-side
 * counter): the observation ring is written at (k - 1) mod (d_obs + 1) and
 * read at k mod (d_obs + 1), at k = 0 every slot takes the first observation;
 * the command ring (zero before the first tick) is written at k mod
 * (d_cmd + 1) and read at (k + 1) mod (d_cmd + 1).  The arithmetic is
 * compiled without contraction in the host class's order and grouping, so the
 * results are numpy's bits. */
#define FFDDP_INJECT_NOISE_TABLE 0  /* the caller passes tick k's normals (uncertainty.predraw) */
#define FFDDP_INJECT_NOISE_PHILOX 1 /* Philox4x64-10 and Box-Muller on the device, from seed */
#define FFDDP_INJECT_NZ 28          /* normals per instance and tick: q, dq, tau (observation), tau (command) */
typedef struct ffddp_fleet_inject {
  int32_t d_obs;         /* observation delay in ticks (>= 0) */
  int32_t d_cmd;         /* command delay in ticks (>= 0) */
  int32_t noise;         /* FFDDP_INJECT_NOISE_* */
  int32_t rows;          /* length of a / b / seed and of a tick's noise table; row[b] >= rows counts as -1 */
  double sigma_q, sigma_dq, sigma_tau;
  double lpf;            /* the torque measurement filter's alpha */
  const int32_t* row;    /* [B] row in a / b / seed / z, or -1: no injector */
  const double* a;       /* [rows] actuation gain */
  const double* b;       /* [rows] actuation bias */
  const uint64_t* seed;  /* [rows] Philox key word 0 (FFDDP_INJECT_NOISE_PHILOX only, else may be NULL) */
  double* obs_ring;      /* [d_obs+1][B][14] delayed (q, dq) */
  double* cmd_ring;      /* [d_cmd+1][B][7] delayed commands */
  double* tau_hat_filt;  /* [B][7] the filtered torque measurement (state) */
  double* z_cmd;         /* [B][7] the command normals the obs kernel leaves for the cmd kernel */
} ffddp_fleet_inject;

/* ffddp_fleet_inject_obs_dev: BatchedUncertaintyInjector.observation_for_controller.
 * q, v: rows of 7 with stride ld_qv (views of the plant's records).  z: tick
 * k's normals [rows][FFDDP_INJECT_NZ] (table mode; ignored for Philox, may be
 * NULL).  Per injected instance: push (q, v) into the ring, read the oldest
 * slot, qv_ctrl[b] = old + (0.0 + sigma * z) (q then dq, [B][14]); tau_hat[b]
 * = a cmd_ring[oldest] + b + (0.0 + sigma_tau z[14..20]); tau_hat_filt <-
 * (1 - lpf) tau_hat_filt + lpf tau_hat; z_cmd[b] = z[21..27].  tau_hat
 * ([B][7], the raw measurement) and tau_ctrl ([B][7], the controllers'
 * measured torque: tau_hat_filt) are optional outputs.  row[b] = -1:
 * qv_ctrl[b] is the plant's (q, v) unchanged and, when tau_filt ([B][7], the
 * filter ffddp_fleet_post_dev maintains; may be NULL) is given, tau_hat[b] =
 * tau_ctrl[b] = tau_filt[b].
 *
 * ffddp_fleet_inject_cmd_dev: command_for_plant.  Per injected instance:
 * cmd_ring[k mod (d_cmd+1)][b] = tau_cmd[b], then tau_app[b] = a
 * cmd_ring[(k+1) mod (d_cmd+1)][b] + b + (0.0 + sigma_tau z_cmd[b]); with
 * row[b] = -1 tau_app[b] (ffddp_fleet_post_dev's scale * tau_cmd) is left.
 *
 * ffddp_fleet_noise_dev: the Philox source alone.  z [B][FFDDP_INJECT_NZ] for
 * tick k from seed [B]; words ([B][7][4], may be NULL) the raw blocks.  Lane
 * j of instance b evaluates philox4x64_10(counter = [k + 1, j, 0, 0], key =
 * [seed_b, TAG]) with TAG = 0x4646444450494e4a ("FFDDPINJ"; INJECT_PHILOX_TAG
 * of csrc/ffddp_consts.hpp) -- the first four words of numpy.random.
 * Philox(key = ..., counter = [k, j, 0, 0]).random_raw(4), which increments
 * the counter before it generates.  Box-Muller on pairs: u1 = ((w0 >> 11) + 1)
 * 2^-53, u2 = (w1 >> 11) 2^-53, z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2
 * ln u1) sin(2 pi u2); (w0, w1) -> joint j's q and dq normals, (w2, w3) -> its
 * two torque normals (observation, command).
 *
 * All three: device pointers, asynchronous on `stream`.  FFDDP_E_INVALID for
 * a null handle, a null required pointer, a delay below 0, an unknown noise
 * mode, a bad stride, k < 0 or B <= 0; FFDDP_E_CAPACITY for B > max_batch. */
int ffddp_fleet_inject_obs_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const double* z,
                               const double* q, const double* v, int ld_qv, const double* tau_filt, double* qv_ctrl,
                               double* tau_hat, double* tau_ctrl, void* stream);
int ffddp_fleet_inject_cmd_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const double* tau_cmd,
                               double* tau_app, void* stream);
int ffddp_fleet_noise_dev(ffddp_handle* h, int B, const uint64_t* seed, int k, double* z, uint64_t* words,
                          void* stream);

/* Per-instance uncertainty profiles: the two injector calls with each injected
 * instance's own delays and noise levels.  ffddp_fleet_inject keeps its layout
 * and its meaning: inj->d_obs / inj->d_cmd are the ring depths (the rings are
 * [d_obs+1][B][14] and [d_cmd+1][B][7] as before), inj->sigma_* the levels of
 * a row whose array below is NULL.  The arrays are device memory indexed like
 * a / b / seed, by row[b].
 *
 * Slot rule per injected instance with row r, no = d_obs[r] + 1: the
 * observation ring is written at (k - 1) mod no and read at k mod no; at k = 0
 * slots 0 .. d_obs[r] take the first observation.  The command ring, nc =
 * d_cmd[r] + 1: written at k mod nc, read at (k + 1) mod nc.  An instance
 * never touches a slot above its own delay; its slot sequence is that of a
 * ring of its own depth.  The kernels clamp a delay into [0, depth], so no
 * value indexes outside a ring (the caller validates; a clamped delay is not
 * the profile that was asked for).  The arithmetic per element is that of
 * ffddp_fleet_inject_obs_dev / _cmd_dev with the row's sigma in place of the
 * scalar: no contraction, numpy's bits.
 *
 * rows == NULL, or all three members NULL: exactly ffddp_fleet_inject_obs_dev
 * / ffddp_fleet_inject_cmd_dev (the same kernels are launched).  Error codes
 * as for those calls. */
typedef struct ffddp_fleet_inject_rows {   /* per row of a / b / seed; a NULL member = the scalar of ffddp_fleet_inject */
  const int32_t* d_obs;   /* [rows] observation delay in ticks, 0 .. inj->d_obs (the ring depth) */
  const int32_t* d_cmd;   /* [rows] command delay in ticks, 0 .. inj->d_cmd */
  const double* sigma;    /* [rows][3] sigma_q, sigma_dq, sigma_tau */
} ffddp_fleet_inject_rows;
int ffddp_fleet_inject_obs_rows_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k, const double* z,
                                    const double* q, const double* v, int ld_qv, const double* tau_filt,
                                    double* qv_ctrl, double* tau_hat, double* tau_ctrl,
                                    const ffddp_fleet_inject_rows* rows, void* stream);
int ffddp_fleet_inject_cmd_rows_dev(ffddp_handle* h, int B, const ffddp_fleet_inject* inj, int k,
                                    const double* tau_cmd, double* tau_app, const ffddp_fleet_inject_rows* rows,
                                    void* stream);

/* Per-instance tasks and start delays: every instance carries a record of its
 * own approach-then-circle task (ffddp/trajectory.py FleetTask, task_records)
 * and the pre kernel samples that instance's N+1 node references and its
 * contact hint itself, where ffddp_fleet_pre_dev takes one row shared by the
 * instances.  A record is FFDDP_FLEET_TASK_W doubles, the closure constants of
 * make_approach_then_circle and with_contact_hold as the host computed them:
 *   [0..2] center, [3] radius, [4] omega, [5] z_contact, [6] t_pre (>= 0),
 *   [7] t_approach (>= 1e-6), [8..10] p_start, [11..13] p_pre,
 *   [14..16] p_contact_start, [17..19] p_hold (the base trajectory's position
 *   at t_contact_phase), [20] t_hold_end (t_contact_phase + t_hold),
 *   [21] delay in seconds (>= 0).
 * The sampler evaluates a record at a task time: knot k at t + k dt_ocp (one
 * multiply, one add; dt_ocp is the handle's), in the MuJoCo world, mapped to
 * the Pinocchio frame as ffddp_build_problem_dev does (diag(-1, -1, 1), minus
 * p_site_minus_frame).  It is compiled without contraction in trajectory.py's
 * order and grouping: outside the circle phase (pre, approach, hold, negative
 * task time, where the smoothstep clamps at the start pose) the entries are
 * numpy's bits; in the circle phase the device sincos stands in for numpy's.
 *
 * ffddp_fleet_task_refs_dev: the sampler alone.  t [B] the instances' task
 * times (the delay already subtracted; tasks.t is not read) -> node_ref
 * [B][N+1][6] and hint [B], the surface flag at t[b].
 *
 * ffddp_fleet_pre_task_dev: ffddp_fleet_pre_dev (sched NULL) or
 * ffddp_fleet_pre_sched_dev (sched given) with node_ref1 / contact_hint
 * replaced per instance: instance b's task time is tasks.t - rec[b].delay (one
 * subtraction), its hint the record's surface flag at that time, node_ref[b]
 * the sampler's knots; everything else is the same code, so an instance given
 * the same references and hint gets the same bits from both.
 *
 * Both: device pointers, asynchronous on `stream`.  FFDDP_E_INVALID for a
 * null handle, a null record pointer or any other null required pointer, a
 * scheduled call with a null since / age / need, B <= 0 and what
 * ffddp_fleet_pre_dev refuses; FFDDP_E_CAPACITY for B > max_batch. */
#define FFDDP_FLEET_TASK_W 22
#define FFDDP_FLEET_TASK_CENTER 0
#define FFDDP_FLEET_TASK_RADIUS 3
#define FFDDP_FLEET_TASK_OMEGA 4
#define FFDDP_FLEET_TASK_Z_CONTACT 5
#define FFDDP_FLEET_TASK_T_PRE 6
#define FFDDP_FLEET_TASK_T_APPROACH 7
#define FFDDP_FLEET_TASK_P_START 8
#define FFDDP_FLEET_TASK_P_PRE 11
#define FFDDP_FLEET_TASK_P_CS 14
#define FFDDP_FLEET_TASK_P_HOLD 17
#define FFDDP_FLEET_TASK_T_HOLD_END 20
#define FFDDP_FLEET_TASK_DELAY 21
typedef struct ffddp_fleet_tasks {
  double p_site_minus_frame[3]; /* the site calibration offset, Pinocchio frame */
  double t;                     /* the tick's time (ffddp_fleet_pre_task_dev) */
  const double* rec;            /* [B][FFDDP_FLEET_TASK_W] the records */
} ffddp_fleet_tasks;
int ffddp_fleet_task_refs_dev(ffddp_handle* h, int B, ffddp_fleet_tasks tasks, const double* t, double* node_ref,
                              uint8_t* hint, void* stream);
int ffddp_fleet_pre_task_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                             const double* q, const double* v, const double* fn_meas, const double* contact,
                             const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                             const double* q_nom, ffddp_fleet_tasks tasks, double* x0, uint8_t* surface,
                             double* inst_ref, double* node_ref, double* xs_init, double* us_init,
                             const ffddp_fleet_sched* sched, void* stream);
/* The pre stage with each instance's own rigid-body model: link_rows is the
 * solve's [B][FFDDP_LINK_W] rows (ffddp_solve_batch_mdl_dev), with which the
 * gravity torque reference inst_ref[14..20] of torque modes 0 and 1 is
 * computed (ffddp_gravity_torque_mdl_dev's bits); every other output is
 * ffddp_fleet_pre_task_dev's.  tasks.rec == NULL: the shared references
 * node_ref1 / contact_hint of ffddp_fleet_pre_dev are used instead of the
 * per-instance tasks.  sched as in ffddp_fleet_pre_task_dev.  link_rows ==
 * NULL gives ffddp_fleet_pre_task_dev's (with tasks.rec == NULL
 * ffddp_fleet_pre_dev's / _pre_sched_dev's) bits.  Errors are theirs, under
 * this function's name. */
int ffddp_fleet_pre_mdl_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                            const double* q, const double* v, const double* fn_meas, const double* contact,
                            const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                            const double* q_nom, ffddp_fleet_tasks tasks, const double* node_ref1, int contact_hint,
                            double* x0, uint8_t* surface, double* inst_ref, double* node_ref, double* xs_init,
                            double* us_init, const ffddp_fleet_sched* sched, const double* link_rows, void* stream);
/* ffddp_fleet_pre_mdl_dev with each instance's own mount: mount_rows is the
 * solve's [B][FFDDP_MOUNT_W] rows (ffddp_solve_batch_mnt_dev), under which (and
 * under link_rows, if given) the gravity torque reference inst_ref[14..20] of
 * torque modes 0 and 1 is computed (ffddp_gravity_torque_mnt_dev's bits).
 * Every other output is unchanged; the measurements handed in are expected in
 * the instance's planning frame (ffddp_fleet_obs_frame_dev).  mount_rows ==
 * NULL gives ffddp_fleet_pre_mdl_dev's bits.  Errors are its, under this
 * function's name. */
int ffddp_fleet_pre_mnt_dev(ffddp_handle* h, int B, const ffddp_fleet_params* p, const ffddp_fleet_state* s,
                            const double* q, const double* v, const double* fn_meas, const double* contact,
                            const double* ee_z, int ld_qv, int ld_scalar, const double* tau_hat, int ld_tau_hat,
                            const double* q_nom, ffddp_fleet_tasks tasks, const double* node_ref1, int contact_hint,
                            double* x0, uint8_t* surface, double* inst_ref, double* node_ref, double* xs_init,
                            double* us_init, const ffddp_fleet_sched* sched, const double* link_rows,
                            const double* mount_rows, void* stream);

/* A plant record per instance (ffddp_plant_step_dev's [B][ld_obs] observation,
 * FFDDP_PLANT_OBS = 69 words, MuJoCo world) re-expressed in each instance's
 * planning frame.  frame is [B][FFDDP_FRAME_W] device doubles, the frame's
 * pose in the MuJoCo world: R (9, row-major) and p (3), x_world = R x_frame +
 * p.  The 69 words are copied to obs_out [B][ld_out], with these replaced:
 *     EE position (28..30)           R^T (x - p)
 *     EE velocity (31..33)           R^T x
 *     EE rotation (34..42)           R^T X
 *     world contact force (43..45)   R^T x
 *     site Jacobian (48..68, 3 x 7)  R^T J
 * q, dq, bias, constraint torque, the normal force and the contact count are
 * joint-space or scalar and stay.  Each replaced entry i is
 * (R[0][i] x0 + R[1][i] x1) + R[2][i] x2 in that order, without contraction
 * (x - p is formed first), so the same expression in IEEE doubles elsewhere
 * gives the same bits.  sel is [B] bytes or NULL (all): an instance with
 * sel[b] == 0 is copied verbatim and its frame row is not read.  obs_out must
 * not overlap obs.  FFDDP_E_INVALID for a null handle, obs, frame or obs_out,
 * B <= 0, ld_obs < 69 or ld_out < 69; FFDDP_E_CAPACITY for B > max_batch. */
#define FFDDP_FRAME_W 12
int ffddp_fleet_obs_frame_dev(ffddp_handle* h, int B, const double* obs, int ld_obs, const double* frame,
                              const uint8_t* sel, double* obs_out, int ld_out, void* stream);

/* The sweep's task metrics accumulated on the device: one call folds one plant
 * record per instance -- the observation after a tick's command -- into
 * per-instance running sums, maxima and counts, everything the sweep's summary
 * (ffddp/runlog.py summary_metrics, the solver-health counters of
 * ffddp/fleet.py) is made of, so a run of any length returns
 * FFDDP_FLEET_METRICS_W doubles per instance instead of its per-tick logs.
 *
 * acc [FFDDP_FLEET_METRICS_W][ld] is field-major with ld >= B (instance b's
 * field f at acc[f * ld + b]; columns b >= B are not touched).  The caller
 * zeroes it before the first call, MAX_FN to -inf.  obs: rows with stride
 * ld_obs (>= 48) laid out as the plant's records; [28..30] the site position,
 * [46] the normal force, [47] the contact flag are read.  Per call and instance
 *   fn = obs[46] * (obs[47] > 0.5), contact = fn > 0.5,
 *   e = obs[28..30] - p_ref, err_tan = sqrt(ex^2 + ey^2),
 *   err_3d = sqrt((ex^2 + ey^2) + ez^2), in_phase = ts >= t_phase[b]
 * and the fields take
 *   N += 1, SUM_TAN2 += err_tan^2, SUM_3D2 += err_3d^2 (the squares of the
 *   rounded norms), SUM_ABS_TAN += |err_tan|, SUM_ABS_FN_ERR += |fn - fn_des|,
 *   MAX_FN = max(MAX_FN, fn), SUM_CONTACT += contact,
 *   MAX_ERR_3D = max(MAX_ERR_3D, err_3d); when in_phase: N_PHASE += 1,
 *   SUM_TAN2_PHASE += err_tan^2, SUM_CONTACT_PHASE += contact,
 *   SUM_FN_PHASE += fn;
 *   with info (the tick's [B][FFDDP_FLEET_INFO_W] row of ffddp_fleet_post_dev;
 *   NULL: these four are not touched): UNSTABLE_TICKS += info[4] != 0,
 *   NEG_ACCEPTED_TICKS += info[7] > 0, NOT_OK_TICKS += info[0] == 0,
 *   SOLVED_TICKS += need[b] != 0 (need [B], the scheduled tick's mask; NULL:
 *   every instance solved);
 *   with plant_fail (ffddp_plant_step_dev's [B] flags of the step that wrote
 *   obs; may be NULL): PLANT_FAIL += plant_fail[b].
 * The reference position p_ref (MuJoCo world) and the series time ts come from
 * one of two sources.  tasks.rec non-NULL: instance b's own record, ts =
 * (tasks.t - rec[b].delay) + dt in that order, p_ref the sampler's knot 0 at
 * ts (the code ffddp_fleet_pre_task_dev inlines, the frame map undone, which
 * is exact); `rows` is the number of records, an instance b >= rows has no
 * reference (NaN: its error fields turn NaN, its force fields go on) and no
 * record is read beyond them; p_ref and ts are ignored.  tasks.rec NULL: the
 * shared device row p_ref [3] and the scalar ts (rows, dt, tasks.t ignored).
 * t_phase [B]: the start of each instance's contact phase in its series time.
 * The terms are compiled without contraction in the host summary's order and
 * grouping (IEEE add, multiply, square root: numpy's bits, given the same
 * reference); NaN propagates into the sums and, as in numpy.max, into both
 * maxima.  Every sum is sequential in call order: reproducible run to run.
 * One lane per instance, no shared memory, no atomics.
 *
 * Device pointers, asynchronous on `stream`.  FFDDP_E_INVALID for a null
 * handle, a null obs / t_phase / acc, neither a record pointer nor p_ref,
 * ld < B, ld_obs < 48, rows < 0 or B <= 0; FFDDP_E_CAPACITY for B > max_batch. */
#define FFDDP_FLEET_METRICS_W 17
#define FFDDP_FLEET_METRICS_N 0
#define FFDDP_FLEET_METRICS_N_PHASE 1
#define FFDDP_FLEET_METRICS_SUM_TAN2 2
#define FFDDP_FLEET_METRICS_SUM_TAN2_PHASE 3
#define FFDDP_FLEET_METRICS_SUM_3D2 4
#define FFDDP_FLEET_METRICS_SUM_ABS_TAN 5
#define FFDDP_FLEET_METRICS_SUM_ABS_FN_ERR 6
#define FFDDP_FLEET_METRICS_MAX_FN 7
#define FFDDP_FLEET_METRICS_SUM_CONTACT 8
#define FFDDP_FLEET_METRICS_SUM_CONTACT_PHASE 9
#define FFDDP_FLEET_METRICS_SUM_FN_PHASE 10
#define FFDDP_FLEET_METRICS_UNSTABLE_TICKS 11
#define FFDDP_FLEET_METRICS_NEG_ACCEPTED_TICKS 12
#define FFDDP_FLEET_METRICS_NOT_OK_TICKS 13
#define FFDDP_FLEET_METRICS_SOLVED_TICKS 14
#define FFDDP_FLEET_METRICS_MAX_ERR_3D 15
#define FFDDP_FLEET_METRICS_PLANT_FAIL 16
int ffddp_fleet_metrics_dev(ffddp_handle* h, int B, int ld, const double* obs, int ld_obs, ffddp_fleet_tasks tasks,
                            int rows, double dt, const double* p_ref, double ts, const double* t_phase, double fn_des,
                            const double* info, const uint8_t* need, const int32_t* plant_fail, double* acc,
                            void* stream);

/* Per-instance force setpoint profiles (ffddp/trajectory.py ForceProfile,
 * force_records).  A record is FFDDP_FLEET_FORCE_W doubles: f0, f1, t_on,
 * t_ramp (>= 0).  At task time tau the desired normal force is
 *   f0 + (f1 - f0) s,  s = min(max((tau - t_on) / t_ramp, 0), 1) for t_ramp > 0,
 *                      s = (tau >= t_on) for t_ramp == 0
 * (add, subtract, multiply, divide, min, max, compiled without contraction:
 * numpy's bits, trajectory.sample_force).
 *
 * ffddp_fleet_force_refs_dev: the sampler, one launch per tick before the
 * solve.  force_ref [B][N+1] (ffddp_solve_batch_fref_dev's argument): knot k of
 * instance b at (tasks.t - rec[b].delay) + k dt_ocp, the task sampler's knot
 * times (only tasks.t and the task records' delay are read; tasks.rec == NULL
 * means no delay); force [rows][FFDDP_FLEET_FORCE_W] the device records, an
 * instance b >= rows takes fn_default at every knot and no record is read
 * beyond min(rows, B).  One lane per (instance, knot), no shared memory.
 * FFDDP_E_INVALID for a null handle, force or force_ref, rows < 0 or B <= 0;
 * FFDDP_E_CAPACITY for B > max_batch.
 *
 * ffddp_fleet_metrics_fref_dev: ffddp_fleet_metrics_dev with SUM_ABS_FN_ERR +=
 * |fn - f(ts)|, f instance b's own force record at the series time ts the
 * call forms (above); an instance b >= rows_force uses the scalar fn_des.
 * force == NULL is ffddp_fleet_metrics_dev: same kernel, same bits (rows_force
 * ignored).  Errors as there, and FFDDP_E_INVALID for rows_force < 0 with
 * records. */
#define FFDDP_FLEET_FORCE_W 4
#define FFDDP_FLEET_FORCE_F0 0
#define FFDDP_FLEET_FORCE_F1 1
#define FFDDP_FLEET_FORCE_T_ON 2
#define FFDDP_FLEET_FORCE_T_RAMP 3
int ffddp_fleet_force_refs_dev(ffddp_handle* h, int B, ffddp_fleet_tasks tasks, const double* force, int rows,
                               double fn_default, double* force_ref, void* stream);
int ffddp_fleet_metrics_fref_dev(ffddp_handle* h, int B, int ld, const double* obs, int ld_obs,
                                 ffddp_fleet_tasks tasks, int rows, double dt, const double* p_ref, double ts,
                                 const double* t_phase, double fn_des, const double* info, const uint8_t* need,
                                 const int32_t* plant_fail, double* acc, const double* force, int rows_force,
                                 void* stream);

/* ---------------------------------------------------------------------------
 * Closed-loop plant stand-in: the MuJoCo plant of the
 * reference's closed loop, FrankaMujocoSim.step() in torque mode
 * (src/sim/franka_sim.py:144-169) on assets/scenes/panda_table_scene.xml:
 * arm (+ joint armature / damping, panda_robot.xml:9), tool sphere at the
 * ee_site (:189-199) against the table_contact plane (condim 1, soft
 * constraint solref/solimp), implicitfast integration, n_substeps physics
 * steps per control step.  Observation record: FFDDP_PLANT_OBS words per
 * instance (q, dq, qfrc_bias, qfrc_constraint, site pos/vel/rot, contact force,
 * site Jacobian), see ffddp_plant.hpp.  Parity with MuJoCo is unpinned.
 * ------------------------------------------------------------------------- */
#define FFDDP_PLANT_OBS 69
typedef struct ffddp_plant_params {
  double timestep;      /* model.opt.timestep (benchmark protocol: 0.001) */
  int32_t n_substeps;   /* physics steps per control step (5) */
  double armature[7], damping[7];
  double r_tool;        /* ee_collision sphere radius (0.03) */
  double margin;        /* contact margin (0.001) */
  double solref[2];     /* (timeconst, dampratio), MuJoCo default (0.02, 1) */
  double solimp[5];     /* MuJoCo default (0.9, 0.95, 0.001, 0.5, 2) */
  double site_R[2];     /* cos, sin of the tool-body yaw (135 deg) */
} ffddp_plant_params;

typedef struct ffddp_plant ffddp_plant;
int ffddp_plant_create(const ffddp_robot* robot, const ffddp_plant_params* p, int device, int max_batch,
                       ffddp_plant** out);
void ffddp_plant_destroy(ffddp_plant* h);
/* One control step of B plants (integrate = 0: forward only, like mj_forward).
 * Host pointers: q, v [B][7] (in/out), tau [B][7] applied torque, plane [B][6]
 * = table normal (3) and a point on the plane (3), MuJoCo world; obs
 * [B][FFDDP_PLANT_OBS].  Returns FFDDP_E_INVALID on a non-SPD mass matrix. */
int ffddp_plant_step(ffddp_plant* h, int B, double* q, double* v, const double* tau, const double* plane,
                     int integrate, double* obs);
/* Same on device pointers, asynchronous on `stream` (per-instance failure flags in fail[B], may be NULL). */
int ffddp_plant_step_dev(ffddp_plant* h, int B, double* q, double* v, const double* tau, const double* plane,
                         int integrate, double* obs, int32_t* fail, void* stream);

/* Per-instance physics: one row per instance of what ffddp_plant_params holds
 * apart from timestep, n_substeps and site_R, which stay the handle's.  rows:
 * host memory, [n][FFDDP_PLANT_ROW_W], row-major; the handle keeps its own
 * device copy (field-major, so a wave's loads of one field are consecutive
 * doubles).  From the next ffddp_plant_step / ffddp_plant_step_dev on, with
 * B <= n, instance b integrates with row b; B > n is FFDDP_E_INVALID.  rows
 * == NULL (n is ignored): back to the handle's struct for all.  The call
 * waits for the device's work before it replaces the copy.
 * FFDDP_E_INVALID with nothing changed for a null handle, n < 1 or n >
 * max_batch, or any row with a non-finite entry, armature < 0 or damping < 0,
 * r_tool <= 0, solref[0] <= 0 or solref[1] <= 0, solimp d0 or dmax outside
 * (0, 1) or dmax < d0, mid outside (0, 1), power < 1. */
#define FFDDP_PLANT_ROW_W 23
#define FFDDP_PLANT_ROW_ARMATURE 0 /* [7] */
#define FFDDP_PLANT_ROW_DAMPING 7  /* [7] */
#define FFDDP_PLANT_ROW_R_TOOL 14
#define FFDDP_PLANT_ROW_MARGIN 15
#define FFDDP_PLANT_ROW_SOLREF 16  /* [2] timeconst, dampratio */
#define FFDDP_PLANT_ROW_SOLIMP 18  /* [5] d0, dmax, width, mid, power */
int ffddp_plant_set_instance_params(ffddp_plant* h, int n, const double* rows);

/* Per-instance link inertial parameters: one link-model row per instance, the
 * row format of ffddp_solve_batch_mdl_dev (FFDDP_LINK_W: entry 16j mass[j],
 * 16j + 1..3 com[j], 16j + 4..12 inertia[j]), as ffddp_link_model_rows writes
 * them, so one set of rows can serve the controller and the plant.
 * link_rows: host memory, [n][FFDDP_LINK_W]; the handle keeps its own device
 * copy (field-major over the 91 used entries).  From the next
 * ffddp_plant_step / ffddp_plant_step_dev on, with B <= n, instance b
 * integrates with the masses, centres of mass and inertias of row b; B > n is
 * FFDDP_E_INVALID.  Kinematics, gravity, timestep, n_substeps and site_R stay
 * the handle's.  link_rows == NULL (n is ignored): back to the handle's
 * ffddp_robot for all.  The call waits for the device's work before it
 * replaces the copy.  Link rows and physics rows
 * (ffddp_plant_set_instance_params) are set and cleared independently.
 * FFDDP_E_INVALID with nothing changed for a null handle, n < 1 or n >
 * max_batch, or any row ffddp_link_model_rows would refuse: a mass that is
 * not finite and > 0, a com or inertia entry that is not finite.  The padding
 * entries (16j + 13..15, 112..127) are neither read nor checked. */
int ffddp_plant_set_instance_links(ffddp_plant* h, int n, const double* link_rows);

#ifdef __cplusplus
}
#endif
#endif /* FFDDP_H_ */
