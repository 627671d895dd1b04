"""Crocoddyl-like solver surface over the batched HIP (Box)FDDP.

Mirrors what the reference uses of crocoddyl.SolverBoxFDDP
(crocoddyl_classical.py:350-388, 442-445; crocoddyl_force_feedback.py:588-628):

    solver = BatchedBoxFDDP(cfg, max_batch)            # SolverBoxFDDP(problem)
    ok = solver.solve(batch, maxiter=10, is_feasible=False)   # solver.solve(...)
    solver.xs, solver.us, solver.K, solver.cost, solver.iter  # read-backs

with a leading batch axis.  Numerical failure never raises (ok[b] = False,
like Crocoddyl); API / device errors raise RuntimeError.

Solver properties (th_stop, th_acceptnegstep, reg_min, ...) are attributes as
on crocoddyl.SolverBoxFDDP; setCallbacks([CallbackVerbose()]) prints the
per-iteration record of instance 0 after each solve (ffddp.callbacks).
"""
from __future__ import annotations

import collections
import ctypes as C
import threading
import weakref

import numpy as np

from . import _abi
from .config import OcpConfig


class FfddpError(RuntimeError):
    pass


_PARAMS = ("th_stop", "th_grad", "th_acceptstep", "th_acceptnegstep", "th_stepdec", "th_stepinc", "reg_min",
           "reg_max", "reg_incfactor", "reg_decfactor", "neg_step_rule")


def _opt_dev_ptr(a, dtype: str, shape, what: str) -> C.c_void_p:
    """The device pointer of an optional solve_dev argument, null for None;
    ValueError(what) unless it is a contiguous device tensor of that torch
    dtype and shape."""
    if a is None:
        return C.c_void_p(0)
    import torch

    if (not isinstance(a, torch.Tensor) or a.dtype != getattr(torch, dtype) or not a.is_cuda
            or not a.is_contiguous() or tuple(a.shape) != shape):
        raise ValueError(what)
    return C.c_void_p(int(a.data_ptr()))


class _RecycledPinned:
    """Page-locked host blocks (ffddp_host_alloc) for solve()'s output arrays,
    recycled instead of freed: every solve() returns fresh arrays (no other
    live array shares their memory), and when the last array viewing a block
    is gone (weakref finalizer) the block goes back to the free list rather
    than to the allocator.  In steady state a solve then neither faults in
    nor unmaps ~118 MB of output pages (B = 4096), and ffddp_solve_batch
    copies into them by DMA as each slice finishes (no staging copy).  At
    most `cap` bytes are page-locked; past that solve() falls back to plain
    numpy arrays.

    The finalizer can run wherever the interpreter allocates (a cyclic GC
    pass), also inside arrays() or close() on the thread that holds the lock,
    so it takes no lock: it only appends the block to `returned` (atomic),
    and arrays() and close() fold `returned` into the free list under the
    lock.  After close() nobody folds any more and the finalizer frees the
    block itself; a block that races close() into `returned` is freed by
    whichever of the two pops it."""

    def __init__(self, cap: int):
        self.cap = int(cap)
        self.total = 0  # bytes page-locked while open (under the lock)
        self.free = {}  # nbytes -> [addresses] (under the lock)
        self.returned = collections.deque()  # (nbytes, address) from finalizers, not yet in `free`
        self.closed = False
        self.lock = threading.Lock()

    def _fold(self):
        while True:
            try:
                tot, p = self.returned.popleft()
            except IndexError:
                return
            self.free.setdefault(tot, []).append(p)

    def arrays(self, specs):
        offs, tot = {}, 0
        for k, (shape, dt) in specs.items():
            offs[k] = tot
            tot += (int(np.prod(shape)) * np.dtype(dt).itemsize + 255) // 256 * 256
        tot = max(tot, 1)
        with self.lock:
            if not self.closed:
                self._fold()
            lst = self.free.get(tot)
            p = lst.pop() if lst else None
            if p is None and self.total + tot <= self.cap:
                self.total += tot
                p = -1
        if p is None:
            return None
        if p == -1:
            q = C.c_void_p()
            if _abi.load().ffddp_host_alloc(tot, C.byref(q)) != 0:
                with self.lock:
                    self.total -= tot
                return None
            p = q.value
        buf = (C.c_char * tot).from_address(p)
        weakref.finalize(buf, self._give_back, tot, p)
        return {k: np.frombuffer(buf, dtype=dt, count=int(np.prod(shape)), offset=offs[k]).reshape(shape)
                for k, (shape, dt) in specs.items()}

    def _give_back(self, tot, p):
        self.returned.append((tot, p))
        if self.closed:
            self._free_returned()

    def _free_returned(self):
        lib = _abi.load()
        while True:
            try:
                _, p = self.returned.popleft()
            except IndexError:
                return
            lib.ffddp_host_free(C.c_void_p(p))

    def close(self):
        with self.lock:
            self.closed = True  # from here on a finalizer frees what it appends
            self._fold()
            free, self.free = self.free, {}
        lib = _abi.load()
        for lst in free.values():
            for p in lst:
                lib.ffddp_host_free(C.c_void_p(p))
        self._free_returned()


class BatchedBoxFDDP:
    def __init__(self, cfg: OcpConfig, max_batch: int, device: int = 0, pinned_outputs: bool = False,
                 outputs: str | None = None, robot=None, mount=None):
        """robot: a robot.LinkModel, the inertial parameters this handle plans
        with in place of the nominal Panda's (the kinematics stay).
        mount: a robot.Mount, the base placement and gravity vector this handle
        plans with in place of the nominal ones.
        outputs: how solve() returns xs / us / K / cost / ...:
          "recycled" (default): fresh numpy arrays per solve() in page-locked
              memory recycled from earlier solves whose arrays are gone
              (_RecycledPinned; up to 4 solves' worth at max_batch), filled by
              DMA as each slice finishes;
          "fresh": fresh pageable numpy arrays per solve() (np.zeros, filled
              through the library's staging buffer);
          "pinned" (or pinned_outputs=True): page-locked arrays owned by the
              solver and overwritten by the next solve() -- copy what must
              outlive it, as the reference does (crocoddyl_classical.py:
              382-385)."""
        self.cfg = cfg
        self.robot = robot
        self.mount = mount
        if outputs is None:
            outputs = "pinned" if pinned_outputs else "recycled"
        if outputs not in ("recycled", "fresh", "pinned"):
            raise ValueError(f"outputs={outputs!r}")
        self.outputs = outputs
        self.pinned_outputs = outputs == "pinned"
        self._pin = {}
        self._pool = None
        self._callbacks = []
        self._trace_it = 0
        self._plans = weakref.WeakSet()  # live SolvePlans: closed before the handle
        self.N = int(cfg.horizon)
        self.nx = cfg.nx
        self.nu = 7
        self.max_batch = int(max_batch)
        self._lib = _abi.load()
        self._cfg_struct = cfg.to_struct()
        h = C.c_void_p()
        rc = self._lib.ffddp_create(
            C.byref(_abi.robot_struct() if robot is None and mount is None else _abi.make_robot(robot, mount)),
            C.byref(self._cfg_struct),
            int(device), self.max_batch, C.byref(h)
        )
        if rc != 0:
            raise FfddpError(f"ffddp_create failed with code {rc}")
        self._h = h
        self.xs = self.us = self.K = self.cost = self.iter = self.ok = self.fn_pred = self.stats = None
        if outputs == "recycled":
            N, nx, Bm = self.N, self.nx, self.max_batch
            one = 8 * Bm * ((N + 1) * nx + N * 7 + N * 7 * nx + 1 + 2) + 4 * Bm * (1 + _abi.NSTATS) + Bm + 8 * 256
            self._pool = _RecycledPinned(4 * one)

    # -- solver properties (crocoddyl SolverFDDP / SolverBoxFDDP attributes) ----------
    @property
    def solver_params(self) -> _abi.SolverParams:
        p = _abi.SolverParams()
        self._check(self._lib.ffddp_get_solver_params(self._h, C.byref(p)), "ffddp_get_solver_params")
        return p

    @solver_params.setter
    def solver_params(self, p: _abi.SolverParams):
        self._check(self._lib.ffddp_set_solver_params(self._h, C.byref(p)), "ffddp_set_solver_params")

    def __getattr__(self, name):
        if name in _PARAMS:
            return getattr(self.solver_params, name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _PARAMS:
            p = self.solver_params
            setattr(p, name, value)
            self.solver_params = p
        else:
            object.__setattr__(self, name, value)

    # -- callbacks / per-iteration trace ------------------------------------------------
    def setCallbacks(self, callbacks, max_iters: int = 64):
        """crocoddyl solver.setCallbacks (crocoddyl_classical.py:353): the device
        keeps a per-iteration record (include/ffddp.h ffddp_trace_*); every
        callback is called with (solver, trace) after each solve."""
        callbacks = list(callbacks)
        self.trace_enable(max_iters if callbacks else 0)  # raises while a SolvePlan is open
        self._callbacks = callbacks

    def getCallbacks(self):
        return list(self._callbacks)

    def trace_enable(self, max_iters: int):
        """Fails (FfddpError) while a SolvePlan of this solver is open: a
        plan's graph keeps the trace buffer it was captured with."""
        self._check(self._lib.ffddp_trace_enable(self._h, int(max_iters)), "ffddp_trace_enable")
        self._trace_it = int(max_iters)

    def trace(self, B: int | None = None) -> np.ndarray:
        """[B][max_iters][TRACE_W] records of the last solve (NaN rows for
        iterations an instance did not run); fields _abi.TRACE_FIELDS."""
        if self._trace_it == 0:
            raise FfddpError("trace not enabled (trace_enable / setCallbacks)")
        B = int(self.cost.shape[0]) if B is None else int(B)
        out = np.zeros((B, self._trace_it, _abi.TRACE_W))
        self._check(self._lib.ffddp_trace_read(self._h, B, _abi.dptr(out)), "ffddp_trace_read")
        return out

    def _run_callbacks(self, B):
        if self._callbacks:
            tr = self.trace(B)
            for cb in self._callbacks:
                cb(self, tr)

    # -- lifecycle ------------------------------------------------------------------
    def close(self):
        for plan in list(getattr(self, "_plans", ())):
            plan.close()
        if getattr(self, "_pool", None) is not None:
            self._pool.close()
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ffddp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.ffddp_last_error(self._h)
            raise FfddpError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    # -- solve (host arrays) ----------------------------------------------------------
    def pinned_batch(self, batch):
        """A copy of `batch`'s solve inputs in page-locked host memory
        (ffddp_host_alloc): solve() then copies them by DMA per slice on the
        slice streams, overlapping the other slices' kernels, instead of
        staging them.  For callers that refill the same input arrays every
        tick."""
        import types

        B, N, nx = int(batch.x0.shape[0]), self.N, self.nx
        specs = dict(x0=((B, nx), np.float64), node_ref=((B, N + 1, 6), np.float64),
                     inst_ref=((B, 21), np.float64), surface=((B,), np.uint8),
                     xs_init=((B, N + 1, nx), np.float64), us_init=((B, N, 7), np.float64))
        o = _abi.pinned_arrays(specs)
        for k, (shape, dt) in specs.items():
            o[k][...] = np.asarray(getattr(batch, k), dt).reshape(shape)
        return types.SimpleNamespace(**o)

    def solve(self, batch, maxiter: int = 10, is_feasible: bool = False, xs_init=None, us_init=None):
        """batch: workload.Batch (or any object with x0, node_ref, inst_ref, surface,
        xs_init, us_init).  Returns ok (B,) bool."""
        B = int(batch.x0.shape[0])
        N, nx = self.N, self.nx
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))
        x0 = f(batch.x0, (B, nx))
        nref = f(batch.node_ref, (B, N + 1, 6))
        iref = f(batch.inst_ref, (B, 21))
        surf = np.ascontiguousarray(np.asarray(batch.surface, np.uint8).reshape(B))
        xsi = f(batch.xs_init if xs_init is None else xs_init, (B, N + 1, nx))
        usi = f(batch.us_init if us_init is None else us_init, (B, N, 7))
        specs = dict(xs=((B, N + 1, nx), np.float64), us=((B, N, 7), np.float64), K=((B, N, 7, nx), np.float64),
                     cost=((B,), np.float64), iters=((B,), np.int32), ok=((B,), np.uint8), fn=((B, 2), np.float64),
                     stats=((B, _abi.NSTATS), np.int32))
        o = None
        if self.outputs == "pinned":
            if B not in self._pin:
                self._pin = {B: _abi.pinned_arrays(specs)}
            o = self._pin[B]
        elif self.outputs == "recycled":
            o = self._pool.arrays(specs)
        if o is None:
            o = {k: np.zeros(shape, dt) for k, (shape, dt) in specs.items()}
        xs, us, K, cost, iters, ok, fn, stats = (o[k] for k in ("xs", "us", "K", "cost", "iters", "ok", "fn", "stats"))
        d, i, u = _abi.dptr, _abi.iptr, _abi.uptr
        rc = self._lib.ffddp_solve_batch(
            self._h, B, d(x0), d(nref), d(iref), u(surf), d(xsi), d(usi), int(maxiter), int(bool(is_feasible)),
            d(xs), d(us), d(K), d(cost), i(iters), u(ok), d(fn), i(stats),
        )
        self._check(rc, "ffddp_solve_batch")
        self.xs, self.us, self.K, self.cost, self.iter = xs, us, K, cost, iters
        self.ok, self.fn_pred, self.stats = ok.astype(bool), fn, stats
        self._run_callbacks(B)
        return self.ok

    # -- solve plan (receding-horizon loop: one graph launch per tick) -----------------
    def plan(self, B: int, maxiter: int = 10, is_feasible: bool = False) -> "SolvePlan":
        """ffddp_plan_create: the host-array solve of B instances captured as one
        HIP graph; see SolvePlan."""
        plan = SolvePlan(self, B, maxiter, is_feasible)
        self._plans.add(plan)
        return plan

    # -- solve (device-resident torch tensors; bench path) ---------------------------
    def solve_dev(self, t, maxiter: int = 10, is_feasible: bool = False, stream=None, active=None, force_ref=None,
                  cost_weights=None, torque_limits=None, link_model=None, mount=None):
        """t: dict of contiguous torch.cuda tensors with keys x0, node_ref, inst_ref,
        surface (uint8), xs_init, us_init and outputs xs, us, K, cost, iters (int32),
        ok (uint8), fn_pred, stats (int32).  Asynchronous on `stream` (hipStream_t int).
        active: optional (B,) uint8 device tensor, the instances that solve
        (ffddp_solve_batch_sel_dev); the others' input rows are not read and
        their output rows not written.
        force_ref: optional (B, N+1) float64 device tensor, the desired normal
        contact force of every instance and node in place of the
        configuration's fn_des (ffddp_solve_batch_fref_dev); goes with or
        without `active`.
        cost_weights: optional (B, _abi.COST_W) float64 device tensor, one row of
        scalar cost weights per instance in place of the configuration's
        (ffddp_solve_batch_wts_dev; config.cost_weight_row builds a row); goes
        with or without `active` and `force_ref`.
        torque_limits: optional (B, _abi.TAU_LIM_W) float64 device tensor, one
        torque-limit row per instance in place of the configuration's
        tau_limits (ffddp_solve_batch_lim_dev; config.torque_limit_rows builds
        the rows); goes with or without the other three.
        link_model: optional (B, _abi.LINK_W) float64 device tensor, one row of
        link inertial parameters per instance in place of the handle's robot's
        (ffddp_solve_batch_mdl_dev; config.link_model_rows builds the rows);
        goes with or without the other four.  t["inst_ref"] stays the caller's:
        gravity_torque_dev(link_model=...) gives the torque reference under
        each instance's model.
        mount: optional (B, _abi.MOUNT_W) float64 device tensor, one row of
        base placement and gravity per instance in place of the handle's
        robot's (ffddp_solve_batch_mnt_dev; config.mount_rows builds the rows);
        goes with or without the other five.  The references in t are the
        caller's, in each instance's planning world; gravity_torque_dev(mount=
        ...) gives the torque reference under each instance's mount."""
        B = int(t["x0"].shape[0])
        p = lambda k: C.c_void_p(int(t[k].data_ptr()))
        rc = self._lib.ffddp_solve_batch_mnt_dev(
            self._h, B, p("x0"), p("node_ref"), p("inst_ref"), p("surface"), p("xs_init"), p("us_init"),
            int(maxiter), int(bool(is_feasible)), p("xs"), p("us"), p("K"), p("cost"), p("iters"), p("ok"),
            p("fn_pred"), p("stats"),
            _opt_dev_ptr(active, "uint8", (B,), "active must be a contiguous (B,) uint8 device tensor"),
            _opt_dev_ptr(force_ref, "float64", (B, self.N + 1),
                         "force_ref must be a contiguous (B, N+1) float64 device tensor"),
            _opt_dev_ptr(cost_weights, "float64", (B, _abi.COST_W),
                         "cost_weights must be a contiguous (B, COST_W) float64 device tensor"),
            _opt_dev_ptr(torque_limits, "float64", (B, _abi.TAU_LIM_W),
                         "torque_limits must be a contiguous (B, TAU_LIM_W) float64 device tensor"),
            _opt_dev_ptr(link_model, "float64", (B, _abi.LINK_W),
                         "link_model must be a contiguous (B, LINK_W) float64 device tensor"),
            _opt_dev_ptr(mount, "float64", (B, _abi.MOUNT_W),
                         "mount must be a contiguous (B, MOUNT_W) float64 device tensor"),
            C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_solve_batch_mnt_dev")

    def gravity_torque_dev(self, q, tau, link_model=None, stream=None, mount=None):
        """tau (B, 7) = rnea(q, 0, 0) for q (B, 7), contiguous float64 device
        tensors (ffddp_gravity_torque_dev), under the handle's robot; with
        link_model, (B, _abi.LINK_W) float64 device rows, under each instance's
        own model, and with mount, (B, _abi.MOUNT_W) float64 device rows, under
        each instance's own base placement and gravity
        (ffddp_gravity_torque_mnt_dev).  Asynchronous on `stream`."""
        B = int(q.shape[0])
        assert tuple(q.shape) == (B, 7) and tuple(tau.shape) == (B, 7) and q.is_contiguous() and tau.is_contiguous()
        assert q.is_cuda and tau.is_cuda and str(q.dtype) == str(tau.dtype) == "torch.float64"
        rc = self._lib.ffddp_gravity_torque_mnt_dev(
            self._h, B, C.c_void_p(int(q.data_ptr())),
            _opt_dev_ptr(link_model, "float64", (B, _abi.LINK_W),
                         "link_model must be a contiguous (B, LINK_W) float64 device tensor"),
            _opt_dev_ptr(mount, "float64", (B, _abi.MOUNT_W),
                         "mount must be a contiguous (B, MOUNT_W) float64 device tensor"),
            C.c_void_p(int(tau.data_ptr())), C.c_void_p(stream if stream else 0))
        self._check(rc, "ffddp_gravity_torque_mnt_dev")

    def fleet_obs_frame_dev(self, obs, frame, obs_out, sel=None, stream=None):
        """obs_out (B, >= 69) = the plant records obs (B, >= 69) re-expressed in
        each instance's planning frame, frame (B, _abi.FRAME_W) float64 device
        rows (robot.Mount.obs_frame: R, p in the MuJoCo world), in one launch
        (ffddp_fleet_obs_frame_dev).  sel: optional (B,) uint8 device tensor;
        an instance with sel[b] == 0 is copied verbatim.  Row-contiguous
        float64 device tensors; obs_out must not overlap obs.  Asynchronous on
        `stream`."""
        B = int(obs.shape[0])
        for a in (obs, obs_out):
            assert a.is_cuda and str(a.dtype) == "torch.float64" and a.dim() == 2 and a.stride(1) == 1
        assert int(obs_out.shape[0]) == B
        rc = self._lib.ffddp_fleet_obs_frame_dev(
            self._h, B, C.c_void_p(int(obs.data_ptr())), int(obs.stride(0)),
            _opt_dev_ptr(frame, "float64", (B, _abi.FRAME_W),
                         "frame must be a contiguous (B, FRAME_W) float64 device tensor"),
            _opt_dev_ptr(sel, "uint8", (B,), "sel must be a contiguous (B,) uint8 device tensor"),
            C.c_void_p(int(obs_out.data_ptr())), int(obs_out.stride(0)), C.c_void_p(stream if stream else 0))
        self._check(rc, "ffddp_fleet_obs_frame_dev")

    # -- fleet tick glue (include/ffddp.h: ffddp_fleet_warm_start_dev / ffddp_fleet_keep_dev) --
    def fleet_warm_start_dev(self, t, stream=None):
        """t["xs_init"], t["us_init"] from t["x0"], t["u_cold"] (B, 7), t["valid"]
        (uint8) and the kept solution t["keep_xs"], t["keep_us"]: the controllers'
        _shift_guess for B instances in one launch.  Asynchronous on `stream`."""
        B = int(t["x0"].shape[0])
        p = lambda k: C.c_void_p(int(t[k].data_ptr()))
        rc = self._lib.ffddp_fleet_warm_start_dev(
            self._h, B, p("x0"), p("u_cold"), p("valid"), p("keep_xs"), p("keep_us"), p("xs_init"), p("us_init"),
            C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_fleet_warm_start_dev")

    def fleet_keep_dev(self, t, stream=None):
        """After solve_dev(t): instances whose us[0] is finite replace the kept
        solution t["keep_xs"], t["keep_us"], t["keep_K"]; t["first"]
        (B, _abi.fleet_first_w(nx)) takes the packed first-knot record.
        Asynchronous on `stream`."""
        B = int(t["x0"].shape[0])
        p = lambda k: C.c_void_p(int(t[k].data_ptr()))
        rc = self._lib.ffddp_fleet_keep_dev(
            self._h, B, p("xs"), p("us"), p("K"), p("cost"), p("iters"), p("ok"), p("fn_pred"), p("stats"),
            p("keep_xs"), p("keep_us"), p("keep_K"), p("first"), C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_fleet_keep_dev")

    # -- fleet closed loop on the device (include/ffddp.h: ffddp_fleet_pre_dev / ffddp_fleet_post_dev) --
    @staticmethod
    def _fleet_state(t) -> _abi.FleetState:
        s = _abi.FleetState()
        for k, _ in _abi.FleetState._fields_:
            setattr(s, k, int(t[k].data_ptr()))
        return s

    @staticmethod
    def _fleet_sched(t, sched: _abi.FleetSched) -> _abi.FleetSched:
        """A copy of `sched` pointing at t["since"], t["age"] (int32) and t["need"] (uint8), all (B,)."""
        import torch

        s = _abi.FleetSched.from_buffer_copy(sched)
        for k, dt in (("since", torch.int32), ("age", torch.int32), ("need", torch.uint8)):
            assert t[k].dtype == dt and t[k].is_contiguous() and t[k].shape[0] >= t["x0"].shape[0], k
            setattr(s, k, int(t[k].data_ptr()))
        return s

    @staticmethod
    def fleet_tasks(rec, p_site_minus_frame, t: float = 0.0) -> _abi.FleetTasks:
        """ffddp_fleet_tasks over the device tensor rec (B, _abi.FLEET_TASK_W)
        float64 (trajectory.task_records, uploaded) with the site offset and
        the tick's time.  The struct holds the pointer: keep the tensor alive."""
        assert rec.is_cuda and rec.is_contiguous() and rec.dim() == 2 and rec.shape[1] == _abi.FLEET_TASK_W
        assert str(rec.dtype) == "torch.float64"
        k = _abi.FleetTasks()
        k.p_site_minus_frame[:] = [float(x) for x in np.asarray(p_site_minus_frame, float).reshape(3)]
        k.t, k.rec = float(t), int(rec.data_ptr())
        return k

    def fleet_task_refs_dev(self, tasks: _abi.FleetTasks, t, node_ref, hint, stream=None):
        """The device task sampler alone: t (B,) float64, the instances' task
        times (the delay already subtracted) -> node_ref (B, N+1, 6) and hint
        (B,) uint8, the surface flag at t.  Asynchronous on `stream`."""
        B = int(t.shape[0])
        assert t.is_contiguous() and node_ref.is_contiguous() and hint.is_contiguous()
        assert tuple(node_ref.shape) == (B, self.N + 1, 6) and tuple(hint.shape) == (B,)
        rc = self._lib.ffddp_fleet_task_refs_dev(
            self._h, B, tasks, C.c_void_p(int(t.data_ptr())), C.c_void_p(int(node_ref.data_ptr())),
            C.c_void_p(int(hint.data_ptr())), C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_fleet_task_refs_dev")

    def fleet_force_refs_dev(self, force, force_ref, t: float = 0.0, tasks: _abi.FleetTasks = None, rows: int = None,
                             fn_default: float = 0.0, stream=None):
        """The device force-profile sampler (ffddp_fleet_force_refs_dev): force
        (rows, _abi.FLEET_FORCE_W) float64 on the device (trajectory.force_records,
        uploaded) -> force_ref (B, N+1), solve_dev's argument: knot k of instance
        b at (t - its task delay) + k dt_ocp.  tasks (fleet_tasks): its t and the
        records' delays are used; None: tick time `t`, no delay.  Instances
        beyond `rows` (by default the records given) take fn_default.
        Asynchronous on `stream`."""
        B = int(force_ref.shape[0])
        assert force.is_cuda and force.is_contiguous() and force.dim() == 2 and force.shape[1] == _abi.FLEET_FORCE_W
        assert tuple(force_ref.shape) == (B, self.N + 1) and force_ref.is_contiguous()
        assert str(force.dtype) == str(force_ref.dtype) == "torch.float64"
        rows = int(force.shape[0]) if rows is None else int(rows)
        assert rows <= int(force.shape[0])
        if tasks is None:
            tasks = _abi.FleetTasks()
            tasks.t = float(t)
        rc = self._lib.ffddp_fleet_force_refs_dev(
            self._h, B, tasks, C.c_void_p(int(force.data_ptr())), rows, float(fn_default),
            C.c_void_p(int(force_ref.data_ptr())), C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_fleet_force_refs_dev")

    def fleet_metrics_dev(self, acc, obs, t_phase, fn_des: float, tasks: _abi.FleetTasks = None, dt: float = 0.0,
                          rows: int = None, p_ref=None, ts: float = 0.0, info=None, need=None, plant_fail=None,
                          stream=None, force=None, rows_force: int = None):
        """Fold one plant record per instance into the task-metric accumulators
        (ffddp_fleet_metrics_dev; runlog.accumulate_metrics is the same step in
        numpy).  acc (_abi.FLEET_METRICS_W, ld >= B) float64, field-major; obs
        (B, >= 48) float64 rows laid out as the plant's records (a strided view
        will do); t_phase (B,) float64.  The reference position: tasks
        (fleet_tasks; instance b's own record at (tasks.t - its delay) + dt,
        `rows` records, by default B) or p_ref (3,) float64 on the device with
        the series time ts.  info (B, FLEET_INFO_W), need (B,) uint8 and
        plant_fail (B,) int32 are optional.  force (rows_force, _abi.FLEET_FORCE_W)
        float64 on the device: the force error is against each instance's own
        record at the series time (ffddp_fleet_metrics_fref_dev), fn_des beyond
        them.  Asynchronous on `stream`."""
        B = int(obs.shape[0])
        assert acc.dim() == 2 and acc.shape[0] == _abi.FLEET_METRICS_W and acc.is_contiguous() and acc.shape[1] >= B
        assert obs.stride(1) == 1 and obs.shape[1] >= 48 and tuple(t_phase.shape) == (B,) and t_phase.is_contiguous()
        assert str(acc.dtype) == str(obs.dtype) == str(t_phase.dtype) == "torch.float64"
        assert info is None or (tuple(info.shape) == (B, _abi.FLEET_INFO_W) and info.is_contiguous())
        assert need is None or (tuple(need.shape) == (B,) and need.is_contiguous())
        assert plant_fail is None or (tuple(plant_fail.shape) == (B,) and plant_fail.is_contiguous())
        assert p_ref is None or (p_ref.numel() == 3 and p_ref.is_contiguous())
        p = lambda a: C.c_void_p(int(a.data_ptr()) if a is not None else 0)  # noqa: E731
        rf = 0
        if force is not None:
            assert force.is_cuda and force.is_contiguous() and force.dim() == 2 and force.shape[1] == _abi.FLEET_FORCE_W
            assert str(force.dtype) == "torch.float64"
            rf = int(force.shape[0]) if rows_force is None else int(rows_force)
            assert rf <= int(force.shape[0])
        rc = self._lib.ffddp_fleet_metrics_fref_dev(
            self._h, B, int(acc.shape[1]), p(obs), int(obs.stride(0)), tasks if tasks is not None else _abi.FleetTasks(),
            B if rows is None else int(rows), float(dt), p(p_ref), float(ts), p(t_phase), float(fn_des), p(info),
            p(need), p(plant_fail), p(acc), p(force), rf, C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_fleet_metrics_fref_dev")

    def fleet_pre_dev(self, t, params: _abi.FleetParams, hint: bool = False, stream=None, sched: _abi.FleetSched = None,
                      tasks: _abi.FleetTasks = None, link_model=None, mount=None):
        """Everything a fleet tick does before the solve, for B instances in one
        launch.  Inputs t["q"], t["v"] (B, 7), t["fn_meas"], t["ee_z"] (B,),
        optionally t["contact"] (B,) and, for force feedback, t["tau_hat"]
        (B, 7) -- all may be strided views of the plant's records --
        t["q_nom"] (B, 7), t["node_ref1"] (N+1, 6) and the trajectory's contact
        `hint`; the controller state t["valid"], t["latched"] (uint8),
        t["loss_count"] (int32), t["prev_mode"] (int8), t["tau_prev"] and the
        kept solution.  Writes the state and the solve's inputs t["x0"],
        t["surface"], t["inst_ref"], t["node_ref"], t["xs_init"], t["us_init"].
        sched (_abi.fleet_sched): the scheduled tick (ffddp_fleet_pre_sched_dev)
        with the counters t["since"], t["age"] (int32); writes t["need"]
        (uint8), the solve's `active`, and warm starts only those instances.
        tasks (fleet_tasks): per-instance tasks (ffddp_fleet_pre_task_dev):
        every instance's references and hint are sampled from its record at
        tasks.t minus its delay; t["node_ref1"] and `hint` are not read.
        link_model: optional (B, _abi.LINK_W) float64 device tensor, the
        solve's link-model rows: the gravity torque reference is each
        instance's own (ffddp_fleet_pre_mdl_dev), with or without sched and
        tasks.  mount: optional (B, _abi.MOUNT_W) float64 device tensor, the
        solve's mount rows: the gravity torque reference is computed under each
        instance's own mount (ffddp_fleet_pre_mnt_dev), with or without the
        others.  Asynchronous on `stream`."""
        B = int(t["x0"].shape[0])
        p = lambda k: C.c_void_p(int(t[k].data_ptr()) if t.get(k) is not None else 0)
        assert t["q"].stride(0) == t["v"].stride(0) and t["fn_meas"].stride(0) == t["ee_z"].stride(0)
        assert t.get("contact") is None or t["contact"].stride(0) == t["fn_meas"].stride(0)
        th = t.get("tau_hat")
        st = self._fleet_state(t)
        head = (self._h, B, C.byref(params), C.byref(st), p("q"), p("v"), p("fn_meas"), p("contact"), p("ee_z"),
                int(t["q"].stride(0)), int(t["fn_meas"].stride(0)), p("tau_hat"),
                int(th.stride(0)) if th is not None else 0, p("q_nom"))
        tail = (p("x0"), p("surface"), p("inst_ref"), p("node_ref"), p("xs_init"), p("us_init"))
        if mount is not None:
            sp = C.byref(self._fleet_sched(t, sched)) if sched is not None else None
            rc = self._lib.ffddp_fleet_pre_mnt_dev(
                *head, tasks if tasks is not None else _abi.FleetTasks(), p("node_ref1"), int(bool(hint)), *tail, sp,
                _opt_dev_ptr(link_model, "float64", (B, _abi.LINK_W),
                             "link_model must be a contiguous (B, LINK_W) float64 device tensor"),
                _opt_dev_ptr(mount, "float64", (B, _abi.MOUNT_W),
                             "mount must be a contiguous (B, MOUNT_W) float64 device tensor"),
                C.c_void_p(stream if stream else 0))
            self._check(rc, "ffddp_fleet_pre_mnt_dev")
            return
        if link_model is not None:
            sp = C.byref(self._fleet_sched(t, sched)) if sched is not None else None
            rc = self._lib.ffddp_fleet_pre_mdl_dev(
                *head, tasks if tasks is not None else _abi.FleetTasks(), p("node_ref1"), int(bool(hint)), *tail, sp,
                _opt_dev_ptr(link_model, "float64", (B, _abi.LINK_W),
                             "link_model must be a contiguous (B, LINK_W) float64 device tensor"),
                C.c_void_p(stream if stream else 0))
            self._check(rc, "ffddp_fleet_pre_mdl_dev")
            return
        if tasks is not None:
            sp = C.byref(self._fleet_sched(t, sched)) if sched is not None else None
            rc = self._lib.ffddp_fleet_pre_task_dev(*head, tasks, *tail, sp, C.c_void_p(stream if stream else 0))
            self._check(rc, "ffddp_fleet_pre_task_dev")
            return
        args = head + (p("node_ref1"), int(bool(hint))) + tail
        if sched is not None:
            rc = self._lib.ffddp_fleet_pre_sched_dev(*args, self._fleet_sched(t, sched), C.c_void_p(stream if stream else 0))
            self._check(rc, "ffddp_fleet_pre_sched_dev")
            return
        rc = self._lib.ffddp_fleet_pre_dev(*args, C.c_void_p(stream if stream else 0))
        self._check(rc, "ffddp_fleet_pre_dev")

    def fleet_post_dev(self, t, params: _abi.FleetParams, lpf: float = 0.0, stream=None,
                       sched: _abi.FleetSched = None, torque_limits=None):
        """Everything a fleet tick does after solve_dev(t): keep, torque policy,
        unstable fallback and _safe_tau -> t["tau_cmd"] (B, 7), t["info"]
        (B, _abi.FLEET_INFO_W; fields _abi.FLEET_INFO_FIELDS) and the state.
        t["tau_bias"] (B, 7) may be a strided view.  Optional: t["tau_app"]
        (B, 7) = t["scale"] (B, 7) * tau_cmd, t["tau_filt"] (B, 7) low-passed by
        `lpf`, t["log_obs"] (B, _abi.FLEET_LOG_W) from the plant records
        t["obs"].  sched: the scheduled tick (ffddp_fleet_post_sched_dev), after
        solve_dev(t, active=t["need"]); reads t["need"], updates t["since"] and
        t["age"].  torque_limits: optional (B, _abi.TAU_LIM_W) float64 device
        tensor, the solve's torque-limit rows: the clips use each instance's own
        limit (ffddp_fleet_post_lim_dev), scheduled or not.  Asynchronous on
        `stream`."""
        B = int(t["x0"].shape[0])
        p = lambda k: C.c_void_p(int(t[k].data_ptr()) if t.get(k) is not None else 0)
        st = self._fleet_state(t)
        obs = t.get("obs")
        args = (self._h, B, C.byref(params), C.byref(st), p("xs"), p("us"), p("K"), p("cost"), p("iters"), p("ok"),
                p("fn_pred"), p("stats"), p("x0"), p("surface"), p("tau_bias"), int(t["tau_bias"].stride(0)),
                p("tau_cmd"), p("info"), p("scale"), p("tau_app"), p("tau_filt"), float(lpf), p("obs"),
                int(obs.stride(0)) if obs is not None else 0, p("log_obs"))
        if torque_limits is not None:
            sp = C.byref(self._fleet_sched(t, sched)) if sched is not None else None
            rc = self._lib.ffddp_fleet_post_lim_dev(
                *args, sp, _opt_dev_ptr(torque_limits, "float64", (B, _abi.TAU_LIM_W),
                                        "torque_limits must be a contiguous (B, TAU_LIM_W) float64 device tensor"),
                C.c_void_p(stream if stream else 0))
            self._check(rc, "ffddp_fleet_post_lim_dev")
            return
        if sched is not None:
            rc = self._lib.ffddp_fleet_post_sched_dev(*args, self._fleet_sched(t, sched), C.c_void_p(stream if stream else 0))
            self._check(rc, "ffddp_fleet_post_sched_dev")
            return
        rc = self._lib.ffddp_fleet_post_dev(*args, C.c_void_p(stream if stream else 0))
        self._check(rc, "ffddp_fleet_post_dev")

    # -- the uncertainty injector around the tick (include/ffddp.h: ffddp_fleet_inject_*_dev) --
    @staticmethod
    def fleet_inject(t, d_obs: int, d_cmd: int, sigma, lpf: float, noise: str) -> _abi.FleetInject:
        """ffddp_fleet_inject from the delays (ticks), sigma = (sigma_q,
        sigma_dq, sigma_tau), the measurement filter's alpha, the noise source
        ("numpy": a pre-drawn table, "philox": generated on the device) and the
        device tensors t["row"] (B,) int32, t["a"], t["b"] (rows,),
        t["seed"] (rows,) uint64 bits (philox; else optional), t["obs_ring"]
        (d_obs + 1, B, 14), t["cmd_ring"] (d_cmd + 1, B, 7), t["tau_hat_filt"],
        t["z_cmd"] (B, 7).  The struct holds the pointers: keep the tensors alive."""
        if noise not in _abi.INJECT_NOISE_MODES:
            raise ValueError(f"fleet_inject: unknown noise source {noise!r} (numpy or philox)")
        B = int(t["row"].shape[0])
        assert tuple(t["obs_ring"].shape) == (int(d_obs) + 1, B, 14) and tuple(t["cmd_ring"].shape) == (int(d_cmd) + 1, B, 7)
        assert t["a"].shape == t["b"].shape and (t.get("seed") is None or t["seed"].shape == t["a"].shape)
        inj = _abi.FleetInject()
        inj.d_obs, inj.d_cmd, inj.noise, inj.rows = int(d_obs), int(d_cmd), _abi.INJECT_NOISE_MODES[noise], int(t["a"].shape[0])
        inj.sigma_q, inj.sigma_dq, inj.sigma_tau = (float(s) for s in sigma)
        inj.lpf = float(lpf)
        for k in ("row", "a", "b", "seed", "obs_ring", "cmd_ring", "tau_hat_filt", "z_cmd"):
            assert t.get(k) is None or t[k].is_contiguous()
            setattr(inj, k, int(t[k].data_ptr()) if t.get(k) is not None else 0)
        return inj

    @staticmethod
    def fleet_inject_rows(t) -> _abi.FleetInjectRows:
        """ffddp_fleet_inject_rows from the device tensors t["d_obs"], t["d_cmd"]
        (rows,) int32 -- each row's delays in ticks, at most the ring depths of
        the ffddp_fleet_inject they go with -- and t["sigma"] (rows, 3)
        float64; a missing one leaves that member null (the scalar holds).
        The delays are read back once and checked against the depths of
        t["obs_ring"] / t["cmd_ring"] (ValueError; the kernels would clamp
        them).  The struct holds the pointers: keep the tensors alive."""
        import torch

        w = _abi.FleetInjectRows()
        n = int(t["a"].shape[0]) if t.get("a") is not None else None
        for k, dt, tail in (("d_obs", torch.int32, ()), ("d_cmd", torch.int32, ()), ("sigma", torch.float64, (3,))):
            a = t.get(k)
            if a is not None:
                assert a.dtype == dt and a.is_contiguous() and tuple(a.shape[1:]) == tail and n in (None, int(a.shape[0]))
            setattr(w, k, int(a.data_ptr()) if a is not None else 0)
        for k, ring in (("d_obs", "obs_ring"), ("d_cmd", "cmd_ring")):
            if t.get(k) is not None and t.get(ring) is not None and t[k].numel():
                d, depth = t[k].cpu().numpy(), int(t[ring].shape[0]) - 1
                if d.min() < 0 or d.max() > depth:
                    raise ValueError(f"fleet_inject_rows: {k} must lie in 0..{depth} (the depth of {ring}), "
                                     f"got {int(d.min())}..{int(d.max())}")
        return w

    def fleet_inject_obs_dev(self, t, inj: _abi.FleetInject, k: int, z=None, stream=None, rows=None):
        """Tick k's observation_for_controller for B instances in one launch,
        enqueued after the plant step and before fleet_pre_dev.  t["q"], t["v"]
        (B, 7): the plant's true state (strided views of its records); z
        (rows, 28): tick k's row of uncertainty.predraw's table (numpy noise).
        Writes t["qv_ctrl"] (B, 14), optionally t["tau_hat"] and t["tau_ctrl"]
        (B, 7: the raw and the filtered torque measurement), and the injector
        state in `inj`; instances with row -1 pass (q, v) and, when given,
        t["tau_filt"] (B, 7) through.  rows: fleet_inject_rows' struct, each
        instance's own delays and sigmas (ffddp_fleet_inject_obs_rows_dev);
        None: the scalars of `inj`.  Asynchronous on `stream`."""
        B = int(t["qv_ctrl"].shape[0])
        p = lambda k_: C.c_void_p(int(t[k_].data_ptr()) if t.get(k_) is not None else 0)
        assert t["q"].stride(0) == t["v"].stride(0) and t["qv_ctrl"].is_contiguous()
        assert z is None or (z.is_contiguous() and tuple(z.shape) == (inj.rows, _abi.INJECT_NZ))
        args = (self._h, B, C.byref(inj), int(k), C.c_void_p(int(z.data_ptr()) if z is not None else 0), p("q"), p("v"),
                int(t["q"].stride(0)), p("tau_filt"), p("qv_ctrl"), p("tau_hat"), p("tau_ctrl"))
        rc = self._lib.ffddp_fleet_inject_obs_rows_dev(*args, C.byref(rows) if rows is not None else None,
                                                       C.c_void_p(stream if stream else 0))
        self._check(rc, "ffddp_fleet_inject_obs_rows_dev")

    def fleet_inject_cmd_dev(self, t, inj: _abi.FleetInject, k: int, stream=None, rows=None):
        """Tick k's command_for_plant, enqueued after fleet_post_dev and before
        the next plant step: t["tau_app"] (B, 7) of the injected instances
        becomes a * (delayed t["tau_cmd"]) + b + noise; the others keep what
        post wrote.  rows: as fleet_inject_obs_dev's.  Asynchronous on `stream`."""
        B = int(t["tau_cmd"].shape[0])
        args = (self._h, B, C.byref(inj), int(k), C.c_void_p(int(t["tau_cmd"].data_ptr())),
                C.c_void_p(int(t["tau_app"].data_ptr())))
        rc = self._lib.ffddp_fleet_inject_cmd_rows_dev(*args, C.byref(rows) if rows is not None else None,
                                                       C.c_void_p(stream if stream else 0))
        self._check(rc, "ffddp_fleet_inject_cmd_rows_dev")

    def fleet_noise_dev(self, seed, k: int, z, words=None, stream=None):
        """The device Philox source alone: z (B, 28) float64 <- tick k's normals
        of the streams keyed by seed (B,) (uint64 bits in an int64 tensor), as
        uncertainty.philox_normals; words (B, 7, 4) int64, optional, takes the
        raw blocks.  Asynchronous on `stream`."""
        B = int(seed.shape[0])
        assert tuple(z.shape) == (B, _abi.INJECT_NZ) and z.is_contiguous() and seed.is_contiguous()
        assert words is None or (tuple(words.shape) == (B, 7, 4) and words.is_contiguous())
        rc = self._lib.ffddp_fleet_noise_dev(
            self._h, B, C.c_void_p(int(seed.data_ptr())), int(k), C.c_void_p(int(z.data_ptr())),
            C.c_void_p(int(words.data_ptr()) if words is not None else 0), C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_fleet_noise_dev")

    # -- device-side problem builder ----------------------------------------------
    def build_problem_dev(self, task, t, stream=None):
        """Fill t["node_ref"], t["inst_ref"], t["surface"] on the device from
        t["t0"] (B,) and t["x0"] (B, nx) for `task` (_abi.Task / make_task):
        _build_problem's references (crocoddyl_classical.py:521-556) for B
        instances in one launch.  Asynchronous on `stream`."""
        B = int(t["x0"].shape[0])
        p = lambda k: C.c_void_p(int(t[k].data_ptr()))
        rc = self._lib.ffddp_build_problem_dev(
            self._h, B, C.byref(task), p("t0"), p("x0"), p("node_ref"), p("inst_ref"), p("surface"),
            C.c_void_p(stream if stream else 0),
        )
        self._check(rc, "ffddp_build_problem_dev")

    # -- per-kernel device timing ----------------------------------------------------
    def profile(self, on=True):
        """on: True (every kernel class), False, or an iterable of class names
        from _abi.KERNEL_CLASSES to time only those."""
        if on is True:
            mask = (1 << len(_abi.KERNEL_CLASSES)) - 1
        elif not on:
            mask = 0
        else:
            mask = 0
            for name in on:
                mask |= 1 << _abi.KERNEL_CLASSES.index(name)
        self._check(self._lib.ffddp_profile_enable(self._h, int(mask)), "ffddp_profile_enable")

    def profile_read(self, reset: bool = True) -> dict:
        ms = np.zeros(len(_abi.KERNEL_CLASSES))
        n = np.zeros(len(_abi.KERNEL_CLASSES), np.int64)
        self._check(
            self._lib.ffddp_profile_read(self._h, _abi.dptr(ms), n.ctypes.data_as(C.POINTER(C.c_int64)), int(reset)),
            "ffddp_profile_read",
        )
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(_abi.KERNEL_CLASSES)}

    # -- problem.calcDiff(xs, us) -------------------------------------------------------
    def calc_diff(self, batch, xs, us, force_ref=None, cost_weights=None, torque_limits=None, link_model=None,
                  mount=None):
        """force_ref: optional (B, N+1) host array, the desired normal contact
        force per instance and node (ffddp_calc_diff_fref).  cost_weights:
        optional (B, _abi.COST_W) host array, the scalar cost weights per
        instance (ffddp_calc_diff_wts).  torque_limits: optional
        (B, _abi.TAU_LIM_W) host array, the torque-limit rows per instance
        (ffddp_calc_diff_lim).  link_model: optional (B, _abi.LINK_W) host
        array, the link-model rows per instance (ffddp_calc_diff_mdl).  mount:
        optional (B, _abi.MOUNT_W) host array, the mount rows per instance
        (ffddp_calc_diff_mnt)."""
        B = int(batch.x0.shape[0])
        N, nx = self.N, self.nx
        f = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))
        out = dict(
            Fx=np.zeros((B, N, nx, nx)), Fu=np.zeros((B, N, nx, 7)), Lx=np.zeros((B, N + 1, nx)),
            Lu=np.zeros((B, N, 7)), Lxx=np.zeros((B, N + 1, nx, nx)), Lxu=np.zeros((B, N, nx, 7)),
            Luu=np.zeros((B, N, 7, 7)), cost=np.zeros((B, N + 1)), xnext=np.zeros((B, N, nx)),
            lam=np.zeros((B, N + 1, 3)),
        )
        d = _abi.dptr
        fr = cw = ul = md = mt = None
        if force_ref is not None:
            fr = np.asarray(force_ref, np.float64)
            if fr.shape != (B, N + 1):
                raise ValueError("force_ref must have shape (B, N+1)")
            fr = np.ascontiguousarray(fr)
        if cost_weights is not None:
            cw = np.asarray(cost_weights, np.float64)
            if cw.shape != (B, _abi.COST_W):
                raise ValueError("cost_weights must have shape (B, COST_W)")
            cw = np.ascontiguousarray(cw)
        if torque_limits is not None:
            ul = np.asarray(torque_limits, np.float64)
            if ul.shape != (B, _abi.TAU_LIM_W):
                raise ValueError("torque_limits must have shape (B, TAU_LIM_W)")
            ul = np.ascontiguousarray(ul)
        if link_model is not None:
            md = np.asarray(link_model, np.float64)
            if md.shape != (B, _abi.LINK_W):
                raise ValueError("link_model must have shape (B, LINK_W)")
            md = np.ascontiguousarray(md)
        if mount is not None:
            mt = np.asarray(mount, np.float64)
            if mt.shape != (B, _abi.MOUNT_W):
                raise ValueError("mount must have shape (B, MOUNT_W)")
            mt = np.ascontiguousarray(mt)
        rc = self._lib.ffddp_calc_diff_mnt(
            self._h, B, d(f(batch.x0, (B, nx))), d(f(batch.node_ref, (B, N + 1, 6))), d(f(batch.inst_ref, (B, 21))),
            _abi.uptr(np.ascontiguousarray(np.asarray(batch.surface, np.uint8))), d(f(xs, (B, N + 1, nx))),
            d(f(us, (B, N, 7))), d(fr) if fr is not None else None, d(cw) if cw is not None else None,
            d(ul) if ul is not None else None, d(md) if md is not None else None, d(mt) if mt is not None else None,
            d(out["Fx"]),
            d(out["Fu"]), d(out["Lx"]), d(out["Lu"]), d(out["Lxx"]), d(out["Lxu"]), d(out["Luu"]), d(out["cost"]),
            d(out["xnext"]), d(out["lam"]),
        )
        self._check(rc, "ffddp_calc_diff_mnt")
        return out


class SolvePlan:
    """A captured solve of a fixed batch (include/ffddp.h ffddp_plan_*): the
    per-tick solve of a receding-horizon loop (crocoddyl_classical.py:367,
    run_classical.py:412) as one graph launch -- inputs up, every kernel,
    outputs down.  Fill the input views (x0, node_ref, inst_ref, surface,
    xs_init, us_init: page-locked numpy arrays owned by the plan) in place,
    call run(); the output views (xs, us, K, cost, iter, ok, fn_pred, stats)
    hold the last run's solution and are overwritten by the next run, so copy
    what must outlive it.  Same results as BatchedBoxFDDP.solve, bit for bit."""

    def __init__(self, solver: BatchedBoxFDDP, B: int, maxiter: int, is_feasible: bool):
        self.solver, self.B, self.maxiter = solver, int(B), int(maxiter)
        lib = solver._lib
        io = _abi.PlanIO()
        h = C.c_void_p()
        solver._check(lib.ffddp_plan_create(solver._h, self.B, self.maxiter, int(bool(is_feasible)), C.byref(h),
                                            C.byref(io)), "ffddp_plan_create")
        self._h, self._lib = h, lib
        B, N, nx = self.B, solver.N, solver.nx

        def view(ptr, shape, ct, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=shape).view(dt)

        f, i32, u8 = C.c_double, C.c_int32, C.c_uint8
        self.x0 = view(io.x0, (B, nx), f, np.float64)
        self.node_ref = view(io.node_ref, (B, N + 1, 6), f, np.float64)
        self.inst_ref = view(io.inst_ref, (B, 21), f, np.float64)
        self.surface = view(io.surface, (B,), u8, np.uint8)
        self.xs_init = view(io.xs_init, (B, N + 1, nx), f, np.float64)
        self.us_init = view(io.us_init, (B, N, 7), f, np.float64)
        self.xs = view(io.xs, (B, N + 1, nx), f, np.float64)
        self.us = view(io.us, (B, N, 7), f, np.float64)
        self.K = view(io.K, (B, N, 7, nx), f, np.float64)
        self.cost = view(io.cost, (B,), f, np.float64)
        self.iter = view(io.iters, (B,), i32, np.int32)
        self._ok = view(io.ok, (B,), u8, np.uint8)
        self.fn_pred = view(io.fn_pred, (B, 2), f, np.float64)
        self.stats = view(io.stats, (B, _abi.NSTATS), i32, np.int32)

    @property
    def ok(self) -> np.ndarray:
        return self._ok.astype(bool)

    def fill(self, batch, xs_init=None, us_init=None):
        """Copy a workload.Batch (and optional warm start) into the input views."""
        self.x0[...] = np.asarray(batch.x0, np.float64).reshape(self.x0.shape)
        self.node_ref[...] = np.asarray(batch.node_ref, np.float64).reshape(self.node_ref.shape)
        self.inst_ref[...] = np.asarray(batch.inst_ref, np.float64).reshape(self.inst_ref.shape)
        self.surface[...] = np.asarray(batch.surface, np.uint8).reshape(self.surface.shape)
        self.xs_init[...] = np.asarray(batch.xs_init if xs_init is None else xs_init, np.float64).reshape(
            self.xs_init.shape)
        self.us_init[...] = np.asarray(batch.us_init if us_init is None else us_init, np.float64).reshape(
            self.us_init.shape)

    def run(self) -> np.ndarray:
        if self._h is None:
            raise FfddpError("plan closed")
        if self.solver._h is None:
            raise FfddpError("the plan's solver is closed")
        self.solver._check(self._lib.ffddp_plan_run(self._h), "ffddp_plan_run")
        self.solver._run_callbacks(self.B)
        return self.ok

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ffddp_plan_destroy(self._h)
        self._h = None
        plans = getattr(getattr(self, "solver", None), "_plans", None)
        if plans is not None:
            plans.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
