"""GPU: the device fleet loop's two kernels (ffddp_fleet_pre_dev,
ffddp_fleet_post_dev) alone, on synthetic arrays, against a numpy restatement
of the fleets' rules (ffddp/fleet.py: _phase, _surface, compute_control,
_command).  Exact except the gravity torque (1e-12 relative, the project's
tolerance for the device gravity torque) and torque entries that pass through
a dot product: per entry at most 64 * 2^-53 * S / d, S the sum of the absolute
values of all terms that enter the entry, d = max(1e-6, 1 - alpha_ctrl) with
the inverse actuation map and 1 otherwise (two summation orders of n <= 24
products differ by at most 2 gamma_n sum|terms| ~ 48 u; 64 leaves room for
fused multiply-adds)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp.config import classical_preset, ff_preset  # noqa: E402
from helpers import rel_err  # noqa: E402

SENTINEL = -777.25
U64 = 64.0 * 2.0 ** -53
# as tests/test_gpu_fleet_tick.py: N = 2 hits the min(k+1, N-1) clamp at once, B = 65 crosses a wave of
# instances, ff has nx = 21 (odd strides) and B = 130 is more than two waves of instances
SHAPES = [("classical", 2, 3), ("classical", 5, 65), ("ff", 3, 130)]
OBS_W = _abi.PLANT_OBS


def _params(**kw) -> _abi.FleetParams:
    p = _abi.FleetParams()
    vals = dict(phase_source=1, contact_release_steps=2, posture_mode=1, torque_mode=0, use_feedback_policy=1,
                ff_use_tau_interpolation=1, ff_inverse_actuation_model=1, ff_dt_mpc_below_dt_ocp=1, z_contact=0.34,
                z_contact_band=0.012, fn_contact_on=1.0, fn_contact_off=0.1, feedback_gain_scale=0.55,
                max_solver_cost=1.0e8, max_tau_raw_inf=30.0, fallback_dq_damping=2.0, eps_pol=0.5, alpha_ocp=0.2,
                alpha_ctrl=0.45)
    vals.update(kw)
    lim = vals.pop("tau_limits", np.full(7, 0.8))
    for k, v in vals.items():
        setattr(p, k, v)
    _abi._fill(p.tau_limits, lim)
    return p


def _state(rng, B, N, nx):
    f = lambda *s: rng.normal(size=s)  # noqa: E731
    return dict(valid=(rng.random(B) < 0.6).astype(np.uint8), latched=(rng.random(B) < 0.5).astype(np.uint8),
                loss_count=rng.integers(0, 3, B).astype(np.int32), prev_mode=rng.integers(-1, 2, B).astype(np.int8),
                tau_prev=f(B, 7), keep_xs=f(B, N + 1, nx), keep_us=f(B, N, 7), keep_K=f(B, N, 7, nx))


def _observations(rng, B, strided):
    """The controllers' inputs; strided: views of (B, PLANT_OBS) records laid out as the plant's."""
    rec = rng.normal(size=(B, OBS_W))
    rec[:, 0:7] = R.Q_NEUTRAL + rng.normal(0.0, 0.3, (B, 7))
    rec[:, 46] = rng.uniform(0.0, 2.0, B)                 # around fn_contact_off / _on
    rec[:, 47] = (rng.random(B) < 0.7).astype(float)
    rec[:, 30] = 0.34 + rng.uniform(-0.03, 0.03, B)       # around z_contact + band
    rec[B // 2, 30] = np.nan
    tau_hat = rng.normal(size=(B, 7))
    cols = dict(q=slice(0, 7), v=slice(7, 14), tau_bias=slice(14, 21), fn_meas=46, contact=47, ee_z=30)
    host = {k: rec[:, c] for k, c in cols.items()}
    host["tau_hat"] = tau_hat
    rec_d = torch.from_numpy(rec).cuda()
    if strided:
        dev = {k: rec_d[:, c] for k, c in cols.items()}
        assert dev["q"].stride(0) == OBS_W and dev["fn_meas"].stride(0) == OBS_W
    else:
        dev = {k: rec_d[:, c].contiguous() for k, c in cols.items()}
        assert dev["q"].stride(0) == 7 and dev["fn_meas"].stride(0) == 1
    dev["tau_hat"] = torch.from_numpy(tau_hat).cuda()
    dev["obs"] = rec_d
    return host, dev, rec


# -- numpy restatement ------------------------------------------------------------------
def _surface_ref(st, P, fn, ee_z, hint):
    """_FleetBase._surface; updates st["latched"], st["loss_count"]."""
    B = fn.shape[0]
    if P.phase_source != 1:
        return np.full(B, bool(hint)), {}
    latched = st["latched"].astype(bool)
    near = np.isfinite(ee_z) & (ee_z <= P.z_contact + P.z_contact_band)
    lost = fn < P.fn_contact_off
    cnt = np.where(latched, np.where(lost, st["loss_count"] + 1, 0), 0)
    release = latched & (cnt >= P.contact_release_steps)
    by_force = (~latched) & (fn > P.fn_contact_on)
    by_hint = (~latched) & ~(fn > P.fn_contact_on) & (bool(hint) & near)
    engage = by_force | by_hint
    st["latched"] = ((latched & ~release) | engage).astype(np.uint8)
    st["loss_count"] = np.where(release | engage, 0, cnt).astype(np.int32)
    ev = dict(by_force=by_force, by_hint=by_hint, release=release, counting=(cnt > 0) & ~release,
              nan_not_near=~np.isfinite(ee_z) & ~latched & bool(hint) & ~(fn > P.fn_contact_on))
    return st["latched"].astype(bool), ev


def _pre_ref(st, P, o, q_nom, node1, hint, variant, N, use_contact):
    """_phase + the references + _shift_guess; st is updated in place."""
    B = q_nom.shape[0]
    fn = o["fn_meas"] * (o["contact"] > 0.5) if use_contact else o["fn_meas"]
    surf, ev = _surface_ref(st, P, fn, o["ee_z"], hint)
    changed = (st["prev_mode"] >= 0) & (surf != (st["prev_mode"] == 1))
    ev["dropped"] = changed & st["valid"].astype(bool)
    st["valid"] = (st["valid"].astype(bool) & ~changed).astype(np.uint8)
    st["prev_mode"] = surf.astype(np.int8)
    x0 = np.concatenate([o["q"], o["v"]] + ([o["tau_hat"]] if variant == "ff" else []), 1)
    nx = x0.shape[1]
    xreg = np.concatenate([q_nom, np.zeros((B, 7))], 1) if P.posture_mode == 1 else x0[:, :14].copy()
    gq = None if P.torque_mode == 2 else (q_nom if P.torque_mode == 1 else o["q"])
    u_cold = o["tau_hat"] if variant == "ff" else st["tau_prev"]
    xs_init, us_init = np.zeros((B, N + 1, nx)), np.zeros((B, N, 7))
    for b in range(B):
        for k in range(N + 1):
            xs_init[b, k] = st["keep_xs"][b, k] if (st["valid"][b] and k >= 1) else x0[b]
        for k in range(N):
            us_init[b, k] = st["keep_us"][b, min(k + 1, N - 1)] if st["valid"][b] else u_cold[b]
    return dict(x0=x0, surface=surf.astype(np.uint8), xreg=xreg, gq=gq, node_ref=np.broadcast_to(node1, (B,) + node1.shape),
                xs_init=xs_init, us_init=us_init), ev


def _absmax(a):
    with np.errstate(invalid="ignore"):
        return np.max(np.abs(a), 1)


def _post_ref(st, P, d, x0, surface, tau_bias, variant, N):
    """keep, the policy and _command as the fleets do them; st updated in place.
    Also S (B, 7): the sum of |terms| entering each policy entry of tau_raw
    (already divided by d) and S_des for tau_des."""
    fin = np.all(np.isfinite(d["us"][:, 0]), axis=1)
    for k, new in (("keep_xs", d["xs"]), ("keep_us", d["us"]), ("keep_K", d["K"])):
        st[k] = np.where(fin.reshape((-1,) + (1,) * (new.ndim - 1)), new, st[k])
    valid = st["valid"].astype(bool) | fin
    xs0, xs1, us0, K0 = st["keep_xs"][:, 0], st["keep_xs"][:, 1], st["keep_us"][:, 0], st["keep_K"][:, 0]
    v, s, B = x0[:, 7:14], P.feedback_gain_scale, x0.shape[0]
    surf = surface.astype(bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if variant == "classical":
            tau_raw = np.where(valid[:, None], us0, st["tau_prev"])
            S = np.abs(us0)
            if P.use_feedback_policy:
                dx = x0 - xs0
                fb = s * np.matmul(K0, dx[:, :, None])[:, :, 0]
                tau_raw = np.where(valid[:, None], tau_raw + fb, tau_raw)
                S = S + s * np.abs(K0 * dx[:, None, :]).sum(2)
            tau_des_inf, S_des = np.full(B, np.nan), S
            fn_pred = np.where(surf, d["fn_pred"][:, 0], np.nan)
        else:
            tau_hat = x0[:, 14:21]
            eps = P.eps_pol if P.ff_use_tau_interpolation else 0.0
            tau0, tau1 = xs0[:, 14:21], xs1[:, 14:21]
            tau_pol = tau0 + eps * (tau1 - tau0)
            S = np.abs(tau0) + np.abs(eps * (tau1 - tau0))
            if P.use_feedback_policy:
                Kx, Ktau = K0[:, :, :14], K0[:, :, 14:21]
                x_err, tau_err = xs0[:, :14] - x0[:, :14], tau0 - tau_hat
                I7 = np.eye(7)
                Ktx = eps * (1.0 - P.alpha_ocp) * Kx
                Ktt = I7 + eps * (1.0 - P.alpha_ocp) * (Ktau - I7)
                tau_pol = tau_pol + s * (np.matmul(Ktx, x_err[:, :, None])[:, :, 0]
                                         + np.matmul(Ktt, tau_err[:, :, None])[:, :, 0])
                S = S + s * (np.abs(Ktx * x_err[:, None, :]).sum(2) + np.abs(Ktt * tau_err[:, None, :]).sum(2))
            tau_des = np.where(valid[:, None], tau_pol, tau_hat)
            tau_raw, S_des = tau_des.copy(), S
            if P.ff_inverse_actuation_model:
                dd = max(1.0e-6, 1.0 - P.alpha_ctrl)
                tau_raw = (tau_raw - P.alpha_ctrl * tau_hat) / dd
                S = (S + np.abs(P.alpha_ctrl * tau_hat)) / dd
            tau_des_inf = _absmax(tau_des)
            f0, f1 = np.abs(d["fn_pred"][:, 0]), np.abs(d["fn_pred"][:, 1])
            f01 = f0 if (N == 1 or not P.ff_dt_mpc_below_dt_ocp) else (1.0 - P.eps_pol) * f0 + P.eps_pol * f1
            fn_next = f0 if N == 1 else np.where(~np.isfinite(f0), f1, np.where(~np.isfinite(f1), f0, f01))
            fn_pred = np.where(surf & np.isfinite(fn_next), fn_next, np.nan)
        policy_idx = np.where(valid, 0, -1)
        # _command
        cost = d["cost"]
        tau_raw_inf = _absmax(tau_raw)
        by_cost = (~np.isfinite(cost)) | (cost > P.max_solver_cost)
        by_tau = tau_raw_inf > P.max_tau_raw_inf
        unstable = by_cost | by_tau
        fallback = tau_bias - P.fallback_dq_damping * v
        tau_sel = np.where(unstable[:, None], fallback, tau_raw)
        st["valid"] = (valid & ~unstable).astype(np.uint8)
        lim = np.array(list(P.tau_limits))
        bad = ~np.all(np.isfinite(tau_sel), 1)
        unclipped = np.where(bad[:, None], st["tau_prev"], tau_sel)
        tau_cmd = np.clip(unclipped, -lim, lim)
        st["tau_prev"] = tau_cmd.copy()
    return dict(fin=fin, valid_policy=valid, tau_raw_inf=tau_raw_inf, tau_des_inf=tau_des_inf, unstable=unstable,
                by_cost=by_cost, by_tau=by_tau, bad=bad, tau_cmd=tau_cmd, unclipped=unclipped, policy_idx=policy_idx,
                fn_pred=fn_pred, S=S, S_des=S_des, tau_cmd_inf=_absmax(tau_cmd))


def _solve_outputs(rng, B, N, nx):
    f = lambda *s: rng.normal(size=s)  # noqa: E731
    d = dict(xs=f(B, N + 1, nx), us=f(B, N, 7), K=0.3 * f(B, N, 7, nx), cost=np.abs(f(B)) * 10.0,
             iters=rng.integers(0, 20, B).astype(np.int32), ok=(rng.random(B) < 0.7).astype(np.uint8),
             fn_pred=f(B, 2), stats=rng.integers(0, 3, (B, _abi.NSTATS)).astype(np.int32))
    return d


def _up(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _down(t, keys):
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in keys}


STATE_KEYS = ("valid", "latched", "loss_count", "prev_mode", "tau_prev", "keep_xs", "keep_us", "keep_K")


def _assert_state(t, st, tag, tau_prev_exact=True):
    got = _down(t, STATE_KEYS)
    for k in STATE_KEYS:
        if k == "tau_prev" and not tau_prev_exact:
            continue
        assert got[k].dtype == st[k].dtype, (tag, k)
        assert np.array_equal(got[k], st[k], equal_nan=True), (tag, k)


@pytest.mark.parametrize("variant,N,B", SHAPES)
def test_fleet_pre_matches_numpy(variant, N, B):
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N * 1000 + B)
    strided = B > 3  # the smallest shape takes dense arrays, the others views of plant records
    seen = {k: False for k in ("warm", "cold", "dropped", "by_force", "by_hint", "release", "counting", "nan_not_near")}
    # every reference mode, both phase sources, both hints, the force with and without the contact flag
    cases = [(ps, pm, tm, hint, uc) for ps in (0, 1) for pm in (0, 1) for tm in (0, 1, 2)
             for hint, uc in ((True, True), (False, False))]
    for ci, (ps, pm, tm, hint, use_contact) in enumerate(cases):
        P = _params(phase_source=ps, posture_mode=pm, torque_mode=tm)
        st = _state(rng, B, N, nx)
        o, od, _ = _observations(rng, B, strided)
        q_nom = R.Q_NEUTRAL + rng.normal(0.0, 0.2, (B, 7))
        node1 = rng.normal(size=(N + 1, 6))
        t = _up(st)
        t.update({k: od[k] for k in ("q", "v", "fn_meas", "ee_z")})
        if use_contact:
            t["contact"] = od["contact"]
        if variant == "ff":
            t["tau_hat"] = od["tau_hat"]
        t.update(_up(dict(q_nom=q_nom, node_ref1=node1)))
        full = lambda *s, dtype=torch.float64: torch.full(s, SENTINEL, dtype=dtype, device="cuda")  # noqa: E731
        t.update(x0=full(B, nx), inst_ref=full(B, 21), node_ref=full(B, N + 1, 6), xs_init=full(B, N + 1, nx),
                 us_init=full(B, N, 7), surface=torch.full((B,), 7, dtype=torch.uint8, device="cuda"))
        st0 = {k: v.copy() for k, v in st.items()}
        solver.fleet_pre_dev(t, P, hint, stream=stream)
        ref, ev = _pre_ref(st, P, o, q_nom, node1, hint, variant, N, use_contact)
        tag = (variant, N, B, ci)
        _assert_state(t, st, tag)
        got = _down(t, ("x0", "surface", "inst_ref", "node_ref", "xs_init", "us_init"))
        for k in ("x0", "surface", "node_ref", "xs_init", "us_init"):
            assert np.array_equal(got[k], ref[k], equal_nan=True), (tag, k)
        assert np.array_equal(got["inst_ref"][:, :14], ref["xreg"]), tag
        if ref["gq"] is None:
            assert np.all(got["inst_ref"][:, 14:] == 0.0), tag
        else:
            assert rel_err(got["inst_ref"][:, 14:], _abi.gravity_torque(ref["gq"])) < 1e-12, tag
        # the kept solution and the previous command are inputs here
        for k in ("tau_prev", "keep_xs", "keep_us", "keep_K"):
            assert np.array_equal(st[k], st0[k]), (tag, k)
        seen["warm"] |= bool(st["valid"].any())
        seen["cold"] |= bool((st["valid"] == 0).any())
        for k, m in ev.items():
            seen[k] |= bool(np.any(m))
    assert all(seen.values()), seen
    solver.close()


def test_fleet_pre_latch_sequence():
    """contact_release_steps = 2 over a sequence of calls: engaging by force,
    engaging by hint and nearness, counting losses, releasing, a NaN ee_z."""
    N, B = 2, 6
    solver = BatchedBoxFDDP(classical_preset(N), max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)
    P = _params(phase_source=1, contact_release_steps=2)
    st = _state(rng, B, N, 14)
    st["valid"][:], st["latched"][:], st["loss_count"][:], st["prev_mode"][:] = 1, 0, 0, -1
    near, far = 0.34, 0.40
    # per call: hint, fn (B,), ee_z (B,)
    #   0: force on, then two losses -> released;  1: hint + near;  2: hint but NaN ee_z;  3: hint but far;
    #   4: force on, one loss, recovers (count back to 0);  5: force on and kept
    seq = [(False, [2.0, 0.5, 0.5, 0.5, 2.0, 2.0], [near, near, np.nan, far, far, far]),
           (True, [0.05, 0.5, 0.5, 0.5, 0.05, 2.0], [near, near, np.nan, far, far, far]),
           (True, [0.05, 0.5, 0.5, 0.5, 0.50, 2.0], [far, far, np.nan, far, far, far]),
           (True, [0.05, 0.05, 0.5, 0.5, 0.05, 2.0], [far, far, np.nan, far, far, far]),
           (False, [0.05, 0.05, 2.0, 0.5, 0.05, 2.0], [far, far, np.nan, far, far, far])]
    t = _up(st)
    q_nom = np.tile(R.Q_NEUTRAL, (B, 1))
    node1 = rng.normal(size=(N + 1, 6))
    t.update(_up(dict(q_nom=q_nom, node_ref1=node1, q=q_nom + 0.1, v=rng.normal(size=(B, 7)))))
    t.update(x0=torch.zeros((B, 14), dtype=torch.float64, device="cuda"),
             inst_ref=torch.zeros((B, 21), dtype=torch.float64, device="cuda"),
             node_ref=torch.zeros((B, N + 1, 6), dtype=torch.float64, device="cuda"),
             xs_init=torch.zeros((B, N + 1, 14), dtype=torch.float64, device="cuda"),
             us_init=torch.zeros((B, N, 7), dtype=torch.float64, device="cuda"),
             surface=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    o = dict(q=q_nom + 0.1, v=t["v"].cpu().numpy())
    trace, events = [], {}
    for call, (hint, fn, ee_z) in enumerate(seq):
        o["fn_meas"], o["ee_z"] = np.array(fn), np.array(ee_z)
        t.update(_up(dict(fn_meas=o["fn_meas"], ee_z=o["ee_z"])))
        solver.fleet_pre_dev(t, P, hint, stream=stream)
        ref, ev = _pre_ref(st, P, o, q_nom, node1, hint, "classical", N, False)
        _assert_state(t, st, call)
        got = _down(t, ("surface", "xs_init"))
        assert np.array_equal(got["surface"], ref["surface"]) and np.array_equal(got["xs_init"], ref["xs_init"]), call
        trace.append(st["latched"].copy())
        for k, m in ev.items():
            events.setdefault(k, []).append(m.copy())
        # the kept solution survives only where the mode did not change; re-arm it for the next call
        st["valid"][:] = 1
        t["valid"].fill_(1)
    trace = np.array(trace)
    assert trace[:, 0].tolist() == [1, 1, 0, 0, 0]                         # engaged by force, released after 2 losses
    assert events["by_force"][0][0] and events["release"][2][0] and events["counting"][1][0]
    assert trace[:, 1].tolist() == [0, 1, 1, 1, 0] and events["by_hint"][1][1]  # engaged by hint and nearness
    assert trace[:, 2].tolist() == [0, 0, 0, 0, 1] and events["nan_not_near"][1][2]  # a NaN ee_z is not near
    assert trace[:, 3].tolist() == [0, 0, 0, 0, 0]                         # far: the hint alone does not engage
    assert trace[:, 4].tolist() == [1, 1, 1, 1, 0] and events["counting"][1][4]  # one loss, recovered, then released
    assert trace[:, 5].tolist() == [1, 1, 1, 1, 1]
    assert any(e.any() for e in events["dropped"])
    solver.close()


def _post_inputs(rng, variant, N, B, nx, shift=0):
    """One batch with every branch of the post kernel (asserted by the caller).
    Case j goes to instance j - shift; B = 3 holds three cases per launch and
    sees the others through `shift` in its later launches."""
    d = _solve_outputs(rng, B, N, nx)
    st = _state(rng, B, N, nx)
    st["keep_K"] *= 0.3

    def case(j, b):
        st["valid"][b] = 0 if j == 1 else 1
        if j == 0:    # not kept; valid before: the policy reads the kept arrays
            d["us"][b, 0, 3], d["fn_pred"][b, 0] = np.nan, np.nan
        elif j == 1:  # not kept and not valid: commands tau_prev / tau_hat
            d["us"][b, 0, 6] = np.inf
        elif j == 2:  # only knot 0 is tested: kept
            d["us"][b, 1, 2], d["fn_pred"][b, 1] = np.nan, np.nan
        elif j == 3:  # unstable by cost
            d["cost"][b] = np.nan
        elif j == 4:  # above max_solver_cost
            d["cost"][b] = 2.0e8
        elif j == 5:  # tau_raw_inf above its limit
            d["K"][b, 0] *= 3.0e3
        elif j == 6:  # a non-finite tau_raw row -> tau_prev
            d["K"][b, 0, 2, 5 if variant == "classical" else 16] = np.nan
        elif j == 7:
            d["fn_pred"][b] = np.nan

    for j in range(8):
        if 0 <= j - shift < B:
            case(j, j - shift)
    return d, st


@pytest.mark.parametrize("variant,N,B", SHAPES)
def test_fleet_post_matches_numpy(variant, N, B):
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N * 1000 + B + 7)
    strided = B > 3
    seen = dict.fromkeys(("valid", "not_valid", "not_fin", "kept_nan_knot1", "cost_nan", "cost_high", "tau_high", "bad",
                          "clipped", "not_clipped", "fn_nan0", "fn_nan1", "surface", "free"), False)
    param_sets = [dict(), dict(use_feedback_policy=0)]
    if variant == "ff":
        param_sets += [dict(ff_use_tau_interpolation=0), dict(ff_inverse_actuation_model=0, ff_dt_mpc_below_dt_ocp=0)]
    launch = 0
    for ci, kw in enumerate(param_sets):
        for with_sweep_args in (True, False):
            P = _params(**kw)
            d, st = _post_inputs(rng, variant, N, B, nx, shift=0 if B >= 8 else (0, 5, 3)[launch % 3])
            launch += 1
            o, od, rec = _observations(rng, B, strided)
            x0 = rng.normal(size=(B, nx))
            surface = (rng.random(B) < 0.6).astype(np.uint8)
            surface[0], surface[2], surface[1] = 1, 1, 0
            scale = rng.uniform(0.8, 1.2, (B, 7))
            filt0 = rng.normal(size=(B, 7))
            t = _up(st)
            t.update(_up(d))
            t.update(_up(dict(x0=x0, surface=surface)))
            t["tau_bias"] = od["tau_bias"]
            t["tau_cmd"] = torch.full((B, 7), SENTINEL, dtype=torch.float64, device="cuda")
            t["info"] = torch.full((B, _abi.FLEET_INFO_W), SENTINEL, dtype=torch.float64, device="cuda")
            lpf = 0.2
            if with_sweep_args:
                t.update(_up(dict(scale=scale, tau_filt=filt0)))
                t["tau_app"] = torch.full((B, 7), SENTINEL, dtype=torch.float64, device="cuda")
                t["log_obs"] = torch.full((B, _abi.FLEET_LOG_W), SENTINEL, dtype=torch.float64, device="cuda")
                t["obs"] = od["obs"]
            valid0 = st["valid"].astype(bool).copy()
            solver.fleet_post_dev(t, P, lpf=lpf, stream=stream)
            r = _post_ref(st, P, d, x0, surface, o["tau_bias"], variant, N)
            tag = (variant, N, B, ci, with_sweep_args)
            got = _down(t, ("tau_cmd", "info"))
            info = {k: got["info"][:, i] for i, k in enumerate(_abi.FLEET_INFO_FIELDS)}
            # per-entry bound for what passed through a dot product; everything else is exact
            pol = r["valid_policy"] & ~r["unstable"] & ~r["bad"]
            tol = np.where(pol[:, None], U64 * r["S"], 0.0)
            assert np.all(np.isfinite(tol)) and np.all(tol < 1e-9), tag
            # the threshold flag: every instance is further from max_tau_raw_inf than its bound, none excluded
            row_tol = np.where(r["valid_policy"] & np.isfinite(r["tau_raw_inf"]), U64 * np.nan_to_num(r["S"]).max(1), 0.0)
            fin_inf = np.isfinite(r["tau_raw_inf"])
            assert np.all(np.abs(r["tau_raw_inf"][fin_inf] - P.max_tau_raw_inf) > row_tol[fin_inf]), tag
            # exact: keep, flags, integer fields, the state
            _assert_state(t, st, tag, tau_prev_exact=False)
            for k, ref in (("ok", d["ok"]), ("cost", d["cost"]), ("iters", d["iters"]), ("fin", r["fin"]),
                           ("unstable", r["unstable"]), ("surface", surface), ("policy_idx", r["policy_idx"]),
                           ("neg_accepted", d["stats"][:, 9]), ("fn_pred", r["fn_pred"])):
                assert np.array_equal(info[k], np.asarray(ref, float), equal_nan=True), (tag, k)
            # torques
            assert np.all(np.isfinite(got["tau_cmd"])), tag
            err = np.abs(got["tau_cmd"] - r["tau_cmd"])
            assert np.all(err <= tol), (tag, float(np.max(err - tol)))
            assert np.array_equal(got["tau_cmd"][~pol], r["tau_cmd"][~pol]), tag
            tp = t["tau_prev"].cpu().numpy()
            assert np.array_equal(tp, got["tau_cmd"]), tag  # tau_prev = tau_cmd
            assert np.array_equal(np.isnan(info["tau_raw_inf"]), np.isnan(r["tau_raw_inf"])), tag
            assert np.all(np.abs(info["tau_raw_inf"][fin_inf] - r["tau_raw_inf"][fin_inf]) <= row_tol[fin_inf]), tag
            assert np.array_equal(info["tau_cmd_inf"], np.max(np.abs(got["tau_cmd"]), 1)), tag
            assert np.all(np.abs(info["tau_cmd_inf"] - r["tau_cmd_inf"]) <= tol.max(1)), tag
            if variant == "ff":
                des_tol = np.where(r["valid_policy"], U64 * np.nan_to_num(r["S_des"]).max(1), 0.0)
                fd = np.isfinite(r["tau_des_inf"])
                assert np.array_equal(np.isnan(info["tau_des_inf"]), ~fd), tag
                assert np.all(np.abs(info["tau_des_inf"][fd] - r["tau_des_inf"][fd]) <= des_tol[fd]), tag
            else:
                assert np.all(np.isnan(info["tau_des_inf"])), tag
            if with_sweep_args:
                g2 = _down(t, ("tau_app", "tau_filt", "log_obs"))
                app = got["tau_cmd"] * scale
                assert np.array_equal(g2["tau_app"], app), tag
                assert np.array_equal(g2["tau_filt"], (1.0 - lpf) * filt0 + lpf * app), tag
                assert np.array_equal(g2["log_obs"], rec[:, [28, 29, 30, 46, 47]], equal_nan=True), tag
            # the solution the kernel read is untouched
            assert np.array_equal(t["K"].cpu().numpy(), d["K"], equal_nan=True), tag
            lim = np.array(list(P.tau_limits))
            clipped = np.abs(r["unclipped"]) > lim
            seen["valid"] |= bool(valid0.any())
            seen["not_valid"] |= bool((~r["valid_policy"]).any())
            seen["not_fin"] |= bool((~r["fin"]).any())
            seen["kept_nan_knot1"] |= bool((r["fin"] & np.isnan(st["keep_us"][:, 1]).any(1)).any())
            seen["cost_nan"] |= bool(np.isnan(d["cost"]).any())
            seen["cost_high"] |= bool((d["cost"] > P.max_solver_cost).any())
            seen["tau_high"] |= bool((r["by_tau"] & ~r["by_cost"]).any())
            seen["bad"] |= bool(r["bad"].any())
            seen["clipped"] |= bool(clipped.any())
            seen["not_clipped"] |= bool((~clipped).any())
            seen["fn_nan0"] |= bool((np.isnan(d["fn_pred"][:, 0]) & ~np.isnan(d["fn_pred"][:, 1]) & (surface != 0)).any())
            seen["fn_nan1"] |= bool((np.isnan(d["fn_pred"][:, 1]) & ~np.isnan(d["fn_pred"][:, 0]) & (surface != 0)).any())
            seen["surface"] |= bool(surface.any())
            seen["free"] |= bool((surface == 0).any())
    assert all(seen.values()), seen
    solver.close()


def test_fleet_loop_kernel_error_codes():
    N, B = 2, 3
    solver = BatchedBoxFDDP(classical_preset(N), max_batch=B, device=0)
    lib, h = solver._lib, solver._h
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    p = C.c_void_p(int(buf.data_ptr()))
    P = _params()
    S = _abi.FleetState()
    for k, _ in _abi.FleetState._fields_:
        setattr(S, k, int(buf.data_ptr()))

    def pre(B_, ptrs, P_=P, S_=S, h_=h):
        a = list(ptrs)  # q v fn contact ee_z | tau_hat | q_nom node1 | x0 surface inst_ref node_ref xs_init us_init
        return lib.ffddp_fleet_pre_dev(h_, B_, C.byref(P_) if P_ is not None else None, C.byref(S_) if S_ is not None else None,
                                       *a[0:5], 7, 1, a[5], 7, a[6], a[7], 1, *a[8:14], None)

    def post(B_, ptrs, P_=P, S_=S, h_=h):
        a = list(ptrs)  # xs..stats (8) | x0 surface tau_bias | tau_cmd info | scale tau_app tau_filt | obs log_obs
        return lib.ffddp_fleet_post_dev(h_, B_, C.byref(P_) if P_ is not None else None, C.byref(S_) if S_ is not None else None,
                                        *a[0:8], a[8], a[9], a[10], 7, a[11], a[12], a[13], a[14], a[15], 0.2, a[16],
                                        _abi.PLANT_OBS, a[17], None)

    assert pre(B + 1, [p] * 14) == -4 and post(B + 1, [p] * 18) == -4  # FFDDP_E_CAPACITY
    assert pre(0, [p] * 14) == -1 and post(-1, [p] * 18) == -1  # FFDDP_E_INVALID
    assert pre(B, [p] * 14, h_=None) == -1 and post(B, [p] * 18, h_=None) == -1
    assert pre(B, [p] * 14, P_=None) == -1 and post(B, [p] * 18, S_=None) == -1
    optional_pre, optional_post = {3, 5}, {13, 14, 15, 16, 17}  # contact, tau_hat (classical) | the sweep's arguments
    for i in range(14):
        if i not in optional_pre:
            assert pre(B, [p] * i + [None] + [p] * (13 - i)) == -1, i
    for i in range(18):
        if i not in optional_post:
            assert post(B, [p] * i + [None] + [p] * (17 - i)) == -1, i
    for k, _ in _abi.FleetState._fields_:  # a null state array
        S2 = _abi.FleetState()
        for k2, _ in _abi.FleetState._fields_:
            setattr(S2, k2, 0 if k2 == k else int(buf.data_ptr()))
        assert pre(B, [p] * 14, S_=S2) == -1 and post(B, [p] * 18, S_=S2) == -1, k
    assert post(B, [p] * 14 + [None, p, p, p]) == -1  # tau_filt without tau_app
    assert post(B, [p] * 16 + [None, p]) == -1         # log_obs without obs
    # force feedback requires tau_hat
    sff = BatchedBoxFDDP(ff_preset(N), max_batch=B, device=0)
    assert pre(B, [p] * 5 + [None] + [p] * 8, h_=sff._h) == -1
    torch.cuda.synchronize()
    sff.close()
    solver.close()
