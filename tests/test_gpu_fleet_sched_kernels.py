"""GPU: the scheduled tick's two kernels (ffddp_fleet_pre_sched_dev,
ffddp_fleet_post_sched_dev) alone, on crafted state, against a numpy
restatement of include/ffddp.h's rules: which instances solve, the warm start
and the policy read through `age` from kept arrays that are never moved, what
is kept, the command filter, the counters.  Everything is exact except torque
entries that pass through a dot product, which get the bound of
tests/test_gpu_fleet_loop_kernels.py (64 * 2^-53 * S / d per entry); the
filter's clips and its smoothing are 1-Lipschitz in the target, so the bound
carries through it.  With period 1, no filter and age 0 both kernels give the
unscheduled entry points' bits."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_fleet_loop_kernels as KT  # noqa: E402  (the unscheduled restatement, the bound, the input makers)
from ffddp import BatchedBoxFDDP, _abi  # noqa: E402
from ffddp import robot as R  # noqa: E402
from ffddp.config import classical_preset, ff_preset  # noqa: E402
from helpers import rel_err  # noqa: E402

SENTINEL = KT.SENTINEL
# N = 5 / 4: the ages {0, 1, N-1, N+3} are all different and the last one saturates every index;
# B = 67 crosses a wave of instances; ff has nx = 21 (odd strides)
SHAPES = [("classical", 5, 16), ("ff", 4, 67)]


def _ages(N, B):
    return np.array([(0, 1, N - 1, N + 3)[b % 4] for b in range(B)], np.int32)


def _sched(period, apply_filter, dt=0.005) -> _abi.FleetSched:
    s = _abi.FleetSched()
    s.period, s.apply_filter, s.dt = period, int(apply_filter), dt
    s.tau_trust_inf, s.tau_smoothing_alpha = 0.9, 0.35
    s.tau_rate_limit[:] = [60.0, 60.0, 60.0, 60.0, 24.0, 24.0, 24.0]  # * dt = 0.3 / 0.12: inside the trust bound
    return s


def _counters(rng, N, B, period):
    """since on both sides of the period (since + 1 >= period decides), the four ages in turn."""
    since = rng.integers(0, period + 1, B).astype(np.int32)
    since[0], since[1] = max(period - 2, 0), period - 1
    return since, _ages(N, B)


def _full(*s, dtype=torch.float64, value=SENTINEL):
    return torch.full(s, value, dtype=dtype, device="cuda")


# -- numpy restatement ------------------------------------------------------------------
def _pre_sched_ref(st, P, sched, since, age, o, q_nom, node1, hint, variant, N, use_contact):
    """The unscheduled rules for the state, the surface and the references
    (KT._pre_ref; st is updated in place), then: need = !valid || since + 1 >=
    period; for need instances the warm start of the lists shifted `age` times;
    the other instances' xs_init / us_init rows are not written (sentinel)."""
    ref, ev = KT._pre_ref(st, P, o, q_nom, node1, hint, variant, N, use_contact)
    B, nx = ref["x0"].shape
    valid = st["valid"].astype(bool)
    need = (~valid) | (since + 1 >= sched.period)
    u_cold = o["tau_hat"] if variant == "ff" else st["tau_prev"]
    xs_init, us_init = np.full((B, N + 1, nx), SENTINEL), np.full((B, N, 7), SENTINEL)
    for b in np.flatnonzero(need):
        a = int(age[b])
        for k in range(N + 1):
            xs_init[b, k] = st["keep_xs"][b, min(k + a, N)] if (valid[b] and k >= 1) else ref["x0"][b]
        for k in range(N):
            us_init[b, k] = st["keep_us"][b, min(k + 1 + a, N - 1)] if valid[b] else u_cold[b]
    ref.update(xs_init=xs_init, us_init=us_init, need=need.astype(np.uint8))
    ev.update(need_invalid=need & ~valid, need_period=need & valid, rest=~need)
    return ref, ev


def _post_sched_ref(st, P, sched, since, age, need, d, x0, surface, tau_bias, variant, N):
    """fin = need && us[b][0] finite; a keep sets age = 0; the policy on knot
    min(age, N-1) of us / K, min(age, N) and min(age + 1, N) of xs (KT._post_ref on
    those knots); the filter; the counters.  st is updated in place."""
    B = x0.shape[0]
    need = need.astype(bool)
    fin = need & np.all(np.isfinite(d["us"][:, 0]), axis=1)
    for k, new in (("keep_xs", d["xs"]), ("keep_us", d["us"]), ("keep_K", d["K"])):
        st[k] = np.where(fin.reshape((-1,) + (1,) * (new.ndim - 1)), new, st[k])
    age1 = np.where(fin, 0, age)
    a = np.minimum(age1, N)
    ar = np.arange(B)
    ku, kx1 = np.minimum(a, N - 1), np.minimum(a + 1, N)
    # the unscheduled restatement on a two-knot view of the kept arrays, nothing left for it to keep
    view = dict(valid=(st["valid"].astype(bool) | fin).astype(np.uint8), tau_prev=st["tau_prev"].copy(),
                keep_xs=np.stack([st["keep_xs"][ar, a], st["keep_xs"][ar, kx1]], 1), keep_us=st["keep_us"][ar, ku][:, None],
                keep_K=st["keep_K"][ar, ku][:, None])
    nothing = dict(xs=np.zeros_like(view["keep_xs"]), us=np.full_like(view["keep_us"], np.nan),
                   K=np.zeros_like(view["keep_K"]), cost=d["cost"], fn_pred=d["fn_pred"])
    prev = st["tau_prev"].copy()
    r = KT._post_ref(view, P, nothing, x0, surface, tau_bias, variant, N)
    tau_cmd = r["tau_cmd"]
    if sched.apply_filter:  # _safe_tau's order and grouping
        lim = np.array(list(P.tau_limits))
        step = np.clip(tau_cmd - prev, -sched.tau_trust_inf, sched.tau_trust_inf)
        max_step = np.array(list(sched.tau_rate_limit)) * sched.dt
        step = np.clip(step, -max_step, max_step)
        al = sched.tau_smoothing_alpha
        tau_cmd = np.clip((1.0 - al) * prev + al * (prev + step), -lim, lim)
        r["filtered"] = np.abs(tau_cmd - r["tau_cmd"]) > 0
    st["valid"], st["tau_prev"] = view["valid"], tau_cmd.copy()
    r.update(fin=fin, tau_cmd=tau_cmd, tau_cmd_inf=KT._absmax(tau_cmd), since=np.where(need, 0, since + 1).astype(np.int32),
             age=np.where(need, age1, age1 + 1).astype(np.int32), neg_accepted=np.where(need, d["stats"][:, 9], 0))
    return r


@pytest.mark.parametrize("variant,N,B", SHAPES)
def test_pre_sched_matches_numpy(variant, N, B):
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N * 100 + B)
    seen = dict.fromkeys(("need_invalid", "need_period", "rest", "dropped", "warm_need"), False)
    for ci, (period, ps, hint) in enumerate([(1, 0, True), (2, 0, False), (3, 1, True), (3, 0, False)]):
        P = KT._params(phase_source=ps)
        sched = _sched(period, False)
        st = KT._state(rng, B, N, nx)
        st["valid"][:4], st["prev_mode"][:4] = 1, (1 if hint else 0)  # warm, no mode change: the period decides
        since, age = _counters(rng, N, B, period)
        o, od, _ = KT._observations(rng, B, strided=B > 16)
        q_nom = R.Q_NEUTRAL + rng.normal(0.0, 0.2, (B, 7))
        node1 = rng.normal(size=(N + 1, 6))
        t = KT._up(st)
        t.update(KT._up(dict(since=since, age=age, q_nom=q_nom, node_ref1=node1)))
        t.update({k: od[k] for k in ("q", "v", "fn_meas", "ee_z", "contact")})
        if variant == "ff":
            t["tau_hat"] = od["tau_hat"]
        t.update(x0=_full(B, nx), inst_ref=_full(B, 21), node_ref=_full(B, N + 1, 6), xs_init=_full(B, N + 1, nx),
                 us_init=_full(B, N, 7), surface=_full(B, dtype=torch.uint8, value=7),
                 need=_full(B, dtype=torch.uint8, value=7))
        st0 = {k: v.copy() for k, v in st.items()}
        solver.fleet_pre_dev(t, P, hint, stream=stream, sched=sched)
        ref, ev = _pre_sched_ref(st, P, sched, since, age, o, q_nom, node1, hint, variant, N, True)
        tag = (variant, N, B, ci)
        KT._assert_state(t, st, tag)
        got = KT._down(t, ("x0", "surface", "inst_ref", "node_ref", "xs_init", "us_init", "need", "since", "age"))
        for k in ("x0", "surface", "node_ref", "xs_init", "us_init", "need"):
            assert np.array_equal(got[k], ref[k], equal_nan=True), (tag, k)
        assert np.array_equal(got["since"], since) and np.array_equal(got["age"], age), tag  # post's to write
        assert np.array_equal(got["inst_ref"][:, :14], ref["xreg"]), tag
        assert rel_err(got["inst_ref"][:, 14:], _abi.gravity_torque(ref["gq"])) < 1e-12, tag
        for k in ("tau_prev", "keep_xs", "keep_us", "keep_K"):
            assert np.array_equal(st[k], st0[k]), (tag, k)
        if period == 1:
            assert ref["need"].all(), tag
        for k in ("need_invalid", "need_period", "rest", "dropped"):
            seen[k] |= bool(np.any(ev[k]))
        # a warm start read through every one of the four ages
        warm_need = ev["need_period"]
        seen["warm_need"] |= len(set(age[warm_need].tolist())) == 4
    assert all(seen.values()), seen
    solver.close()


@pytest.mark.parametrize("variant,N,B", SHAPES)
def test_post_sched_matches_numpy(variant, N, B):
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N * 100 + B + 7)
    seen = dict.fromkeys(("solved_kept", "solved_not_kept", "stale_finite_not_kept", "policy_aged", "not_valid",
                          "unstable", "filtered", "unfiltered", "bad_row"), False)
    cases = [(3, True, dict()), (3, False, dict()), (2, True, dict(use_feedback_policy=0))]
    if variant == "ff":
        cases.append((2, True, dict(ff_inverse_actuation_model=0, ff_dt_mpc_below_dt_ocp=0)))
    for ci, (period, apply_filter, kw) in enumerate(cases):
        P = KT._params(**kw)
        sched = _sched(period, apply_filter)
        d, st = KT._post_inputs(rng, variant, N, B, nx)  # its cases 0..7 on instances 0..7
        since, age = _counters(rng, N, B, period)
        need = (rng.random(B) < 0.5).astype(np.uint8)
        need[:8] = 1          # _post_inputs' cases are about this tick's solve ...
        need[4:6] = 0         # ... except two whose stale rows (cost above the limit, huge K) are then read or not
        need[8:12] = 0        # instances that do not solve, one per age, with a finite us[0] that must not be kept
        st["valid"][8:12] = 1
        assert np.all(np.isfinite(d["us"][8:12, 0]))
        o, od, rec = KT._observations(rng, B, strided=B > 16)
        x0 = rng.normal(size=(B, nx))
        surface = (rng.random(B) < 0.6).astype(np.uint8)
        surface[0], surface[2], surface[1] = 1, 1, 0
        scale = rng.uniform(0.8, 1.2, (B, 7))
        filt0 = rng.normal(size=(B, 7))
        t = KT._up(st)
        t.update(KT._up(d))
        t.update(KT._up(dict(x0=x0, surface=surface, since=since, age=age, need=need, scale=scale, tau_filt=filt0)))
        t.update(tau_bias=od["tau_bias"], obs=od["obs"], tau_cmd=_full(B, 7), info=_full(B, _abi.FLEET_INFO_W),
                 tau_app=_full(B, 7), log_obs=_full(B, _abi.FLEET_LOG_W))
        st0 = {k: v.copy() for k, v in st.items()}
        lpf = 0.2
        solver.fleet_post_dev(t, P, lpf=lpf, stream=stream, sched=sched)
        r = _post_sched_ref(st, P, sched, since, age, need, d, x0, surface, o["tau_bias"], variant, N)
        tag = (variant, N, B, ci)
        got = KT._down(t, ("tau_cmd", "info", "since", "age", "need", "tau_app", "tau_filt", "log_obs"))
        info = {k: got["info"][:, i] for i, k in enumerate(_abi.FLEET_INFO_FIELDS)}
        pol = r["valid_policy"] & ~r["unstable"] & ~r["bad"]
        tol = np.where(pol[:, None], KT.U64 * r["S"], 0.0)
        assert np.all(np.isfinite(tol)) and np.all(tol < 1e-9), tag
        fin_inf = np.isfinite(r["tau_raw_inf"])
        row_tol = np.where(r["valid_policy"] & fin_inf, KT.U64 * np.nan_to_num(r["S"]).max(1), 0.0)
        assert np.all(np.abs(r["tau_raw_inf"][fin_inf] - P.max_tau_raw_inf) > row_tol[fin_inf]), tag
        # exact: what is kept, the flags, the counters, the state
        KT._assert_state(t, st, tag, tau_prev_exact=False)
        assert np.array_equal(got["since"], r["since"]) and np.array_equal(got["age"], r["age"]), tag
        assert np.array_equal(got["need"], need), tag
        for k, ref in (("ok", d["ok"]), ("cost", d["cost"]), ("iters", d["iters"]), ("fin", r["fin"]),
                       ("unstable", r["unstable"]), ("surface", surface), ("policy_idx", r["policy_idx"]),
                       ("neg_accepted", r["neg_accepted"]), ("fn_pred", r["fn_pred"])):
            assert np.array_equal(info[k], np.asarray(ref, float), equal_nan=True), (tag, k)
        for b in range(8, 12):  # did not solve: the kept arrays are the old ones although us[0] is finite
            for k in ("keep_xs", "keep_us", "keep_K"):
                assert np.array_equal(st[k][b], st0[k][b]), (tag, k, b)
        # torques
        assert np.all(np.isfinite(got["tau_cmd"])), tag
        err = np.abs(got["tau_cmd"] - r["tau_cmd"])
        assert np.all(err <= tol), (tag, float(np.max(err - tol)))
        assert np.array_equal(got["tau_cmd"][~pol], r["tau_cmd"][~pol]), tag
        assert np.array_equal(t["tau_prev"].cpu().numpy(), got["tau_cmd"]), tag
        assert np.all(np.abs(info["tau_raw_inf"][fin_inf] - r["tau_raw_inf"][fin_inf]) <= row_tol[fin_inf]), tag
        assert np.array_equal(info["tau_cmd_inf"], np.max(np.abs(got["tau_cmd"]), 1)), tag
        app = got["tau_cmd"] * scale
        assert np.array_equal(got["tau_app"], app) and np.array_equal(got["tau_filt"], (1.0 - lpf) * filt0 + lpf * app), tag
        assert np.array_equal(got["log_obs"], rec[:, [28, 29, 30, 46, 47]], equal_nan=True), tag
        nb = need.astype(bool)
        seen["solved_kept"] |= bool(r["fin"].any())
        seen["solved_not_kept"] |= bool((nb & ~r["fin"]).any())
        seen["stale_finite_not_kept"] |= bool((~nb & np.all(np.isfinite(d["us"][:, 0]), 1)).any())
        seen["policy_aged"] |= len(set(age[~nb & pol].tolist())) == 4
        seen["not_valid"] |= bool((~r["valid_policy"]).any())
        seen["unstable"] |= bool(r["unstable"].any())
        seen["bad_row"] |= bool(r["bad"].any())
        if apply_filter:
            seen["filtered"] |= bool(r["filtered"].any())
        else:
            seen["unfiltered"] = True
    assert all(seen.values()), seen
    solver.close()


@pytest.mark.parametrize("variant,N,B", SHAPES)
def test_period_one_no_filter_equals_unscheduled_kernels(variant, N, B):
    cfg = classical_preset(N) if variant == "classical" else ff_preset(N)
    nx = cfg.nx
    solver = BatchedBoxFDDP(cfg, max_batch=B, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(N * 100 + B + 13)
    P = KT._params()
    sched = _sched(1, False)
    d, st = KT._post_inputs(rng, variant, N, B, nx)
    o, od, _ = KT._observations(rng, B, strided=True)
    q_nom = R.Q_NEUTRAL + rng.normal(0.0, 0.2, (B, 7))
    node1 = rng.normal(size=(N + 1, 6))
    outs = []
    for use_sched in (False, True):
        t = KT._up(st)
        t.update(KT._up(d))
        t.update(KT._up(dict(q_nom=q_nom, node_ref1=node1, since=np.zeros(B, np.int32), age=np.zeros(B, np.int32),
                             scale=np.full((B, 7), 0.9), tau_filt=np.zeros((B, 7)))))
        t.update({k: od[k] for k in ("q", "v", "fn_meas", "ee_z", "contact", "tau_bias", "obs")})
        if variant == "ff":
            t["tau_hat"] = od["tau_hat"]
        t.update(x0=_full(B, nx), inst_ref=_full(B, 21), node_ref=_full(B, N + 1, 6), xs_init=_full(B, N + 1, nx),
                 us_init=_full(B, N, 7), surface=_full(B, dtype=torch.uint8, value=7),
                 need=_full(B, dtype=torch.uint8, value=7), tau_cmd=_full(B, 7), info=_full(B, _abi.FLEET_INFO_W),
                 tau_app=_full(B, 7), log_obs=_full(B, _abi.FLEET_LOG_W))
        kw = dict(sched=sched) if use_sched else {}
        solver.fleet_pre_dev(t, P, True, stream=stream, **kw)
        solver.fleet_post_dev(t, P, lpf=0.2, stream=stream, **kw)
        outs.append(KT._down(t, KT.STATE_KEYS + ("x0", "surface", "inst_ref", "node_ref", "xs_init", "us_init", "tau_cmd",
                                                 "info", "tau_app", "tau_filt", "log_obs", "need", "since", "age")))
    plain, sch = outs
    for k in plain:
        if k not in ("need", "since", "age"):
            assert np.array_equal(plain[k], sch[k], equal_nan=True), k
    assert np.all(sch["need"] == 1) and np.all(sch["since"] == 0)
    fin = sch["info"][:, _abi.FLEET_INFO_FIELDS.index("fin")] != 0
    assert np.array_equal(sch["age"], np.zeros(B, np.int32)) and fin.any() and not fin.all()
    solver.close()


def test_sched_error_codes():
    N, B = 2, 3
    solver = BatchedBoxFDDP(classical_preset(N), max_batch=B, device=0)
    lib, h = solver._lib, solver._h
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    p = C.c_void_p(int(buf.data_ptr()))
    P, S = KT._params(), _abi.FleetState()
    for k, _ in _abi.FleetState._fields_:
        setattr(S, k, int(buf.data_ptr()))

    def sched(**kw):
        q = _sched(2, True)
        q.since = q.age = q.need = int(buf.data_ptr())
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def pre(B_, q):
        return lib.ffddp_fleet_pre_sched_dev(h, B_, C.byref(P), C.byref(S), *([p] * 5), 7, 1, p, 7, p, p, 1, *([p] * 6), q, None)

    def post(B_, q):
        return lib.ffddp_fleet_post_sched_dev(h, B_, C.byref(P), C.byref(S), *([p] * 8), p, p, p, 7, p, p, None, None,
                                              None, 0.2, None, 0, None, q, None)

    assert pre(B + 1, sched()) == -4 and post(B + 1, sched()) == -4  # FFDDP_E_CAPACITY
    assert pre(0, sched()) == -1 and post(0, sched()) == -1          # FFDDP_E_INVALID
    for bad in (dict(period=0), dict(since=0), dict(age=0), dict(need=0), dict(tau_smoothing_alpha=1.5)):
        assert pre(B, sched(**bad)) == -1 and post(B, sched(**bad)) == -1, bad
    torch.cuda.synchronize()
    solver.close()
