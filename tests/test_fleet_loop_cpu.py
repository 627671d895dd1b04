"""The device fleet loop's host side (no device here): the new structs' ctypes
layouts against the header, the entry points' null-handle codes, run_sweep's
refusals, and the loop's reference table against the fleets' _node_ref."""
import ctypes
import subprocess
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from ffddp import _abi
from ffddp import controller as CT
from ffddp import fleet as FL
from ffddp import robot as R
from ffddp.trajectory import benchmark_traj

ROOT = Path(__file__).resolve().parents[1]


def test_fleet_struct_layouts_match_header():
    fp = [n for n, _ in _abi.FleetParams._fields_]
    fs = [n for n, _ in _abi.FleetState._fields_]
    offs = "".join(f'  printf("%zu ", offsetof(ffddp_fleet_params, {n}));\n' for n in fp)
    offs += "".join(f'  printf("%zu ", offsetof(ffddp_fleet_state, {n}));\n' for n in fs)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ffddp.h"\nint main(void) {\n'
           '  printf("%zu %zu %d %d ", sizeof(ffddp_fleet_params), sizeof(ffddp_fleet_state), FFDDP_FLEET_INFO_W,\n'
           '         FFDDP_FLEET_LOG_W);\n' + offs + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(src)
        exe = Path(d) / "t"
        subprocess.run(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(exe)], check=True)
        vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[:4] == [ctypes.sizeof(_abi.FleetParams), ctypes.sizeof(_abi.FleetState), _abi.FLEET_INFO_W,
                        _abi.FLEET_LOG_W]
    assert len(_abi.FLEET_INFO_FIELDS) == _abi.FLEET_INFO_W
    want = [getattr(_abi.FleetParams, n).offset for n in fp] + [getattr(_abi.FleetState, n).offset for n in fs]
    assert vals[4:] == want
    # the header's field order is the binding's
    hdr = (ROOT / "include" / "ffddp.h").read_text()
    body = hdr.split("typedef struct ffddp_fleet_state {")[1].split("} ffddp_fleet_state;")[0]
    assert [ln.split(";")[0].split("*")[-1].strip() for ln in body.strip().splitlines()] == fs


def test_fleet_loop_null_handle_errors():
    lib = _abi.load()
    p, s = _abi.FleetParams(), _abi.FleetState()
    pre = lib.ffddp_fleet_pre_dev(None, 1, ctypes.byref(p), ctypes.byref(s), *([None] * 5), 7, 1, None, 7, None, None, 0,
                                  *([None] * 6), None)
    post = lib.ffddp_fleet_post_dev(None, 1, ctypes.byref(p), ctypes.byref(s), *([None] * 8), None, None, None, 7,
                                    None, None, None, None, None, 0.2, None, 0, None, None)
    assert pre == -1 and post == -1  # FFDDP_E_INVALID


def test_run_sweep_device_loop_refusals():
    """Both are refused before any device object is made, so this runs without a device."""
    with pytest.raises(NotImplementedError, match="injector"):
        FL.run_sweep(scenarios=("actuation_uncertainty",), seeds=1, total_time=0.1, verbose=False, device_loop=True)
    with pytest.raises(NotImplementedError, match="injector"):
        FL.run_sweep(scenarios=("flat", "actuation_uncertainty"), seeds=1, total_time=0.1, verbose=False,
                     variant="ff", device_loop=True)
    with pytest.raises(NotImplementedError, match="record"):
        FL.run_sweep(scenarios=("flat",), seeds=1, total_time=0.1, verbose=False, record=(0,), device_loop=True)


@pytest.mark.parametrize("vectorised", [True, False])
def test_reference_table_matches_fleet_node_ref(vectorised):
    from ffddp.fleet_loop import reference_table

    traj, meta = benchmark_traj(np.array([-0.4, 0.05, 0.55]))
    if not vectorised:  # a plain Python traj_fn takes _node_ref's scalar path
        base = traj
        traj = lambda t: base(t)  # noqa: E731
    N, dt_ocp, dt, steps, t0 = 6, 0.01, 0.005, 30, 0.7
    p_off = np.array([0.01, -0.02, 0.03])
    refs, hints, times = reference_table(traj, steps, dt, N, dt_ocp, R.R_MJ_FROM_PIN, p_off, t0=t0)
    assert refs.shape == (steps, N + 1, 6) and hints.shape == (steps,) and hints.dtype == bool
    fleet = SimpleNamespace(traj_fn=traj, N=N, dt_ocp=dt_ocp, R_mj_from_pin=R.R_MJ_FROM_PIN.copy(),
                            p_site_minus_frame_pin=p_off)
    t = t0
    for k in range(steps):
        assert times[k] == t
        assert np.array_equal(refs[k], FL._FleetBase._node_ref(fleet, t)), k
        assert hints[k] == bool(traj(t)[2])
        t += dt
    assert hints.any() and not hints.all()  # the window crosses the contact onset


def test_fleet_params_from_config():
    from ffddp.fleet_loop import fleet_params

    cfg = CT.ff_benchmark_config(0.005, 0.342, phase_source="force_latch")
    p = fleet_params(cfg, "ff", 0.01)
    assert (p.phase_source, p.posture_mode, p.torque_mode, p.contact_release_steps) == (1, 1, 0, 80)
    assert p.ff_dt_mpc_below_dt_ocp == 1 and p.eps_pol == 0.5 and p.ff_inverse_actuation_model == 1
    assert p.alpha_ocp == CT.ff_filter_alpha(cfg, 0.01) and p.alpha_ctrl == CT.ff_filter_alpha(cfg, 0.005)
    assert list(p.tau_limits) == list(np.asarray(cfg.tau_limits, float))
    c = CT.classical_benchmark_config(0.005, 0.342)
    c.posture_ref_mode, c.torque_ref_mode = "x0", "zero"
    p = fleet_params(c, "classical", 0.01)
    assert (p.phase_source, p.posture_mode, p.torque_mode, p.contact_release_steps) == (0, 0, 2, 60)
    assert p.feedback_gain_scale == 0.55 and p.max_tau_raw_inf == 300.0
