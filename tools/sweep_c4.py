#!/usr/bin/env python3
"""BASELINE configs[3]: all 5 scenarios x 256 seeds = 1280 closed-loop runs,
sharded over the ranks (one process per GPU, torchrun), each rank stepping its
shard as one fleet (FleetClassicalMPC, or FleetForceFeedbackMPC with
--variant ff, + BatchedPlant); RCCL all-gather of the
per-instance summaries; rank 0 prints one JSON line (per-scenario statistics,
wall time, closed-loop ticks/s).

  python tools/sweep_c4.py [--seeds 256] [--time 4]            # 1 GPU
  python tools/sweep_c4.py --variant ff                        # force-feedback fleet
  python tools/sweep_c4.py --device-tick 1                     # classical, tick glue in HIP kernels
  python tools/sweep_c4.py --device-loop 1 --device-noise numpy   # the whole closed loop on the device, the
                                                               # injector's normals from a pre-drawn table
  python tools/sweep_c4.py --device-loop 1 --device-noise philox  # ... or generated on the device
  python tools/sweep_c4.py --device-loop 1 --solve-period 2     # solve every 2nd tick, the feedback policy between
  python tools/sweep_c4.py --command-filter 1                   # _safe_tau's trust / rate / smoothing filter
  python tools/sweep_c4.py --device-loop 1 --device-refs 1      # references sampled on the device from task records
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --task-spread 0.3 0.3   # radius and speed vary per instance
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --solve-period 4 --stagger 4   # start delays (b mod 4) dt
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --device-summary 1 --keep-logs 0   # the summary's sums on the
                                                               # device, no per-tick logs: any --time in constant memory
  python tools/sweep_c4.py --device-loop 1 --device-noise philox --plant-spread 0.5 0.5 --uncertainty-spread 0.5 3
                                                               # table stiffness, joint damping, noise levels and
                                                               # delays vary per instance (host path too)
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --force-spread 8 36 --force-ramp 0.5
                                                               # a force setpoint per instance, ramped in after touchdown
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --weight-spread w_fn 7 112 --weight-spread w_tau 2e-4 3.2e-3
                                                               # the controller's cost weights per instance, log-uniform
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --limit-spread 0.25 1
                                                               # the torque limits per instance, scaled log-uniformly
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --payload-spread 0 3
                                                               # a payload (kg) in each controller's model, uniform
  python tools/sweep_c4.py --device-loop 1 --device-refs 1 --device-noise philox --tilt-known 1
                                                               # the controllers are told the table's tilt
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 tools/sweep_c4.py
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import ffddp_path  # noqa: E402,F401


ALL_SCENARIOS = ("flat", "tilted_5", "tilted_10", "tilted_15", "actuation_uncertainty")


def weight_spread_arg(items):
    """--weight-spread NAME LO HI, repeatable -> run_sweep's {name: (lo, hi)} (None without the option)."""
    if not items:
        return None
    out = {}
    for name, lo, hi in items:
        if name in out:
            raise ValueError(f"--weight-spread: {name} given twice")
        out[name] = (float(lo), float(hi))
    return out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--time", type=float, default=4.0)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--neg-step-rule", type=int, choices=(0, 1), default=0,
                    help="ascent-direction comparator: 0 Crocoddyl's (default), 1 bounded rise")
    ap.add_argument("--variant", choices=("classical", "ff"), default="classical",
                    help="controller: classical (default) or force feedback")
    ap.add_argument("--device-tick", type=int, choices=(0, 1), default=0,
                    help="classical only: 1 runs the tick's glue through the library's fleet kernels "
                         "(the ff fleet always does)")
    ap.add_argument("--device-loop", type=int, choices=(0, 1), default=0,
                    help="1 runs the whole closed loop on the device (DeviceFleetLoop); scenarios with an "
                         "uncertainty injector (actuation_uncertainty) need --device-noise")
    ap.add_argument("--device-noise", choices=("numpy", "philox"), default=None,
                    help="with --device-loop 1: run the uncertainty injector on the device, its normals from a "
                         "table drawn ahead with numpy (the host loop's perturbations) or from Philox on the device")
    ap.add_argument("--solve-period", type=int, default=1,
                    help="mpc_update_steps: solve every P-th tick, the feedback policy on the receding plan between")
    ap.add_argument("--command-filter", type=int, choices=(0, 1), default=0,
                    help="1: apply_command_filter (trust region, rate limit, smoothing of the command)")
    ap.add_argument("--device-refs", type=int, choices=(0, 1), default=0,
                    help="with --device-loop 1: sample every instance's references on the device from its task record")
    ap.add_argument("--task-spread", type=float, nargs=2, default=None, metavar=("DR", "DW"),
                    help="with --device-refs 1: per-instance radius 0.10 (1 + DR u1) and omega 1.5 (1 + DW u2), u in [-1, 1]")
    ap.add_argument("--stagger", type=int, default=0,
                    help="with --device-refs 1: instance b starts its task (b mod S) ticks late")
    ap.add_argument("--device-summary", type=int, choices=(0, 1), default=0,
                    help="with --device-loop 1: accumulate the summary's sums on the device, one more launch per tick")
    ap.add_argument("--keep-logs", type=int, choices=(0, 1), default=1,
                    help="with --device-summary 1: 0 keeps no per-tick logs (memory no longer grows with --time)")
    ap.add_argument("--plant-spread", type=float, nargs=2, default=None, metavar=("DS", "DD"),
                    help="per-instance plant physics: contact time constant 0.02 (1 + DS u0), joint damping "
                         "1.0 (1 + DD u1), u in [-1, 1]; each spread in [0, 0.9]")
    ap.add_argument("--uncertainty-spread", type=float, nargs=2, default=None, metavar=("DN", "D"),
                    help="per-instance injector profile: sigmas scaled by 1 + DN u, u in [-1, 1], DN in [0, 1); "
                         "observation and command delay each 0..D ticks, D an integer 0..16")
    ap.add_argument("--force-spread", type=float, nargs=2, default=None, metavar=("F_LO", "F_HI"),
                    help="with --device-loop 1: per-instance force setpoint F_LO + (F_HI - F_LO) (1 + u) / 2, u in [-1, 1]")
    ap.add_argument("--force-ramp", type=float, default=None, metavar="T",
                    help="with --force-spread: the reference ramps from F_LO to the setpoint over T seconds from the end "
                         "of the contact hold (0: the setpoint from the start)")
    ap.add_argument("--weight-spread", nargs=3, action="append", default=None, metavar=("NAME", "LO", "HI"),
                    help="with --device-loop 1, repeatable: cost weight NAME (w_fn, w_tangent_pos, w_tau, ...) per "
                         "instance, log-uniform in [LO, HI]")
    ap.add_argument("--limit-spread", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="with --device-loop 1: per-instance torque limits, the configuration's scaled log-uniformly "
                         "in [LO, HI]")
    ap.add_argument("--payload-spread", type=float, nargs=2, default=None, metavar=("M_LO", "M_HI"),
                    help="with --device-loop 1: per-instance controller models, the nominal arm with a point payload "
                         "of M_LO..M_HI kg (uniform) at the EE offset; the plant is unchanged")
    ap.add_argument("--plant-payload-spread", type=float, nargs=2, default=None, metavar=("M_LO", "M_HI"),
                    help="per-instance plants: the arm carries a point payload of M_LO..M_HI kg (uniform) at the EE "
                         "offset; the controllers plan with the nominal model unless --payload-known 1")
    ap.add_argument("--payload-known", type=int, choices=(0, 1), default=0,
                    help="with --plant-payload-spread and --device-loop 1: 1 gives each controller its plant's model")
    ap.add_argument("--tilt-known", type=int, choices=(0, 1), default=0,
                    help="with --device-loop 1: 1 tells each controller its table's tilt (it plans in the table's "
                         "frame, and is scored there); the plant is unchanged")
    ap.add_argument("--scenarios", nargs="+", default=list(ALL_SCENARIOS), help="scenarios to sweep (default: all 5)")
    return ap


def main():
    ap = build_parser()
    a = ap.parse_args()
    try:
        wspread = weight_spread_arg(a.weight_spread)
    except ValueError as e:
        ap.error(str(e))
    import torch
    import torch.distributed as dist
    from ffddp import fleet, shard

    uspread = None
    if a.uncertainty_spread is not None:
        if a.uncertainty_spread[1] != int(a.uncertainty_spread[1]):
            ap.error("--uncertainty-spread: D is an integer number of ticks")
        uspread = (a.uncertainty_spread[0], int(a.uncertainty_spread[1]))
    rank, world, local = shard.env_ranks()
    shard.init("nccl", local, world)
    torch.cuda.set_device(local)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    res = fleet.run_sweep(scenarios=tuple(a.scenarios), seeds=a.seeds, total_time=a.time, rank=rank, world=world,
                           device=local, verbose=(rank == 0), neg_step_rule=a.neg_step_rule, variant=a.variant, device_tick=bool(a.device_tick),
                           device_loop=bool(a.device_loop), device_noise=a.device_noise,
                           solve_period=a.solve_period, command_filter=bool(a.command_filter),
                           device_refs=bool(a.device_refs), task_spread=a.task_spread, stagger=a.stagger,
                           device_summary=bool(a.device_summary), keep_logs=bool(a.keep_logs),
                           plant_spread=a.plant_spread, uncertainty_spread=uspread,
                           force_spread=a.force_spread, force_ramp=a.force_ramp, weight_spread=wspread,
                           limit_spread=a.limit_spread, payload_spread=a.payload_spread,
                           plant_payload_spread=a.plant_payload_spread, payload_known=bool(a.payload_known),
                           tilt_known=bool(a.tilt_known))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    m = fleet.gather_summaries(res, res["n_all"], device=torch.device("cuda", local))
    names, _, _, _ = fleet._sweep_instances(tuple(a.scenarios), a.seeds)
    if rank == 0:
        line = {"config": "%d scenarios x %d seeds closed loop, %.1f s each" % (len(a.scenarios), a.seeds, a.time),
                "ranks": world, "device_loop": int(a.device_loop), "device_noise": a.device_noise, "loop_wall_s": res["wall_s"],
                "neg_step_rule": a.neg_step_rule, "variant": a.variant,
                "device_tick": int(a.device_tick or a.variant == "ff"),
                "solve_period": a.solve_period, "command_filter": int(a.command_filter),
                "rank0_solve_share": float(res["solved_ticks"].sum() / max(1, res["ticks"] * res["instances"])),
                "instances": int(res["n_all"]), "ticks": res["ticks"], "wall_s": wall,
                "closed_loop_ticks_per_s": res["n_all"] * res["ticks"] / wall,
                "rank0_controller_s": res["controller_s"], "scenarios": fleet.scenario_table(names, m)}
        line.update(device_refs=int(a.device_refs), task_spread=a.task_spread, stagger=a.stagger,
                    loop_ms_per_tick=1.0e3 * res["wall_s"] / max(1, res["ticks"]))
        line.update(device_summary=int(a.device_summary), keep_logs=int(a.keep_logs),
                    wall_ms_per_tick=1.0e3 * wall / max(1, res["ticks"]), rank0_device_memory=dict(fleet.DEVICE_MEMORY) or None)
        # the mismatch axes as run (this rank's shard): the ranges of the contact time constant, the joint damping,
        # the injectors' delays and torque-noise level, and the instances lost to a failed plant step
        rows, dly, sig = res["plant_rows"], res["inject_delay"], res["inject_sigma"]
        inj = dly[:, 0] >= 0
        line.update(plant_spread=a.plant_spread, uncertainty_spread=a.uncertainty_spread,
                    rank0_timeconst_range=[float(rows[:, 16].min()), float(rows[:, 16].max())],
                    rank0_damping_range=[float(rows[:, 7].min()), float(rows[:, 7].max())],
                    rank0_inject_delay_max=[int(x) for x in dly[inj].max(0)] if inj.any() else None,
                    rank0_sigma_tau_range=[float(sig[inj, 2].min()), float(sig[inj, 2].max())] if inj.any() else None,
                    rank0_plant_fail_instances=int(np.count_nonzero(res.get("plant_fail", 0))))
        if "force_rec" in res:  # this rank's shard by setpoint: measured contact-phase force and force error
            f1 = res["force_rec"][:, 1]
            pi = res["per_instance"]
            edges = np.linspace(a.force_spread[0], a.force_spread[1], 5)
            which = np.clip(np.digitize(f1, edges) - 1, 0, 3)
            line.update(force_spread=a.force_spread, force_ramp=a.force_ramp, rank0_force_bins=[
                {"setpoint_lo": float(edges[i]), "setpoint_hi": float(edges[i + 1]), "instances": int(np.sum(which == i)),
                 "setpoint_mean": float(np.mean(f1[which == i])),
                 "fn_mean_contact_phase": float(np.nanmean(pi["fn_mean_contact_phase"][which == i])),
                 "avg_abs_force_err": float(np.nanmean(pi["avg_abs_force_err"][which == i])),
                 "contact_loss_contact_phase_pct": float(np.nanmean(pi["contact_loss_contact_phase_pct"][which == i]))}
                for i in range(4) if np.any(which == i)])
        if "weights" in res:  # this rank's shard by each swept weight, four log-spaced bins
            pi = res["per_instance"]
            line["weight_spread"] = wspread
            line["rank0_weight_bins"] = {}
            for name, w in res["weights"].items():
                edges = np.geomspace(wspread[name][0], wspread[name][1], 5)
                which = np.clip(np.digitize(w, edges) - 1, 0, 3)
                line["rank0_weight_bins"][name] = [
                    {"weight_lo": float(edges[i]), "weight_hi": float(edges[i + 1]), "instances": int(np.sum(which == i)),
                     "weight_mean": float(np.mean(w[which == i])),
                     "fn_mean_contact_phase": float(np.nanmean(pi["fn_mean_contact_phase"][which == i])),
                     "avg_abs_force_err": float(np.nanmean(pi["avg_abs_force_err"][which == i])),
                     "rms_tangential_error_contact_phase":
                         float(np.nanmean(pi["rms_tangential_error_contact_phase"][which == i])),
                     "contact_loss_contact_phase_pct": float(np.nanmean(pi["contact_loss_contact_phase_pct"][which == i]))}
                    for i in range(4) if np.any(which == i)]
        if "limit_scale" in res:  # this rank's shard by torque-limit scale, four log-spaced bins
            pi, sc = res["per_instance"], res["limit_scale"]
            edges = np.geomspace(a.limit_spread[0], a.limit_spread[1], 5)
            which = np.clip(np.digitize(sc, edges) - 1, 0, 3)
            line.update(limit_spread=a.limit_spread, rank0_limit_bins=[
                {"scale_lo": float(edges[i]), "scale_hi": float(edges[i + 1]), "instances": int(np.sum(which == i)),
                 "scale_mean": float(np.mean(sc[which == i])),
                 "fn_mean_contact_phase": float(np.nanmean(pi["fn_mean_contact_phase"][which == i])),
                 "avg_abs_force_err": float(np.nanmean(pi["avg_abs_force_err"][which == i])),
                 "rms_tangential_error_contact_phase":
                     float(np.nanmean(pi["rms_tangential_error_contact_phase"][which == i])),
                 "contact_loss_contact_phase_pct": float(np.nanmean(pi["contact_loss_contact_phase_pct"][which == i]))}
                for i in range(4) if np.any(which == i)])
        if "payload_mass" in res:  # this rank's shard by the controller model's payload mass, four linear bins
            pi, pm = res["per_instance"], res["payload_mass"]
            edges = np.linspace(a.payload_spread[0], a.payload_spread[1], 5)
            which = np.clip(np.digitize(pm, edges) - 1, 0, 3)
            line.update(payload_spread=a.payload_spread, rank0_payload_bins=[
                {"mass_lo": float(edges[i]), "mass_hi": float(edges[i + 1]), "instances": int(np.sum(which == i)),
                 "mass_mean": float(np.mean(pm[which == i])),
                 "fn_mean_contact_phase": float(np.nanmean(pi["fn_mean_contact_phase"][which == i])),
                 "avg_abs_force_err": float(np.nanmean(pi["avg_abs_force_err"][which == i])),
                 "rms_tangential_error_contact_phase":
                     float(np.nanmean(pi["rms_tangential_error_contact_phase"][which == i])),
                 "contact_loss_contact_phase_pct": float(np.nanmean(pi["contact_loss_contact_phase_pct"][which == i]))}
                for i in range(4) if np.any(which == i)])
        if "plant_payload_mass" in res:  # this rank's shard by the plant's payload mass, four linear bins
            pi, pm = res["per_instance"], res["plant_payload_mass"]
            edges = np.linspace(a.plant_payload_spread[0], a.plant_payload_spread[1], 5)
            which = np.clip(np.digitize(pm, edges) - 1, 0, 3)
            line.update(plant_payload_spread=a.plant_payload_spread, payload_known=int(a.payload_known),
                        rank0_plant_payload_bins=[
                {"mass_lo": float(edges[i]), "mass_hi": float(edges[i + 1]), "instances": int(np.sum(which == i)),
                 "mass_mean": float(np.mean(pm[which == i])),
                 "fn_mean_contact_phase": float(np.nanmean(pi["fn_mean_contact_phase"][which == i])),
                 "avg_abs_force_err": float(np.nanmean(pi["avg_abs_force_err"][which == i])),
                 "rms_tangential_error_contact_phase":
                     float(np.nanmean(pi["rms_tangential_error_contact_phase"][which == i])),
                 "contact_loss_contact_phase_pct": float(np.nanmean(pi["contact_loss_contact_phase_pct"][which == i]))}
                for i in range(4) if np.any(which == i)])
        line["tilt_known"] = int(bool(res.get("tilt_known", False)))
        # instances that left the nominal regime, per scenario: any tick on the unstable fallback; a non-finite summary
        ui, ri = fleet.SUMMARY_KEYS.index("unstable_ticks"), fleet.SUMMARY_KEYS.index("rms_3d_error")
        line["diverged"] = {str(s): {"unstable_instances": int(np.sum(m[names == s, ui] > 0)),
                                     "nonfinite_instances": int(np.sum(~np.isfinite(m[names == s, ri])))}
                            for s in dict.fromkeys(names)}
        if "solved" in res:  # the share of instances that solve per tick, once every instance has switched to contact
            surf, share = res["surface"], res["solved"].mean(1)
            k0 = int(np.max(np.argmax(surf, 0))) + 1 if surf.any(0).all() else len(share)
            if k0 < len(share):
                line.update(rank0_share_after_switch_mean=float(share[k0:].mean()),
                            rank0_share_after_switch_max=float(share[k0:].max()), rank0_last_switch_tick=k0 - 1)
        print(json.dumps(line), flush=True)
        if a.out:
            Path(a.out).write_text(json.dumps(line, indent=1))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
