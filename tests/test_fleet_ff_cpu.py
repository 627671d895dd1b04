"""CPU: the torque measurement the batched uncertainty injector exposes for
the force-feedback fleet (tau_hat, tau_hat_filt) against per-instance
ScenarioUncertaintyInjector outputs (tau_meas_act, tau_meas_act_filt)."""
from __future__ import annotations

import numpy as np

from ffddp import plant as PL
from ffddp import uncertainty as U


def _obs(q, dq):
    z7 = np.zeros(7)
    return PL.Observation(q=q.copy(), dq=dq.copy(), tau_meas=z7, tau_meas_filt=z7, tau_meas_act=z7,
                          tau_meas_act_filt=z7, tau_cmd=z7, tau_act=z7, tau_constraint=z7, tau_total=z7, tau_bias=z7,
                          f_contact_world=np.zeros(3), f_contact_normal=0.0, f_contact_normal_world_z=0.0,
                          f_contact_tangent=0.0, contact_count_ee=0, contact_count_table=0,
                          table_normal_world=np.array([0.0, 0.0, 1.0]), ee_pos=np.zeros(3),
                          ee_quat=np.array([1.0, 0.0, 0.0, 0.0]), J_pos=None, J_rot=None, ee_vel=np.zeros(3))


def test_batched_injector_torque_measurement_matches_scalar():
    """300 ticks (across the 256-tick pre-draw chunk), 4 seeds, the sweep's
    control period; a filter constant other than the default, so that a
    dropped tau_lpf_alpha would show."""
    seeds = [15, 1500003, 7, 42]
    dt, alpha = 0.005, 0.3
    cfgs = [U.config_for_scenario("actuation_uncertainty", seed=s) for s in seeds]
    bat = U.BatchedUncertaintyInjector(dt=dt, nu=7, configs=cfgs, tau_lpf_alpha=alpha)
    sc = [U.ScenarioUncertaintyInjector(dt=dt, nu=7, config=c, tau_lpf_alpha=alpha) for c in cfgs]
    assert bat.tau_hat.shape == (4, 7) and np.all(bat.tau_hat_filt == 0.0)
    rng = np.random.default_rng(3)
    for k in range(300):
        q, dq, tau = rng.normal(size=(4, 7)), rng.normal(size=(4, 7)), rng.normal(size=(4, 7)) * 10
        qb, dqb = bat.observation_for_controller(q, dq)  # the return value stays (q, dq)
        th, thf = bat.tau_hat.copy(), bat.tau_hat_filt.copy()
        ab = bat.command_for_plant(tau)
        for b, j in enumerate(sc):
            d = j.observation_for_controller(_obs(q[b], dq[b]))
            assert np.array_equal(qb[b], d.q) and np.array_equal(dqb[b], d.dq), (k, b)
            assert np.array_equal(th[b], d.tau_meas_act), (k, b)
            assert np.array_equal(thf[b], d.tau_meas_act_filt), (k, b)
            assert np.array_equal(ab[b], j.command_for_plant(tau[b])), (k, b)


def test_default_filter_constant_is_the_scalar_one():
    cfg = U.config_for_scenario("actuation_uncertainty", seed=5)
    bat = U.BatchedUncertaintyInjector(dt=0.005, nu=7, configs=[cfg])
    sc = U.ScenarioUncertaintyInjector(dt=0.005, nu=7, config=cfg)
    for k in range(3):
        bat.observation_for_controller(np.zeros((1, 7)), np.zeros((1, 7)))
        d = sc.observation_for_controller(_obs(np.zeros(7), np.zeros(7)))
        bat.command_for_plant(np.full((1, 7), 3.0))
        sc.command_for_plant(np.full(7, 3.0))
        assert np.array_equal(bat.tau_hat_filt[0], d.tau_meas_act_filt), k
