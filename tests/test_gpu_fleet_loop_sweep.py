"""GPU: run_sweep(device_loop=True): the summary has the host path's keys and
shapes, finite values, the right counts, and a second run gives the same."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from ffddp import fleet as FL  # noqa: E402

KW = dict(scenarios=("flat", "tilted_10"), seeds=2, total_time=0.2, verbose=False)


@pytest.mark.parametrize("variant", ["classical", "ff"])
def test_device_loop_sweep_summary(variant):
    host = FL.run_sweep(variant=variant, **KW)
    a = FL.run_sweep(variant=variant, device_loop=True, **KW)
    b = FL.run_sweep(variant=variant, device_loop=True, **KW)
    assert set(a) == set(host) and set(a["per_instance"]) == set(host["per_instance"]) == set(FL.SUMMARY_KEYS)
    assert a["ticks"] == host["ticks"] == 40 and a["instances"] == host["instances"] == 4
    assert a["shard"] == host["shard"] and a["n_all"] == host["n_all"] == 4 and a["variant"] == variant
    assert list(a["names"]) == list(host["names"]) and np.array_equal(a["seed"], host["seed"])
    assert a["wall_s"] > 0.0 and a["controller_s"] is None
    # 0.2 s ends before the contact phase (t >= 0.8 s), so the three statistics over that phase are
    # NaN by definition (runlog.summary_metrics on an empty phase), on either path; all others are finite
    undefined = {"rms_tangential_error_contact_phase", "contact_loss_contact_phase_pct", "fn_mean_contact_phase"}
    for k in FL.SUMMARY_KEYS:
        va, vh = a["per_instance"][k], host["per_instance"][k]
        assert va.shape == vh.shape == (4,) and va.dtype == vh.dtype, k
        if k in undefined:
            assert np.all(np.isnan(va)) and np.all(np.isnan(vh)), (k, va)
        else:
            assert np.all(np.isfinite(va)), (k, va)
        assert np.array_equal(va, b["per_instance"][k], equal_nan=True), k
    # the same loops up to the policy's rounding: 40 ticks in, the tracking errors are still close
    assert np.allclose(a["per_instance"]["rms_3d_error"], host["per_instance"]["rms_3d_error"], rtol=1e-3)
    m = FL.gather_summaries(a, a["n_all"])
    assert m.shape == (4, len(FL.SUMMARY_KEYS))
