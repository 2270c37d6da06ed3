"""The continuous model-comparison example runs end to end on the GPU, at a small size: every number of its table is finite
and the scores' invariants hold.  Which model wins is a statistical outcome and is not asserted."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_continuous_model_comparison_example():
    main = importlib.import_module("continuous_exponential_network_hawkes_model_comparison").main
    scores, table = main(duration=200.0, nnodes=4, nblocks=16, nsteps=60, burn=20, score_every=2)
    assert list(scores) == ["standard", "dense network", "Bernoulli network"]
    for name, (w, h) in scores.items():
        assert all(np.isfinite(v) for v in table[name].values()), (name, table[name])
        assert w.n == h.n == 20 and w.cells == 64 and h.cells == 16
        assert w.bins[0] == 0.0 and w.bins[-1] == 160.0 and h.bins[0] == 160.0 and h.bins[-1] == 200.0
        for s in (w, h):
            assert s.p_waic >= 0 and np.all(s.per_node[1] >= 0) and s.joint_lpd >= s.joint_mean and s.se_elpd >= 0
            assert s.waic == -2.0 * s.elpd_waic and s.elpd_waic <= s.lppd
            assert np.all(np.isfinite(s.pointwise)) and s.pointwise.shape == (len(s.edges) - 1, 4)
            for k, field in enumerate(("lppd", "p_waic", "elpd_waic")):
                assert abs(s.per_node[k].sum() - getattr(s, field)) <= 1e-12 * np.abs(s.per_node[k]).sum()
    assert table["standard"]["diff"] == 0.0 and table["standard"]["diff_se"] == 0.0
