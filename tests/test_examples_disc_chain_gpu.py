"""The discrete convergence-diagnostics example runs end to end on the GPU, at a small size."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_discrete_chain_diagnostics_example():
    main = importlib.import_module("discrete_gaussian_network_hawkes_diagnostics").main
    chain, z = main(duration=1500, nnodes=4, nbasis=2, nlags=4, nsteps=120, burn=20)
    d = chain.diagnostics
    assert d["n"] == 100 and d["batch_len"] == 10 and d["nbatches"] == 10
    assert list(d["summary"]) == ["baseline", "impulses.θ", "weights", "adjacency", "network.ρ"]
    for name, entries in (("baseline", 4), ("impulses.θ", 32), ("weights", 16), ("adjacency", 16), ("network.ρ", 1)):
        g = d["summary"][name]
        assert g["entries"] == entries and 0 <= g["undefined"] <= entries
        if g["undefined"] < entries:
            assert g["min_ess"] > 0 and 0 <= g["min_ess_index"] < entries and g["max_rhat"] > 0.9 and g["max_mcse"] >= 0
    assert d["summary"]["baseline"]["undefined"] == 0 and d["summary"]["network.ρ"]["undefined"] == 0
    assert len(chain.samples) == 1 and chain.mean.shape == z.shape == d["ess"].shape == chain.samples[0].shape
    assert np.isfinite(z).sum() >= 4 + 32 + 16 + 1              # every continuous parameter moved in both chains
