"""The latent-distance-network variational example runs end to end on the GPU and separates the planted links."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_the_example_runs():
    """The planted design is tests/clatvb_ref.py's RECOVERY with the package's simulator's events.  On these events the restatement
    (tests/clatvb_ref.py's run, 200 steps, on the CPU) gives mean ρv 0.978 on the planted links, 0.010 on the absent ones and a
    correlation of 0.958 of the network's own link probabilities with the planted ones; the bars are those with room for the
    stopping rule: 0.8, 0.2 and 0.7.  The trace never falls."""
    A, P, res = importlib.import_module("continuous_exponential_latent_distance_network_hawkes_vb").main()
    assert np.all(np.isfinite(res.trace)) and np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo))
    rho = res.link_probability()
    assert rho[A == 1.0].mean() > 0.8 and rho[A == 0.0].mean() < 0.2
    assert np.corrcoef(res.network_link_probability().ravel(), P.ravel())[0, 1] > 0.7
