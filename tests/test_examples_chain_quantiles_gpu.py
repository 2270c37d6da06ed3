"""The credible-intervals example runs end to end on the GPU, at a small size."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_chain_quantiles_example():
    main = importlib.import_module("continuous_exponential_network_hawkes_intervals").main
    N = 6
    chain, found, links = main(duration=400.0, nnodes=N, nsteps=120, burn=20)
    q = chain.quantiles
    assert q.n == 100 and q.every == 1 and q.effective_weights and q.values.shape == (3, len(chain.mean))
    lower, upper = q.interval(0.95)
    state = slice(0, 1 + N + 2 * N * N)                       # ρ, λ0, W, θ; vec(A) has no quantiles
    assert np.all(np.isfinite(q.values[:, state])) and np.all(np.isnan(q.values[:, state.stop:]))
    assert np.all(q.min[state] <= lower[state]) and np.all(lower[state] <= q.values[1][state])
    assert np.all(q.values[1][state] <= upper[state]) and np.all(upper[state] <= q.max[state])
    assert found.shape == links.shape == (N, N) and found.dtype == bool
    # a link whose interval of A·W excludes zero was on in nearly every kept step: its 0.025 marker is off the spike, and the
    # marker's rank is within 0.1 of 0.025 at this length (twice the 0.045 measured at n = 200, tests/test_chain_quantiles_host.py)
    on = chain.mean[state.stop:].reshape((N, N), order="F")
    assert np.all(on[found] > 0.8)
