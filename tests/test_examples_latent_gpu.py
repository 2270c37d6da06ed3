"""The latent-distance-network example runs end to end on the GPU and prints a finite result."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_latent_distance_network_example(capsys):
    truth, P_true, P, chain = importlib.import_module("continuous_exponential_latent_distance_network_hawkes").main()
    printed = capsys.readouterr().out
    assert "posterior mean link probability" in printed and "nan" not in printed
    assert chain.n == 200 and chain.exhausted == 0
    assert P.shape == (16, 16) and np.all(np.isfinite(P)) and np.all((P > 0) & (P < 1))
    assert np.isfinite(chain.mean).all() and np.isfinite(chain.m2).all()
    same = truth[:, None] == truth[None, :]
    off = ~np.eye(16, dtype=bool)
    assert P[same & off].mean() > P[~same].mean()
