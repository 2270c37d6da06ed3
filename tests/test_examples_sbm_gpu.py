"""The block-network example runs end to end on the GPU and finds the planted blocks."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_block_network_example():
    truth, blocks, rho_mean, chain = importlib.import_module("continuous_exponential_block_network_hawkes").main()
    assert chain.n == 200 and chain.block_counts.shape == (16, 2) and np.all(chain.block_counts.sum(axis=1) == 200)
    assert rho_mean.shape == (2, 2) and np.all((rho_mean > 0) & (rho_mean < 1))
    agree = max(np.mean(blocks == truth), np.mean(blocks == 1 - truth))
    assert agree >= 0.75, agree
    assert min(rho_mean[0, 0], rho_mean[1, 1]) > max(rho_mean[0, 1], rho_mean[1, 0])
