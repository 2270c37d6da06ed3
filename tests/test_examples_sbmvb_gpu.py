"""examples/discrete_gaussian_block_network_hawkes_vb.py on the GPU, with the settings it ships with: it recovers the planted
partition, as it says.  (The numpy reference on the same data and start reaches it with a smallest max_k mv of 0.797; data
seeds 3 and 5 recover, 4 leaves one node on the wrong side.)"""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_the_block_network_vb_example_recovers_the_planted_blocks(capsys):
    ex = importlib.import_module("discrete_gaussian_block_network_hawkes_vb")
    fit, truth, labels = ex.main()
    out = capsys.readouterr().out
    planted = truth.network.z
    assert np.array_equal(labels, planted) or np.array_equal(1 - labels, planted)
    assert "planted partition recovered up to the swap of the labels: True" in out
    assert "links classified as in the truth" in out and "E[π]" in out
    net = fit.network
    assert net.mv.shape == (12, 2) and np.array_equal(net.z, labels)
    assert min(net.ρ[0, 0], net.ρ[1, 1]) > max(net.ρ[0, 1], net.ρ[1, 0])         # links are likelier inside a block
