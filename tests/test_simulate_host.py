"""rand(process, duration; device=...): the argument errors raised before any device work, and the host route unchanged."""
import numpy as np
import pytest


def _continuous(nhp):
    W = np.array([[0.2, 0.1], [0.0, 0.3]])
    return nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.array([0.5, 1.0])),
                                               nhp.ExponentialImpulseResponse(2 * np.ones((2, 2))), nhp.DenseWeightModel(W))


def _discrete(nhp):
    p = nhp.DiscreteStandardHawkesProcess.__new__(nhp.DiscreteStandardHawkesProcess)
    p.baseline = nhp.DiscreteHomogeneousProcess(np.array([0.2, 0.4]), 1.0)
    p.impulses = nhp.DiscreteGaussianImpulseResponse.__new__(nhp.DiscreteGaussianImpulseResponse)
    p.impulses.θ, p.impulses.nlags, p.impulses.dt = np.full((2, 2, 2), 0.5), 4, 1.0
    p.impulses.basis = lambda: np.full((4, 2), 0.25)
    p.weights, p.dt = nhp.DenseWeightModel(np.full((2, 2), 0.2)), 1.0
    return p


def test_device_rand_of_a_discrete_process_is_not_implemented(nhp):
    with pytest.raises(NotImplementedError, match="continuous"):
        nhp.rand(_discrete(nhp), 100, seed=0, device=True)


def test_parents_need_the_device_route(nhp):
    with pytest.raises(ValueError, match="device=True"):
        nhp.rand(_continuous(nhp), 100.0, seed=0, return_parents=True)
    with pytest.raises(ValueError, match="device=True"):
        nhp.rand(_discrete(nhp), 100, seed=0, return_parents=True, device=False)


def test_host_route_is_the_host_simulator(nhp):
    proc = _continuous(nhp)
    a = nhp.rand(proc, 500.0, seed=3, device=False, max_events=5_000_000)
    b = nhp.synthetic.rand_continuous(proc, 500.0, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    with pytest.raises(RuntimeError, match="exploded"):
        nhp.rand(proc, 500.0, seed=3, max_events=10)
