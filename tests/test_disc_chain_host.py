"""The discrete mcmc_'s new arguments, checked where no device is needed: every refusal happens before any device work."""
import numpy as np
import pytest


def standard(nhp, N=3, B=2, L=4):
    th = np.full((N, N, B), 1.0 / 4)
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    return nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(th, L, 1.0),
                                             nhp.DenseWeightModel(np.full((N, N), 0.1)), 1.0)


def network(nhp, net, N=3, weights=None):
    p = standard(nhp, N)
    return nhp.DiscreteNetworkHawkesProcess(p.baseline, p.impulses, weights or p.weights, np.ones((N, N)), net, 1.0)


@pytest.fixture
def no_device(nhp, monkeypatch):
    from nhp_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "default_context", refuse)
    monkeypatch.setattr(_lib, "lib", refuse)


def test_arguments_are_checked_before_any_device_work(nhp, no_device):
    data = np.ones((3, 40), dtype=np.int64)
    p = standard(nhp)
    with pytest.raises(ValueError, match="moments"):
        nhp.mcmc_(p, data, nsteps=4, diagnostics=True, moments=False)
    with pytest.raises(ValueError, match="diagnostics must be"):
        nhp.mcmc_(p, data, nsteps=4, diagnostics="all", moments=True)
    with pytest.raises(ValueError, match="batch_len"):
        nhp.mcmc_(p, data, nsteps=4, diagnostics=True, moments=True, batch_len=0)
    with pytest.raises(ValueError, match="batch_len"):
        nhp.mcmc_(p, data, nsteps=4, batch_len=-2)                  # checked on every route, as the continuous mcmc_ does


@pytest.mark.parametrize("route", [dict(moments=True), dict(keep_samples=False), dict(keep_samples=False, moments=True, diagnostics=True)])
def test_what_the_resident_route_is_not_built_for_is_refused_by_name(nhp, no_device, route):
    data = np.ones((3, 40), dtype=np.int64)
    x = np.array([0.0, 20.0, 40.0])
    lgcp = standard(nhp)
    lgcp.baseline = nhp.DiscreteLogGaussianCoxProcess(x, np.ones((3, 3)), None, 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="homogeneous baseline.*DiscreteLogGaussianCoxProcess"):
        nhp.mcmc_(lgcp, data, nsteps=4, **route)
    sparse = network(nhp, nhp.BernoulliNetworkModel(0.5, 3), weights=nhp.SparseWeightModel(np.full((3, 3), 0.1)))
    with pytest.raises(NotImplementedError, match="DenseWeightModel.*SparseWeightModel"):
        nhp.mcmc_(sparse, data, nsteps=4, **route)
    with pytest.raises(NotImplementedError, match="device_draws=False"):
        nhp.mcmc_(standard(nhp), data, nsteps=4, device_draws=False, **route)
    block = network(nhp, nhp.StochasticBlockNetworkModel(3, 2))
    with pytest.raises(NotImplementedError, match="StochasticBlockNetworkModel.*default route"):
        nhp.mcmc_(block, data, nsteps=4, **route)
    latent = network(nhp, nhp.LatentDistanceNetworkModel(3, 2))
    with pytest.raises(NotImplementedError, match="LatentDistanceNetworkModel.*default route"):
        nhp.mcmc_(latent, data, nsteps=4, **route)


def test_the_sums_follow_params_without_the_link_probability(nhp):
    from nhp_amd import discrete
    p = standard(nhp, N=4)
    assert discrete.disc_moments_length(p) == len(p.params()) == 4 + 16 * 2
    for net, k in ((nhp.BernoulliNetworkModel(0.5, 4), 1), (nhp.DenseNetworkModel(4), 0)):
        q = network(nhp, net, N=4)
        assert discrete.disc_moments_length(q) == len(q.params()) - k == 4 + 16 + 32 + 16
