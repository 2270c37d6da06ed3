"""The stochastic block network model without a GPU: the reference the GPU tests replay against (tests/sbm_ref.py) held to
brute-force enumeration of the joint, and the host component (components.StochasticBlockNetworkModel)."""
import numpy as np
import pytest

import sbm_ref as sr


@pytest.mark.parametrize("N,K", [(5, 2), (4, 3)])
def test_conditional_is_the_ratio_of_joint_probabilities(N, K):
    rng = np.random.default_rng(10 * N + K)
    A = (rng.uniform(size=(N, N)) < 0.4).astype(np.float64)          # diagonal included
    assert A.diagonal().any() and not A.diagonal().all()
    rho = rng.uniform(0.05, 0.95, (K, K))
    pi = rng.dirichlet(np.full(K, 2.0))
    worst = 0.0
    for z in sr.all_labelings(N, K):
        for n in range(N):
            worst = max(worst, np.max(np.abs(sr.conditional(A, z, n, rho, pi) - sr.conditional_by_enumeration(A, z, n, rho, pi))))
    assert worst < 1e-14, worst


def test_conditionals_sum_the_joint_over_one_label():
    # Σ_k joint(z_n = k) / joint = 1 / p(z_n | rest): the conditional against the full normalised joint at (5, 2)
    N, K = 5, 2
    rng = np.random.default_rng(3)
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
    rho, pi = rng.uniform(0.1, 0.9, (K, K)), np.array([0.3, 0.7])
    states = list(sr.all_labelings(N, K))
    joint = np.exp([sr.log_joint(A, z, rho, pi) for z in states])
    joint /= joint.sum()
    for z, pz in zip(states, joint):
        for n in range(N):
            rest = sum(pj for zj, pj in zip(states, joint) if all(zj[m] == z[m] for m in range(N) if m != n))
            assert abs(sr.conditional(A, z, n, rho, pi)[z[n]] - pz / rest) < 1e-14


@pytest.mark.parametrize("N,K", sr.SHAPES)
def test_counts_match_a_double_loop(N, K):
    c = sr.make_case(N, K, 5 + N)
    L, n = sr.counts(c["A"], c["z0"], K)
    L2, n2 = sr.counts_loops(c["A"], c["z0"], K)
    assert np.array_equal(L, L2) and np.array_equal(n, n2)
    assert L.sum() == int(c["A"].sum()) and n.sum() == N


def test_component(nhp):
    N, K = 7, 3
    rng = np.random.default_rng(0)
    rho = rng.uniform(0.1, 0.9, (K, K))
    pi = np.array([0.2, 0.3, 0.5])
    z = np.array([0, 1, 2, 2, 1, 0, 2])
    net = nhp.StochasticBlockNetworkModel(N, K, ρ=rho, π=pi, z=z, α=2.0, β=3.0, γ=0.5)
    P = net.link_probability()
    assert P.shape == (N, N)
    for p in range(N):
        for c in range(N):
            assert P[p, c] == rho[z[p], z[c]]
    x = net.params()                                                     # [vec(ρ) column-major; π]
    assert len(x) == K * K + K
    assert np.array_equal(x[:K * K], rho.ravel(order="F")) and np.array_equal(x[K * K:], pi)
    assert x[1] == rho[1, 0] and x[K] == rho[0, 1]
    A = net.rand(np.random.default_rng(1))
    assert A.shape == (N, N) and set(np.unique(A)) <= {0.0, 1.0}
    assert net.z.shape == (N,) and net.z.min() >= 0 and net.z.max() < K
    # defaults: ρ = 0.5, π uniform, labels round-robin
    d = nhp.StochasticBlockNetworkModel(5, 2)
    assert np.all(d.ρ == 0.5) and np.allclose(d.π, 0.5) and list(d.z) == [0, 1, 0, 1, 0]
    # K = 1 is the Bernoulli model: a constant matrix
    one = nhp.StochasticBlockNetworkModel(6, 1, ρ=[[0.3]])
    assert np.array_equal(one.link_probability(), nhp.BernoulliNetworkModel(0.3, 6).link_probability())
    assert len(one.params()) == 2 and one.params()[0] == 0.3 and one.params()[1] == 1.0
    # a network process carries the block model's parameters in front, like ρ of the Bernoulli model
    proc = nhp.ContinuousNetworkHawkesProcess(nhp.HomogeneousProcess(np.ones(N)), nhp.ExponentialImpulseResponse(np.ones((N, N)), 1.0, 1.0, 1.0),
                                              nhp.DenseWeightModel(np.full((N, N), 0.1)), A, net)
    assert np.array_equal(proc.params()[:K * K + K], net.params())


def test_component_refuses_bad_arguments(nhp):
    with pytest.raises(ValueError):
        nhp.StochasticBlockNetworkModel(4, 0)
    with pytest.raises(ValueError):
        nhp.StochasticBlockNetworkModel(4, 65)
    with pytest.raises(nhp.DomainError):
        nhp.StochasticBlockNetworkModel(4, 2, z=[0, 1, 2, 0])
    with pytest.raises(nhp.DomainError):
        nhp.StochasticBlockNetworkModel(4, 2, ρ=[[0.5, 1.0], [0.5, 0.5]])
    with pytest.raises(nhp.DomainError):
        nhp.StochasticBlockNetworkModel(4, 2, π=[0.5, 0.6])
    with pytest.raises(nhp.DomainError):
        nhp.StochasticBlockNetworkModel(4, 2, α=0.0)


def test_no_gpu_case_has_a_uniform_near_a_boundary():
    """The GPU decision test excuses nodes whose uniform lies within 1e-9 of a cumulative boundary; with the chosen seeds no
    node of any case does, so that exclusion can never hide a failure."""
    cases = dict(sr.decision_cases())
    cases["stale"] = sr.stale_case()
    for name, c in cases.items():
        zs, probs, margins = sr.run_sweeps(c)
        assert margins.min() > 1e-9, (name, margins.min())
        assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-14)
        assert zs[-1].min() >= 0 and zs[-1].max() < c["K"]
    # the stale-tables case is only worth its name if most nodes move in the first sweep
    c = sr.stale_case()
    zs, _, _ = sr.run_sweeps(c)
    assert np.mean(zs[0] != c["z0"]) > 0.5


def test_planted_partition_is_recovered_by_the_reference_chain():
    c = sr.planted_case()
    z = c["z0"].astype(np.int64)
    for _ in range(sr.RECOVERY_ITERS):
        rho, pi, u = sr.recovery_draws(c, z, c["rng"])
        z, _, _ = sr.sweep(c["A"], z, rho, pi, u)
    assert sr.same_partition(z, c["truth"])


def test_device_gather_of_chain_summaries_refuses_a_block_network(nhp):
    """nhp_gather_moments exchanges the scalar ρ's sums only; a block network's K² + K sums are not in it, so the device
    gather refuses (run_chains sends such chains through the host exchange, where res.mean / res.m2 are complete)."""
    import types
    from nhp_amd import chains
    N = 4
    net = nhp.StochasticBlockNetworkModel(N, 2)
    proc = nhp.ContinuousNetworkHawkesProcess(nhp.HomogeneousProcess(np.ones(N)), nhp.ExponentialImpulseResponse(np.ones((N, N)), 1.0, 1.0, 1.0),
                                              nhp.DenseWeightModel(np.full((N, N), 0.1)), np.ones((N, N)), net)
    with pytest.raises(NotImplementedError, match="block network"):
        chains.gather_device_summaries({0: (proc, None)}, 1, None, types.SimpleNamespace(world=1, rank=0))
