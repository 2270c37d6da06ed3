"""The latent distance network model without a GPU: the reference the GPU tests replay against (tests/latent_ref.py) held
to brute force, the streams and the sample sizes those tests rely on, and the host component
(components.LatentDistanceNetworkModel)."""
import math
import types

import numpy as np
import pytest
from scipy import stats

import latent_ref as lr


@pytest.fixture(autouse=True)
def component(nhp):
    """The reference restates the model of components.LatentDistanceNetworkModel; without the component there is nothing
    these tests pin."""
    return nhp.LatentDistanceNetworkModel


def test_conditional_is_the_difference_of_full_loglikelihoods():
    """L_n(z') - L_n(z) = loglik(z with z_n = z') - loglik(z): the conditional leaves out only terms without z_n."""
    rng = np.random.default_rng(0)
    for N, D in [(4, 1), (5, 2), (3, 3)]:
        A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
        z, b = rng.standard_normal((N, D)), 0.3
        for n in range(N):
            moved = z.copy()
            moved[n] = rng.standard_normal(D)
            want = lr.loglik(A, moved, b) - lr.loglik(A, z, b)
            got = lr.conditional(A, z, b, n, moved[n]) - lr.conditional(A, z, b, n)
            assert abs(got - want) < 1e-12
            assert abs(lr.conditional_vec(A, z, b, n, moved[n]) - lr.conditional(A, z, b, n, moved[n])) < 1e-12
        assert abs(lr.loglik_vec(A, z, b) - lr.loglik(A, z, b)) < 1e-12


def test_loglikelihood_is_the_bernoulli_log_probability():
    rng = np.random.default_rng(1)
    N = 4
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
    z, b = rng.standard_normal((N, 2)), -0.2
    P = lr.link_probability(z, b)
    assert abs(lr.loglik(A, z, b) - np.sum(A * np.log(P) + (1 - A) * np.log1p(-P))) < 1e-12
    assert np.allclose(P.diagonal(), 1.0 / (1.0 + math.exp(0.2)))


def test_candidate_angles_depend_on_the_uniforms_alone():
    """ess_step on two different likelihoods proposes the same angles: the candidates of a step can be laid out before
    any likelihood is known."""
    rng = np.random.default_rng(2)
    us = rng.uniform(size=100)
    th = lr.angles(us)
    assert len(th) == 100 and th[0] == lr.TWO_PI * us[0]
    lo, hi = th[0] - lr.TWO_PI, th[0]
    for k in range(1, 100):
        lo, hi = (th[k - 1], hi) if th[k - 1] < 0 else (lo, th[k - 1])
        assert lo <= 0.0 <= hi and lo <= th[k] <= hi                  # the current value (θ = 0) stays inside the bracket
    seen = []

    def spy(target):
        def L(x):
            seen[-1].append(x)
            return target(x)
        return L
    for target in (lambda x: -50.0 * (x - 0.3) ** 2, lambda x: -50.0 * (x + 2.0) ** 2):
        seen.append([])
        lr.ess_step(spy(target), 1.0, 0.5, 0.9, us)
    for a, b in zip(seen[0][1:], seen[1][1:]):                       # (the first call is L at the current value)
        assert a == b


def test_reference_chain_samples_the_exact_posterior():
    """The posterior test of the GPU file on the reference chain alone, with its thinning and sample size."""
    sigma, b = 1.0, 0.5
    for k, (name, A) in enumerate(lr.posterior_cases().items()):
        rng = np.random.default_rng(100 + k)
        z, out = np.array([[0.3], [-0.2]]), []
        for _ in range(lr.POSTERIOR_SAMPLES):
            for _ in range(lr.POSTERIOR_THIN):
                z, _, att, _, _ = lr.sweep(A, z, b, sigma, 0.0, 1.0, lr.make_draws(rng, 2, 1), do_offset=False, fast=False)
                assert max(att) <= lr.MAX_ATTEMPTS
            out.append(z[0, 0] - z[1, 0])
        p = stats.kstest(out, lambda x: lr.delta_cdf(A[0, 1] + A[1, 0], b, sigma, x)).pvalue
        assert p > lr.P_MIN, (name, p)
    # the linked pair sits closer than the unlinked one: the two targets are not the same distribution
    assert lr.delta_cdf(2.0, b, sigma, 1.0) - lr.delta_cdf(2.0, b, sigma, -1.0) > lr.delta_cdf(0.0, b, sigma, 1.0) - lr.delta_cdf(0.0, b, sigma, -1.0) + 0.2
    A, z, mu_b, sigma_b = lr.offset_posterior_case()
    rng = np.random.default_rng(200)
    bb, out = 0.0, []
    for _ in range(lr.POSTERIOR_SAMPLES):
        for _ in range(lr.OFFSET_THIN):
            d = lr.make_draws(rng, 3, 2)
            bb, att, _, _ = lr.offset_step(A, z, bb, mu_b, sigma_b, *_offset_draws(d, 3, 2))
            assert att <= lr.MAX_ATTEMPTS
        out.append(bb)
    p = stats.kstest(out, lambda x: lr.offset_cdf(A, z, mu_b, sigma_b, x)).pvalue
    assert p > lr.P_MIN, p


def _offset_draws(d, N, D):
    nrm, u0, us = lr.node_draws(d, N, D, 0, N)
    return nrm[0], u0, us


def _run(case):
    z, b, att, margins = case["z0"], case["b0"], [], []
    for s in range(case["n_sweeps"]):
        z, b, a, _, m = lr.sweep(case["A"], z, b, case["sigma"], case["mu_b"], case["sigma_b"], case["draws"], sweep_index=s)
        att += a; margins += m
    return z, b, att, margins


def test_no_gpu_case_has_a_candidate_near_its_threshold():
    """The GPU replay excuses steps whose smallest |L - threshold| is below 1e-9·max(1, |L|); with the chosen seeds every
    margin is at least 1e-6, so that exclusion can never hide a failure."""
    cases = dict(lr.decision_cases())
    cases["stale"] = lr.stale_case()
    for name, c in cases.items():
        z, b, att, margins = _run(c)
        assert min(margins) >= 1e-6, (name, min(margins))
        assert max(att) <= lr.MAX_ATTEMPTS and np.all(np.isfinite(z)) and np.isfinite(b)
    assert lr.decision_cases()["1x1"]["N"] == 1
    z, b, att, _ = _run(lr.decision_cases()["1x1"])
    assert att[0] == 1                                                  # N = 1: L ≡ 0, the first candidate passes
    # the stale-state case is only worth its name if the nodes move, and far, in a sweep
    c = lr.stale_case()
    z1, _, _, _, _ = lr.sweep(c["A"], c["z0"], c["b0"], c["sigma"], c["mu_b"], c["sigma_b"], c["draws"])
    moved = np.linalg.norm(z1 - c["z0"], axis=1)
    assert np.all(moved > 0) and np.mean(moved > 0.1) > 0.8 and moved.mean() > 0.5
    # the diagonal changes the offset's update and no position's
    c0, c1 = lr.decision_cases()["33x2-diag0"], lr.decision_cases()["33x2-diag1"]
    za, _, _, ta, _ = lr.sweep(c0["A"], c0["z0"], c0["b0"], 1.0, 0.0, 1.0, c0["draws"])
    zb, _, _, tb, _ = lr.sweep(c1["A"], c1["z0"], c1["b0"], 1.0, 0.0, 1.0, c1["draws"])
    assert np.array_equal(za, zb) and ta[:-1] == tb[:-1] and abs(ta[-1][0] - tb[-1][0]) > 1.0
    # the far case: finite and hugely negative
    far = lr.decision_cases()["33x2-far"]
    assert lr.loglik(far["A"], far["z0"], far["b0"]) < -1e5


def test_steered_streams_do_what_they_say():
    """The fallback case accepts exactly one candidate after the planned failures (on both sides of the batch edges) and
    the exhaustion case fails all 100 where planned: such streams exist for the rule as stated."""
    plan = [[6, 7, 8, 15, 16, 14], [23, 0, 40, 99, 1, 15], [2, 3, 4, 5, 6, 16], [0, 0, 0, 0, 0, 99]]
    c = lr.fallback_case()
    z, b, att, margins = _run(c)
    assert att == [f + 1 for fails in plan for f in fails]
    assert min(margins) >= 1e-6
    assert np.max(np.abs(z - 1.0)) < 1e-12 and abs(b - 1.0) < 1e-12
    c = lr.exhaustion_case()
    z, b, att, margins = _run(c)
    assert att == [101, 1, 4, 101, 1, 101] and min(margins) >= 1e-6
    assert np.array_equal(z[0], c["z0"][0]) and np.array_equal(z[3], c["z0"][3]) and b == c["b0"]     # kept, bit for bit
    for us in (lr.steering_uniforms(100), lr.steering_uniforms(40)):
        assert np.all((us >= 0) & (us < 1))


def test_reference_chain_separates_the_planted_clusters():
    c = lr.planted_case()
    gap = lr.reference_recovery_gap(c)
    truth_gap = lr.cluster_gap(lr.link_probability(c["z_true"], c["b_true"]), c["truth"])
    print(f"reference chain gap {gap:.3f}, gap of the generating link probabilities {truth_gap:.3f}")
    assert gap > 0.3 * truth_gap > 0.05


def test_component(nhp):
    N, D = 6, 3
    rng = np.random.default_rng(0)
    z = rng.standard_normal((N, D))
    net = nhp.LatentDistanceNetworkModel(N, D, z=z, b=0.7, σ=2.0, μb=0.1, σb=3.0)
    assert np.array_equal(net.params(), [0.7]) and net.z.shape == (N, D)
    P = net.link_probability()
    assert P.shape == (N, N) and np.allclose(P, lr.link_probability(z, 0.7), rtol=0, atol=1e-15)
    assert np.allclose(P, P.T) and np.allclose(P.diagonal(), 1.0 / (1.0 + math.exp(-0.7)))
    A = net.rand(np.random.default_rng(1))
    assert A.shape == (N, N) and set(np.unique(A)) <= {0.0, 1.0} and net.z.shape == (N, D) and not np.array_equal(net.z, z)
    d = nhp.LatentDistanceNetworkModel(4)
    assert d.ndims == 2 and np.all(d.z == 0) and d.b == 0.0 and np.all(d.link_probability() == 0.5)
    far = nhp.LatentDistanceNetworkModel(2, 1, z=[[0.0], [100.0]])
    assert far.link_probability()[0, 1] == 0.0                           # underflows without a warning
    proc = nhp.ContinuousNetworkHawkesProcess(nhp.HomogeneousProcess(np.ones(N)), nhp.ExponentialImpulseResponse(np.ones((N, N)), 1.0, 1.0, 1.0),
                                              nhp.DenseWeightModel(np.full((N, N), 0.1)), A, net)
    assert proc.params()[0] == net.b and len(proc.params()) == 1 + N + 3 * N * N


def test_component_refuses_bad_arguments(nhp):
    for D in (0, 9):
        with pytest.raises(ValueError):
            nhp.LatentDistanceNetworkModel(4, D)
    with pytest.raises(ValueError):
        nhp.LatentDistanceNetworkModel(0)
    with pytest.raises(nhp.DomainError):
        nhp.LatentDistanceNetworkModel(2, 1, z=[[0.0], [np.nan]])
    with pytest.raises(nhp.DomainError):
        nhp.LatentDistanceNetworkModel(2, 1, b=np.inf)
    for kw in ({"σ": 0.0}, {"σb": -1.0}, {"μb": np.nan}):
        with pytest.raises(nhp.DomainError):
            nhp.LatentDistanceNetworkModel(2, 1, **kw)


def test_variational_drivers_and_shards_refuse_the_model(nhp):
    from nhp_amd import chains, discrete
    from nhp_amd.sharded import ShardedDataset
    N, B = 4, 2
    net = nhp.LatentDistanceNetworkModel(N)
    dproc = nhp.DiscreteNetworkHawkesProcess(
        nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), 1.0), nhp.DiscreteGaussianImpulseResponse(np.full((N, N, B), 1.0 / B), 4, 1.0),
        nhp.SparseWeightModel(np.full((N, N), 0.05)), np.ones((N, N)), net, 1.0)
    with pytest.raises(NotImplementedError, match="LatentDistanceNetworkModel"):
        discrete._vb_kind(dproc, "vb!")
    proc = nhp.ContinuousNetworkHawkesProcess(nhp.HomogeneousProcess(np.ones(N)), nhp.ExponentialImpulseResponse(np.ones((N, N)), 1.0, 1.0, 1.0),
                                              nhp.DenseWeightModel(np.full((N, N), 0.1)), np.ones((N, N)), net)
    with pytest.raises(NotImplementedError, match="not sharded"):
        nhp.mcmc_(proc, ShardedDataset.__new__(ShardedDataset), nsteps=1, keep_samples=False)
    with pytest.raises(ValueError, match="positions_every"):
        nhp.mcmc_(proc, None, nsteps=1, positions_every=0)
    with pytest.raises(NotImplementedError, match="latent distance network"):
        chains.gather_device_summaries({0: (proc, None)}, 1, None, types.SimpleNamespace(world=1, rank=0))
