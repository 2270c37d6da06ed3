"""The continuous network variational fit's definition, checked without a GPU: the numpy/scipy restatement
(tests/cnetvb_ref.py) raises its ELBO at every step for both impulse families under a Bernoulli and a dense network, its dense
limit is tests/vb_ref.py's standard fit, its logit is the literal formula, ContinuousNetworkVariational's accessors return
what the planes hold, and the argument errors are raised before any device work."""
import numpy as np
import pytest
from scipy.special import digamma, gammaln

import cnetvb_ref as cr
import em_ref as er
import vb_ref as vr
from helpers import random_case

SLAB = dict(alpha0=2.0, beta0=1.5, kappa=1.5, nu=2.0, a=2.0, b=0.7, mu_mu=-0.5, kappa_mu=2.0)


def _problem(nhp, kind, dt_max, recursive):
    N = 4
    c = random_case(N, 400, 40.0, kind, dt_max, seed=11, nhp=nhp)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive)
    guess = er.from_vector(np.random.default_rng(3).uniform(0.2, 0.8, len(c["proc"].params())), N, kind, dt_max)
    return N, pr, guess


@pytest.mark.parametrize("net", [cr.NET, None], ids=["bernoulli", "dense"])
@pytest.mark.parametrize("kind,dt_max,recursive", [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)])
def test_restated_elbo_never_falls(nhp, kind, dt_max, recursive, net):
    """25 restated updates from a random guess, spike (0.3, 30), slab (1.5, 2).  Every block is an exact coordinate-ascent
    update, so L_{k+1} >= L_k in exact arithmetic; the sums are math.fsum, so what is left is the rounding of the terms' own
    evaluation: 1e-11·max(1, |L|), the bound tests/test_cont_vb_host.py holds the standard trace to."""
    N, pr, guess = _problem(nhp, kind, dt_max, recursive)
    q = cr.priors(net=net, base=SLAB)
    state, trace = cr.run(guess, pr, q, 25, *cr.NET_START)
    assert len(trace) == 25 and np.all(np.isfinite(trace))
    rise = np.diff(trace)
    print(f"{kind} dt_max={dt_max} recursive={recursive} net={net}: L {trace[0]:.4f} -> {trace[-1]:.6f}, smallest rise {rise.min():.3e}")
    assert rise.min() >= -1e-11 * max(1.0, abs(trace[-1]))
    assert trace[-1] > trace[0]
    assert trace[-1] == pytest.approx(cr.elbo(state, pr, q, dt_max), rel=1e-13)
    back = cr.from_planes(*cr.planes(state), N, kind)
    assert all(np.array_equal(back[k], state[k]) for k in state)
    if net is None:
        assert np.all(state["rho"] == 1.0) and (state["na"], state["nb"]) == cr.NET_START
    else:
        assert np.all((state["rho"] > 0.0) & (state["rho"] <= 1.0))
        assert state["na"] + state["nb"] == pytest.approx(net[0] + net[1] + N * N, rel=1e-14)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_the_dense_limit_is_the_standard_fit(nhp, kind):
    """ρ ≡ 1: the slab's tables, the trace and the surrogate are tests/vb_ref.py's, whatever the spike."""
    N, pr, guess = _problem(nhp, kind, 1.5, False)
    got, trace = cr.run(guess, pr, cr.priors(net=None, base=SLAB), 6, *cr.NET_START)
    want, wtrace = vr.run(guess, pr, SLAB, 6)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert np.allclose(trace, wtrace, rtol=1e-13, atol=0.0)


def test_the_logit_is_the_literal_formula_and_its_limits():
    """The cancellation-free logit against the definition's literal form (scipy's gammaln), on tables on both sides of the
    lnΓ difference's threshold; symmetric priors give the network's term exactly; a node without events gives the network's
    term up to the rounding of terms that cancel."""
    rng = np.random.default_rng(4)
    q = cr.priors(base=SLAB)
    EM, cnt = rng.uniform(0.0, 60.0, (5, 5)), rng.integers(0, 80, 5).astype(float)
    EM[0], cnt[0] = 0.0, 0.0
    st = dict(kappa0=q["kappa0"] + EM, nu0=q["nu0"] + cnt[:, None] * np.ones((5, 5)), kappa=q["kappa"] + EM, nu=q["nu"] + cnt[:, None] * np.ones((5, 5)))
    assert np.any(st["kappa0"] < 16.0) and np.any(st["kappa0"] >= 16.0)
    na, nb = cr.NET_START
    net = digamma(na) - digamma(nb)
    side = lambda k, n, kv, nv: k * np.log(n) - gammaln(k) + gammaln(kv) - kv * np.log(nv)
    literal = net + side(q["kappa"], q["nu"], st["kappa"], st["nu"]) - side(q["kappa0"], q["nu0"], st["kappa0"], st["nu0"])
    got = cr.logit(st, na, nb, q)
    assert np.max(np.abs(got - literal)) <= 1e-12 * np.max(np.abs(literal))
    assert np.max(np.abs(got[0] - net)) <= 1e-14
    sym = cr.priors(spike=(SLAB["kappa"], SLAB["nu"]), base=SLAB)
    st_sym = dict(st, kappa0=st["kappa"], nu0=st["nu"])
    assert np.all(cr.logit(st_sym, na, nb, sym) == net)


def _state_object(nhp, state, kind, N, q, **kw):
    return nhp.ContinuousNetworkVariational(kind, N, *cr.planes(state), prior_kappa=q["kappa"], **kw)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_the_result_class_returns_what_the_planes_hold(nhp, kind):
    N = 3
    q = cr.priors(base=SLAB)
    st = cr.random_state(N, kind, seed=5)
    res = _state_object(nhp, st, kind, N, q)
    assert isinstance(res, nhp.ContinuousVariational)
    for name, key in (("kappa0", "kappa0"), ("nu0", "nu0"), ("rho", "rho"), ("kappa", "kappa"), ("nu", "nu"), ("a", "a"), ("b", "b")):
        assert np.array_equal(getattr(res, name), st[key]), name
    assert (res.net_alpha, res.net_beta) == cr.NET_START and not res.dense
    assert np.array_equal(res.link_probability(), st["rho"]) and res.link_probability() is not res.rho
    want = (1.0 - st["rho"]) * st["kappa0"] / st["nu0"] + st["rho"] * st["kappa"] / st["nu"]
    assert np.allclose(res.effective_weight_mean(), want, rtol=1e-15, atol=0.0)
    # mean / sd / interval run over the S, R planes in their own order, the slab for W (the last N² entries)
    S, R, _ = cr.planes(st)
    mean, sd = res.mean(), res.sd()
    lo, hi = res.interval(0.9)
    assert mean.shape == sd.shape == lo.shape == hi.shape == S.shape
    assert np.array_equal(mean[-N * N:], (st["kappa"] / st["nu"]).ravel(order="F")) and np.array_equal(mean[:N], st["alpha"] / st["beta"])
    assert np.allclose(sd[-N * N:], (np.sqrt(st["kappa"]) / st["nu"]).ravel(order="F"), rtol=1e-15)
    assert np.all(lo[-N * N:] < mean[-N * N:]) and np.all(mean[-N * N:] < hi[-N * N:])
    assert np.array_equal(res.expected_links(), st["kappa"] - q["kappa"])
    with pytest.raises(ValueError, match="Q must hold"):
        nhp.ContinuousNetworkVariational(kind, N, S, R, np.ones(3 * N * N))
    with pytest.raises(ValueError, match="Parameter vector length"):
        nhp.ContinuousNetworkVariational(kind, N, S[:-1], R[:-1], cr.planes(st)[2])


def _network_process(nhp, N=3, kind="exponential", network=None, weights=None, lgcp=False):
    c = random_case(N, 50, 10.0, kind, 1.0, lgcp=lgcp, seed=1, nhp=nhp)
    base = c["proc"]
    w = nhp.SparseWeightModel(base.weights.W, 0.3, 30.0, 1.5, 2.0) if weights is None else weights
    net = nhp.BernoulliNetworkModel(0.4, N, 1.5, 2.5, 2.0, 3.0) if network is None else network
    return nhp.ContinuousNetworkHawkesProcess(base.baseline, base.impulses, w, np.ones((N, N)), net), c["data"]


def test_argument_errors_are_raised_before_any_device_work(nhp):
    """DenseWeightModel on a network process: TypeError (as before this fit existed); a block or latent distance network, an
    LGCP baseline and a ShardedDataset: NotImplementedError; a hyper-parameter, ρv table, guess or state that cannot be:
    ValueError / TypeError -- none of them touches a device."""
    N = 3
    for fn in (nhp.vb_, nhp.update_):
        proc, data = _network_process(nhp, weights=nhp.DenseWeightModel(np.full((N, N), 0.1)))
        with pytest.raises(TypeError, match="SparseWeightModel"):
            fn(proc, data)
        sbm = nhp.StochasticBlockNetworkModel(N, 2)
        with pytest.raises(NotImplementedError, match="StochasticBlockNetworkModel"):
            fn(*_network_process(nhp, network=sbm))
        latent = object.__new__(nhp.LatentDistanceNetworkModel)
        with pytest.raises(NotImplementedError, match="LatentDistanceNetworkModel"):
            fn(*_network_process(nhp, network=latent))
        with pytest.raises(NotImplementedError, match="LogGaussianCoxProcess"):
            fn(*_network_process(nhp, lgcp=True))
        proc, data = _network_process(nhp)
        with pytest.raises(NotImplementedError, match="shard"):
            fn(proc, object.__new__(nhp.ShardedDataset))
        for holder, name in ((proc.weights, "κ0"), (proc.weights, "ν0"), (proc.weights, "κ1"), (proc.network, "α"), (proc.network, "β"),
                             (proc.network, "αv"), (proc.network, "βv"), (proc.baseline, "α0")):
            for bad in (0.0, -1.0, np.nan, np.inf):
                keep = getattr(holder, name)
                setattr(holder, name, bad)
                with pytest.raises(ValueError, match="must be positive and finite"):
                    fn(proc, data)
                setattr(holder, name, keep)
        proc.weights.ρv = np.full((N, N), 1.5)
        with pytest.raises(ValueError, match="ρv"):
            fn(proc, data)
        proc.weights.ρv = None
        with pytest.raises(TypeError, match="ContinuousNetworkVariational"):
            fn(proc, data, init=nhp.ContinuousVariational("exponential", N, *vr.planes(vr.random_state(N, "exponential", 1))))
        other = _state_object(nhp, cr.random_state(N, "logitnormal", 1), "logitnormal", N, cr.priors())
        with pytest.raises(ValueError, match="Parameter vector length"):
            fn(proc, data, init=other)
    proc, data = _network_process(nhp)
    with pytest.raises(ValueError, match="Parameter vector length"):
        nhp.vb_(proc, data, guess=np.full(7, 0.5))
    with pytest.raises(ValueError):
        nhp.vb_(proc, data, max_steps=0)
    good = _state_object(nhp, cr.random_state(N, "exponential", 1), "exponential", N, cr.priors())
    with pytest.raises(ValueError, match="not both"):
        nhp.vb_(proc, data, init=good, guess=np.full(N + 2 * N * N, 0.5))
    # a dense network reads neither the Beta prior nor its variational pair
    dense, data = _network_process(nhp, network=nhp.DenseNetworkModel(N))
    from nhp_amd import inference
    pr, netp, is_dense = inference._netvb_check(dense, data, "vb!")
    assert is_dense and (pr.kappa, pr.nu) == (1.5, 2.0) and list(netp[:2]) == [0.3, 30.0]
    Q = inference._netvb_start_Q(dense, True)
    assert Q.shape == (3 * N * N + 2,) and np.all(Q[2 * N * N:3 * N * N] == 1.0)
    proc.weights.ρv = np.full((N, N), 0.25)
    assert np.all(inference._netvb_start_Q(proc, False)[2 * N * N:3 * N * N] == 0.25) and list(inference._netvb_start_Q(proc, False)[-2:]) == [2.0, 3.0]
