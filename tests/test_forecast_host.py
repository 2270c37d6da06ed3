"""forecast(process, data, horizon) without a GPU: the argument errors raised before any device work, and the numpy
restatement of the law (tests/forecast_ref.py, part a) against closed forms on a bipartite model, where every mean is a
one-line integral: sources {0, 1} have no incoming weight, sinks {2, 3} no outgoing weight."""
import math

import numpy as np
import pytest

import forecast_ref as fr

S, H = 4000, 6.0


def bipartite(nhp, kind, dt_max=8.0):
    lam0 = np.array([0.9, 0.6, 0.3, 0.5])
    W = np.zeros((4, 4))
    W[:2, 2:] = [[0.5, 0.3], [0.2, 0.6]]
    r = np.random.default_rng(12)
    theta, mu, tau = r.uniform(0.15, 0.6, (4, 4)), r.normal(0.0, 1.0, (4, 4)), r.uniform(0.5, 2.0, (4, 4))
    imp = (nhp.ExponentialImpulseResponse(theta, 1.0, 1.0, dt_max) if kind == "exponential"
           else nhp.LogitNormalImpulseResponse(mu, tau, dt_max))
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), imp, nhp.DenseWeightModel(W))
    times, nodes, T0 = nhp.rand(proc, 70.0, seed=3)
    return proc, np.asarray(times), np.asarray(nodes), T0


def integral_of_cdf(m, p, c, h):
    """∫_0^h F_pc(d) dd: closed for the exponential, composite Gauss-Legendre for the logit-normal (F = 1 from Δtmax on)."""
    if m.expo:
        th = m.theta[p, c]
        return h - (1.0 - math.exp(-th * h)) / th
    top = min(h, m.dt_max)
    x, w = np.polynomial.legendre.leggauss(16)
    edges = np.linspace(0.0, top, 401)
    mid, half = 0.5 * (edges[1:] + edges[:-1]), 0.5 * np.diff(edges)
    d = (mid[:, None] + half[:, None] * x[None, :]).ravel()
    f = np.array([fr.cdf_ln(m.mu[p, c], m.tau[p, c], v, m.dt_max) for v in d])
    return float(np.sum(f * (half[:, None] * w[None, :]).ravel())) + (h - top)


def sink_means(proc, times, nodes, T0, h):
    m = fr.Model(proc)
    carry = fr.carry_expected(proc, times, nodes, T0, h)
    return np.array([m.lam0[c] * h + carry[c] + sum(m.lam0[p] * m.V[p, c] * integral_of_cdf(m, p, c, h) for p in (0, 1))
                     for c in (2, 3)]), carry


@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_restatement_against_closed_forms_on_a_bipartite_model(nhp, kind):
    proc, times, nodes, T0 = bipartite(nhp, kind)
    assert 150 <= len(times) <= 260
    counts = fr.ensemble(proc, times, nodes, T0, H, S, seed=5)
    assert counts.shape == (S, 4) and 10 <= counts.sum(axis=1).mean() <= 30
    lam0 = np.asarray(proc.baseline.λ)
    mean, se = counts.mean(axis=0), counts.std(axis=0, ddof=1) / math.sqrt(S)
    want, carry = sink_means(proc, times, nodes, T0, H)
    assert np.all(carry[:2] == 0.0) and np.all(carry[2:] > 0.5)        # the carry-over shows: > 10 standard errors
    z_src = (mean[:2] - lam0[:2] * H) / se[:2]
    z_snk = (mean[2:] - want) / se[2:]
    print(f"{kind}: carry {carry[2:]}, sink means {mean[2:]} vs {want}, z sources {z_src}, sinks {z_snk}")
    assert np.all(np.abs(z_src) < 4.5) and np.all(np.abs(z_snk) < 4.5)
    # a source's count is Poisson: variance = mean, to the spread of a sample variance (sqrt(2/S) relative, 4.5 of them)
    var = counts[:, :2].var(axis=0, ddof=1)
    assert np.all(np.abs(var / (lam0[:2] * H) - 1.0) < 4.5 * np.sqrt(2.0 / S + 1.0 / (S * lam0[:2] * H)))


def test_argument_errors_come_before_any_device_work(nhp):
    proc, times, nodes, T0 = bipartite(nhp, "exponential")
    data = (times, nodes, T0)
    disc = object.__new__(nhp.DiscreteStandardHawkesProcess)       # refused by its type, before anything is read from it
    with pytest.raises(TypeError, match="ContinuousStandardHawkesProcess.*ContinuousNetworkHawkesProcess"):
        nhp.forecast(disc, np.zeros((2, 10), dtype=np.int64), 1.0)
    x = np.linspace(0.0, T0, 5)
    lgcp = nhp.ContinuousStandardHawkesProcess(nhp.LogGaussianCoxProcess(x, [np.ones(5)] * 4), proc.impulses, proc.weights)
    with pytest.raises(NotImplementedError, match="the grid ends where the data end"):
        nhp.forecast(lgcp, data, 1.0)
    shard = object.__new__(nhp.ShardedDataset)
    with pytest.raises(NotImplementedError, match="column shard"):
        nhp.forecast(proc, shard, 1.0)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="nsamples"):
            nhp.forecast(proc, data, 1.0, nsamples=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="horizon"):
            nhp.forecast(proc, data, bad)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="max_events"):
            nhp.forecast(proc, data, 1.0, max_events=bad)


def test_window_start_and_carry_of_a_quiet_history(nhp):
    proc, times, nodes, T0 = bipartite(nhp, "logit-normal", dt_max=2.0)
    w0 = fr.window_start(times, T0, 2.0)
    assert 0 < w0 < len(times) and np.all(T0 - times[w0:] < 2.0) and T0 - times[w0 - 1] >= 2.0
    # a history that ends more than Δtmax before T0 carries nothing over; without weights nothing either
    assert np.all(fr.carry_expected(proc, times, nodes, times[-1] + 2.5, H) == 0.0)
    mute = nhp.ContinuousStandardHawkesProcess(proc.baseline, proc.impulses, nhp.DenseWeightModel(np.zeros((4, 4))))
    assert np.all(fr.carry_expected(mute, times, nodes, T0, H) == 0.0)
