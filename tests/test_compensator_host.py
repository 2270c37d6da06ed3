"""The compensator's definition, checked without a GPU: the numpy restatement (tests/compensator_ref.py) against
Gauss-Legendre quadrature of the CPU oracle's intensity, the identities the outputs satisfy, and the argument errors
raised before any device work."""
import numpy as np
import pytest

import compensator_ref as cr
from helpers import random_case


def _oracle_total(orc, om, times, nodes, T, dt_max, N, sub, grid_x=None):
    """∫₀ᵀ orc.intensity by 40-point Gauss-Legendre panels split at every t_i and t_i + Δtmax (and the LGCP grid)."""
    breaks = [np.array([0.0, T]), times, times + dt_max]
    if grid_x is not None:
        breaks.append(np.asarray(grid_x, float))
    b = np.concatenate(breaks)
    b = b[(b >= 0.0) & (b <= T)]
    return cr.gauss_legendre_total(lambda q: orc.intensity(om, times, nodes, q), b, N, sub=sub)


def _simulated(nhp, orc, kind, dt_max):
    """Host-simulated data (N = 3, T = 30, seed 1) from a seeded model, with the oracle's twin of the model."""
    N, T = 3, 30.0
    r = np.random.default_rng(1)
    lam0, W = r.uniform(0.3, 0.8, N), r.uniform(0.0, 0.5, (N, N)) / 1.5
    theta, mu, tau = r.uniform(1.0, 5.0, (N, N)) / dt_max, r.normal(0.0, 1.0, (N, N)), r.uniform(0.5, 2.0, (N, N))
    if kind == "exponential":
        imp, kw = nhp.ExponentialImpulseResponse(theta, 1.0, 1.0, dt_max), dict(theta=theta)
    else:
        imp, kw = nhp.LogitNormalImpulseResponse(mu, tau, dt_max), dict(mu=mu, tau=tau)
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), imp, nhp.DenseWeightModel(W))
    times, nodes, _ = nhp.rand(proc, T, seed=1)
    return cr.Model(lam0, W, dt_max, **kw), orc.ContModel(lam0, W, dt_max=dt_max, **kw), times, nodes, T, N


@pytest.mark.parametrize("kind,dt_max", [("exponential", 1.0), ("exponential", 0.5), ("logitnormal", 1.0), ("logitnormal", 2.0)])
def test_restatement_is_the_integral_of_the_oracle_intensity(nhp, orc, kind, dt_max):
    model, om, times, nodes, T, N = _simulated(nhp, orc, kind, dt_max)
    assert 40 <= len(times) <= 200
    want = _oracle_total(orc, om, times, nodes, T, dt_max, N, sub=1 if kind == "exponential" else 32)
    _, _, total = cr.compensator(model, times, nodes, T)
    err = np.max(np.abs(total - want) / want)
    print(f"{kind} dt_max={dt_max}: M={len(times)} max rel err of total {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("network,lgcp", [(True, False), (False, True)])
def test_restatement_network_mask_and_lgcp_baseline(nhp, orc, kind, network, lgcp):
    case = random_case(3, 90, 30.0, kind, 1.0, network=network, lgcp=lgcp, seed=5, nhp=nhp, orc=orc)
    model = cr.Model.of(case["proc"])
    want = _oracle_total(orc, case["om"], case["times"], case["nodes"], case["T"], 1.0, 3,
                         sub=1 if kind == "exponential" else 32, grid_x=model.grid_x)
    _, _, total = cr.compensator(model, case["times"], case["nodes"], case["T"])
    err = np.max(np.abs(total - want) / want)
    print(f"{kind} network={network} lgcp={lgcp}: max rel err of total {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_restatement_identities(nhp, kind):
    case = random_case(4, 300, 40.0, kind, 1.0, seed=3, nhp=nhp)
    model = cr.Model.of(case["proc"])
    at, res, total = cr.compensator(model, case["times"], case["nodes"], case["T"])
    nodes0 = case["nodes"] - 1
    assert np.all(res >= 0.0)
    for c in range(4):
        k = np.flatnonzero(nodes0 == c)
        assert abs(np.sum(res[k]) - at[k[-1]]) <= 1e-12 * at[k[-1]]          # the residuals telescope
        assert total[c] >= at[k[-1]]                                          # the censored tail is non-negative
    # the O(window + N) form used at the metric size is the same function
    np.testing.assert_allclose(cr.at_events_slice(model, case["times"], case["nodes"], 100, 200), at[100:200], rtol=1e-13)
    np.testing.assert_allclose(cr.total_closed_form(model, case["times"], case["nodes"], case["T"]), total, rtol=1e-13)


def test_restatement_without_weights_is_the_baseline():
    r = np.random.default_rng(0)
    N, M, T = 3, 200, 50.0
    times, nodes = np.sort(r.uniform(0.0, T, M)), r.integers(1, N + 1, M)
    lam0 = r.uniform(0.5, 1.5, N)
    model = cr.Model(lam0, np.zeros((N, N)), 1.0, theta=np.ones((N, N)))
    at, res, total = cr.compensator(model, times, nodes, T)
    for c in range(N):
        t = times[nodes == c + 1]
        # a difference of cumulative values loses ε·Λ: Λ <= 75 here, a few roundings of 1.7e-14
        np.testing.assert_allclose(res[nodes == c + 1], lam0[c] * np.diff(t, prepend=0.0), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(total, lam0 * T, rtol=1e-15)


def test_ks_pvalue_matches_scipy():
    from scipy import stats
    r = np.random.default_rng(2)
    for n, scale in ((50, 1.0), (2000, 1.0), (2000, 1.1)):
        x = r.exponential(scale, n)
        d, p = cr.ks_exp1(x)
        ref = stats.kstest(x, "expon")
        assert abs(d - ref.statistic) < 1e-12
        assert abs(p - ref.pvalue) < 0.02 + 0.05 * ref.pvalue, (p, ref.pvalue)


def test_discrete_process_is_refused(nhp):
    proc = object.__new__(nhp.DiscreteStandardHawkesProcess)       # refused by its type, before anything is read from it
    data = np.zeros((2, 10), dtype=np.int64)
    for fn in (nhp.compensator, nhp.time_rescaling_test):
        with pytest.raises(TypeError, match="ContinuousStandardHawkesProcess.*ContinuousNetworkHawkesProcess"):
            fn(proc, data)


def test_package_kolmogorov_pvalue(nhp):
    from nhp_amd.continuous import kolmogorov_pvalue
    r = np.random.default_rng(4)
    x = r.exponential(1.0, 500)
    d, p = cr.ks_exp1(x)
    assert kolmogorov_pvalue(d, 500) == pytest.approx(p, rel=1e-12)
    assert np.isnan(kolmogorov_pvalue(float("nan"), 0))
