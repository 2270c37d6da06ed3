"""tests/lgcp_ref.py against closed forms, against itself in float64, and against the oracle; and the serial elliptical-slice
restatement against the posterior it must leave invariant -- with three mutants that the same harness must reject, which is
what gives the GPU invariance test of tests/test_lgcp_edges_gpu.py its teeth.  No GPU."""
import math

import numpy as np
import pytest

import lgcp_ref as ref

CONT = sorted(ref.CASES)
DISC = sorted(ref.DISC_CASES)
SIGMA2 = np.array([[1.0, 0.6], [0.6, 1.0]])
M2 = math.log(1.5)
EVENTS = (0.5, 1.0, 3.5)
X2 = 4.0
REPLICAS = 128


def test_case_builders_hold_what_they_promise():
    c = ref.prepared("knots")[0]["counts"]
    assert 1400 <= c["M"] <= 1600 and c["silent"] == 1 and c["at_zero"] >= 1
    assert c["interior_points_hit"] >= 3 and c["doubled"] >= 1 and c["on_interior"] >= 5
    assert c["last_cell"] >= 10 and c["at_end"] >= 1
    assert ref.prepared("narrow")[0]["counts"]["in_narrow"] >= 30
    assert len(ref.prepared("one_cell")[0]["grid_x"]) == 2
    for name in CONT:
        case = ref.prepared(name)[0]
        k = case["counts"]
        assert k["all_attributed"] >= 1, name
        assert k["none_attributed"] >= 1 or case["N"] == 1, name
        assert np.all(np.diff(case["times"]) >= 0) and case["times"][-1] <= case["grid_x"][-1]
    assert ref.prepared("crowded")[0]["counts"]["base_events"] == 50000
    for g in (4094, 4095, 4096):
        assert len(ref.prepared("wide_grid(%d)" % g)[0]["grid_x"]) == g
    for name in DISC:
        d = ref.disc_case(name)
        assert d["bins_on_grid"] >= 1 and d["data"].min() == 0
    assert max(ref.disc_case(n)["data"].max() for n in DISC) >= 35
    assert ref.disc_case("x0=1")["bins_at_end"] == 1 and all(ref.disc_case(n)["bins_at_end"] == 0 for n in DISC if n != "x0=1")


def test_constant_and_linear_curves_have_closed_forms():
    case = ref.prepared("knots")[0]
    t, nodes, pn, N, gx = (case[k] for k in ("times", "nodes", "parentnodes", "N", "grid_x"))
    X = np.longdouble(gx[-1])
    nb = np.array([((nodes == c + 1) & (pn == 0)).sum() for c in range(N)])
    k = np.array([0.3, 1.0, 2.5, 7.0, 0.01])
    res = ref.cont_candidate_ll(t, nodes, pn, N, gx, np.repeat(k[:, None], len(gx), axis=1))
    want = -np.asarray(k, dtype=np.longdouble) * X + nb * np.log(np.asarray(k, dtype=np.longdouble))
    assert np.all(np.abs(res.ll - want) <= res.bound)
    a, b = np.array([0.5, 1.0, 2.0, 0.25, 3.0]), np.array([0.125, 0.0, 0.5, 1.0, 0.03125])
    res = ref.cont_candidate_ll(t, nodes, pn, N, gx, a[:, None] + b[:, None] * gx[None, :])
    want = np.zeros(N, dtype=np.longdouble)
    for c in range(N):
        tc = np.asarray(t[(nodes == c + 1) & (pn == 0)], dtype=np.longdouble)
        want[c] = -(a[c] * X + b[c] * X * X / 2) + np.log(a[c] + b[c] * tc).sum()
    assert np.all(np.abs(res.ll - want) <= res.bound)
    # discrete: a constant curve makes every bin Poisson(k·dt)
    d = ref.disc_case("dt.5")
    s = d["data"].T
    G = len(d["grid_x"])
    kk = np.array([0.7, 2.0, 11.0])
    res = ref.disc_candidate_ll(s, d["grid_x"], np.repeat(kk[None, :], G, axis=0), d["dt"])
    for n in range(3):
        lam = kk[n] * d["dt"]
        want = sum(int(v) * math.log(lam) - lam - math.lgamma(int(v) + 1.0) for v in s[:, n])
        assert abs(float(res.ll[n]) - want) <= res.bound[n]


@pytest.mark.parametrize("name", CONT)
def test_float64_evaluations_stay_inside_the_continuous_bound(name):
    case, res = ref.prepared(name)
    for order in ("forward", "reversed"):
        got = ref.cont_candidate_ll(case["times"], case["nodes"], case["parentnodes"], case["N"], case["grid_x"], case["lam"],
                                    real=np.float64, order=order)
        r, bad = ref.ratio(got.ll, res)
        assert len(bad) == 0, (name, order, r)
    # a node without baseline events is the trapezoid sum alone
    c = case["none_base"]
    if c is not None:
        assert res.n[c - 1] == 0 and abs(float(res.ll[c - 1]) + ref.sequential_trapezoid(case["grid_x"], case["lam"][c - 1])) <= res.bound[c - 1]


@pytest.mark.parametrize("name", DISC)
def test_float64_evaluations_stay_inside_the_discrete_bound(name):
    d = ref.disc_case(name)
    cand = np.exp(d["m"] + d["Y"])
    res = ref.disc_candidate_ll(d["data"].T, d["grid_x"], cand, d["dt"])
    for order in ("forward", "reversed"):
        got = ref.disc_candidate_ll(d["data"].T, d["grid_x"], cand, d["dt"], real=np.float64, order=order)
        r, bad = ref.ratio(got.ll, res)
        assert len(bad) == 0, (name, order, r)


@pytest.mark.parametrize("name", ["knots", "one_cell", "narrow"])
def test_oracle_continuous_inside_the_bound(orc, name):
    case, res = ref.prepared(name)
    got = orc.lgcp_loglik(case["times"], case["nodes"], case["parentnodes"], case["N"], case["grid_x"], case["lam"])
    r, bad = ref.ratio(got, res)
    assert len(bad) == 0, (name, r, got, res.ll)


@pytest.mark.parametrize("name", DISC)
def test_oracle_discrete_inside_the_bound(orc, name):
    d = ref.disc_case(name)
    cand = np.exp(d["m"] + d["Y"])
    res = ref.disc_candidate_ll(d["data"].T, d["grid_x"], cand, d["dt"])
    got = orc.disc_lgcp_loglik(d["data"].T, d["grid_x"], cand, d["dt"])
    r, bad = ref.ratio(got, res)
    assert len(bad) == 0, (name, r)


def test_scripted_rng_replays_the_generator():
    rng = ref.ScriptedRng(5)
    plain = np.random.default_rng(5)
    a, b = rng.standard_normal((3, 4)), rng.uniform(size=3)
    assert np.array_equal(a, plain.standard_normal((3, 4))) and np.array_equal(b, plain.uniform(size=3))
    assert [k for k, _ in rng.record] == ["normal", "uniform"] and np.array_equal(rng.record[1][1], b)


def _start(seed):
    return np.random.default_rng(seed).standard_normal((REPLICAS, 2)) @ np.linalg.cholesky(SIGMA2).T


def _pvalues(sampler_ll, use_log_u=True, seed=1):
    truth = ref.two_point_cont_loglik(X2, M2, EVENTS)
    cdfs = ref.posterior_cdfs(truth, SIGMA2)
    sweep = ref.serial_sweeper(sampler_ll, np.linalg.cholesky(SIGMA2), seed, REPLICAS, use_log_u=use_log_u)
    return ref.invariance_pvalues(sweep, _start(seed), cdfs)


def test_serial_loop_leaves_the_posterior_invariant():
    p = _pvalues(ref.two_point_cont_loglik(X2, M2, EVENTS))
    assert min(p) > ref.P_MIN, p
    # ... and the Poisson-count likelihood
    counts, dt = (3, 0, 1, 2, 0, 4, 1, 2), 1.0
    ll = ref.two_point_disc_loglik(8.0, M2, counts, dt)
    sweep = ref.serial_sweeper(ll, np.linalg.cholesky(SIGMA2), 2, REPLICAS)
    p = ref.invariance_pvalues(sweep, _start(2), ref.posterior_cdfs(ll, SIGMA2))
    assert min(p) > ref.P_MIN, p


def test_posterior_quadrature_without_data_is_the_prior():
    from scipy import stats
    cdfs = ref.posterior_cdfs(lambda a, b: 0.0 * a, SIGMA2)
    v = np.linspace(-3, 3, 13)
    assert np.max(np.abs(cdfs[0](v) - stats.norm.cdf(v))) < 1e-5 and np.max(np.abs(cdfs[1](v) - stats.norm.cdf(v))) < 1e-5


def test_the_harness_rejects_three_mutants():
    # 1. the slice level without log u: the chain only climbs (or uses up its attempts)
    try:
        p = _pvalues(ref.two_point_cont_loglik(X2, M2, EVENTS), use_log_u=False)
    except RuntimeError:
        p = (0.0, 0.0)
    assert min(p) < ref.P_MIN, p
    # 2. one of the three events dropped from the likelihood
    p = _pvalues(ref.two_point_cont_loglik(X2, M2, EVENTS[:2]))
    assert min(p) < ref.P_MIN, p
    # 3. the two interpolation weights swapped
    p = _pvalues(ref.two_point_cont_loglik(X2, M2, EVENTS, weights_swapped=True))
    assert min(p) < ref.P_MIN, p
