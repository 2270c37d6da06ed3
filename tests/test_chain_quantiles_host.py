"""The numpy restatement of the streaming quantiles (tests/chain_quantiles_ref.py, from include/nhp.h) against np.quantile on
stored series, its invariants on series with ties, exact zeros and a constant, and the argument checks of mcmc_ that come
before the library is touched.  No GPU: this tests the algorithm, nothing on the device."""
import numpy as np
import pytest

import chain_quantiles_ref as ref

PROBS = (0.025, 0.5, 0.975)

# Worst rank error |F̂_n(q̂) − p| over the 1000 entries of each group, measured with this file (printed by the test), and the
# bound asserted: twice the measurement.
#   group   n      measured (p = 0.025, 0.5, 0.975)
MEASURED = {
    ("plain", 200): (0.045, 0.100, 0.140),
    ("plain", 1000): (0.022, 0.026, 0.037),
    ("gamma", 200): (0.025, 0.065, 0.075),
    ("gamma", 1000): (0.007, 0.017, 0.013),
    # half of these series' values are exact zeros: the 0.025 quantile is the atom itself, P² puts its marker a hair above it
    # (measured: at most 3.9e-9 above at n = 200, 3.4e-31 at n = 1000) and the rank of such a point says nothing; that
    # probability is held by value below instead
    ("masked", 200): (None, 0.125, 0.105),
    ("masked", 1000): (None, 0.044, 0.025),
}
MASKED_LOW_VALUE = {200: 3.93e-9, 1000: 3.5e-31}


@pytest.fixture(scope="module")
def series():
    s = ref.prototype_series(1000)
    gamma = np.random.default_rng(5).gamma(0.7, 2.0, (1000, 1000))
    return {"masked": s[:, :1000], "plain": s[:, 1000:2000], "gamma": gamma, "all": s}


@pytest.mark.parametrize("n", [200, 1000])
def test_rank_error_against_the_stored_series(series, n):
    for group in ("plain", "gamma", "masked"):
        x = series[group][:n]
        p2 = ref.feed(PROBS, x)
        p2.check_invariants()
        est = p2.values()
        err = ref.rank_error(x, est, PROBS).max(axis=1)
        val = np.abs(est - np.quantile(x, PROBS, axis=0)).max(axis=1)
        print(f"{group} n = {n}: worst rank error {err}, worst |q̂ − np.quantile| {val}")
        for j, m in enumerate(MEASURED[group, n]):
            if m is not None:
                assert err[j] <= 2.0 * m, (group, n, PROBS[j], err[j])
        if group == "masked":
            assert np.all(np.quantile(x, PROBS[0], axis=0) == 0.0)
            assert 0.0 <= est[0].min() and est[0].max() <= 2.0 * MASKED_LOW_VALUE[n]
        assert np.array_equal(p2.min(), x.min(axis=0)) and np.array_equal(p2.max(), x.max(axis=0))


@pytest.mark.parametrize("probs", [(0.5,), PROBS, (0.05, 0.25, 0.75, 0.95)])
def test_invariants_with_ties_zeros_and_a_constant(series, probs):
    rng = np.random.default_rng(9)
    x = series["all"][:300, ::20].copy()                       # masked and plain entries and the constant (the last)
    x = np.concatenate([x, rng.integers(0, 4, (300, 30)) / 4.0], axis=1)        # heavy ties: four values
    x[:, 3] = x[:, 2]                                          # two entries with one history
    p2 = ref.P2(probs, x.shape[1])
    K = 2 * len(probs) + 3
    for t, row in enumerate(x):
        p2.add(row)
        p2.check_invariants()
        assert p2.n == t + 1
        assert np.array_equal(p2.min(), x[:t + 1].min(axis=0)) and np.array_equal(p2.max(), x[:t + 1].max(axis=0))
        v = p2.values()
        assert v.shape == (len(probs), x.shape[1])
        if t + 1 < K:
            assert np.all(np.isnan(v))
        else:
            assert np.all(v >= p2.min()) and np.all(v <= p2.max()) and np.all(np.diff(v, axis=0) >= 0.0)
        if t + 1 == K:                                         # the warm-up ends on the sorted first K values
            assert np.array_equal(p2.q, np.sort(x[:K], axis=0))
    const = x.shape[1] - 31
    assert np.all(x[:, const] == 0.375) and np.all(p2.values()[:, const] == 0.375)
    assert np.array_equal(p2.values()[:, 2], p2.values()[:, 3])
    assert np.array_equal(ref.marker_probs(probs)[2:-1:2], probs)


def test_every_takes_every_kth_row(series):
    x = series["plain"][:90, :50]
    assert np.array_equal(ref.feed(PROBS, x, every=3).values(), ref.feed(PROBS, x[::3]).values())
    assert ref.feed(PROBS, x, every=3).n == 30


def test_interval_picks_its_rows(nhp):
    v = np.arange(12.0).reshape(3, 4)
    q = nhp.ChainQuantiles(PROBS, v, v[0] - 1, v[2] + 1, 50, 2)
    lo, hi = q.interval(0.95)
    assert np.array_equal(lo, v[0]) and np.array_equal(hi, v[2]) and q.n == 50 and q.every == 2
    with pytest.raises(ValueError, match="0.05"):
        q.interval(0.9)
    with pytest.raises(ValueError):
        q.interval(1.0)


def test_quantile_arguments_are_checked_before_the_library_is_touched(nhp, monkeypatch):
    from nhp_amd import _lib
    from helpers import random_case

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "default_context", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    c = random_case(3, 50, 10.0, "exponential", 1.0, nhp=nhp)
    run = lambda **kw: nhp.mcmc_(c["proc"], c["data"], nsteps=4, **kw)
    with pytest.raises(ValueError, match="moments"):
        run(quantiles=True)
    for bad in ((0.5, 0.5), (0.9, 0.1), (0.0, 0.5), (0.5, 1.0), (), (np.nan,), "median", ((0.1, 0.2),)):
        with pytest.raises(ValueError):
            run(quantiles=bad, moments=True)
    with pytest.raises(ValueError, match="at most 4"):
        run(quantiles=(0.1, 0.2, 0.3, 0.4, 0.5), moments=True)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="quantiles_every"):
            run(quantiles=True, moments=True, quantiles_every=bad)
    with pytest.raises(NotImplementedError, match="device_draws=True"):
        run(quantiles=True, moments=True, device_draws=False)
    # the discrete driver takes the same arguments and checks them the same way
    N, B = 3, 2
    dp = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), 1.0),
                                           nhp.DiscreteGaussianImpulseResponse(np.full((N, N, B), 1.0 / B), 4, 1.0),
                                           nhp.DenseWeightModel(np.full((N, N), 0.1)), 1.0)
    counts = np.ones((N, 40), dtype=np.int64)
    with pytest.raises(ValueError, match="moments"):
        nhp.mcmc_(dp, counts, nsteps=4, quantiles=True)
    with pytest.raises(ValueError, match="at most 4"):
        nhp.mcmc_(dp, counts, nsteps=4, quantiles=(0.1, 0.2, 0.3, 0.4, 0.5), moments=True)
    with pytest.raises(ValueError, match="strictly"):
        nhp.mcmc_(dp, counts, nsteps=4, quantiles=(0.6, 0.4), moments=True)
    with pytest.raises(NotImplementedError, match="device_draws=False"):
        nhp.mcmc_(dp, counts, nsteps=4, quantiles=True, moments=True, device_draws=False)
