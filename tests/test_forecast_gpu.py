"""forecast(process, data, horizon) on the device: nhp_cont_forecast (csrc/cont_forecast.hip).

The output contract, determinism, the deterministic carry against its numpy restatement, an exact replay of the
documented counter scheme (tests/forecast_ref.py, part b), the closed forms of a bipartite model, a general model against
the numpy ensemble (part a), the degenerate cases and the round trip into loglikelihood / compensator.  Statistical bounds:
4.5 standard errors at fixed seeds, Kolmogorov-Smirnov and χ² at p > 1e-4 (the rules of test_simulate_gpu.py)."""
import math

import numpy as np
import pytest

import forecast_ref as fr
from test_forecast_host import bipartite, sink_means
from test_simulate_gpu import KS_CRIT, _chi2_ok, _ks_two, _ks_uniform, make, small

pytestmark = pytest.mark.gpu


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def history(nhp, proc, T0, seed=2):
    t, n, T = nhp.rand(proc, T0, seed=seed)
    return np.asarray(t, float), np.asarray(n, np.int64), T


def same_forecast(a, b, paths=True):
    ok = np.array_equal(host(a.counts), host(b.counts)) and np.array_equal(host(a.carry), host(b.carry))
    if paths:
        ok = ok and all(np.array_equal(host(x), host(y)) for x, y in zip(a.paths, b.paths))
    return ok


# ---- contract ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,network", [("exponential", False), ("logit-normal", True)])
def test_output_contract(nhp, kind, network):
    import torch
    ctx = nhp.default_context()
    proc = small(nhp, N=5, kind=kind, network=network, scale=0.25)
    t, n, T0 = history(nhp, proc, 100.0)
    assert 300 <= len(t) <= 2000
    N, S, h = 5, 50, 2.0
    f = nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=3, return_paths=True)
    counts, carry, (pt, pn, off) = f
    assert counts.shape == (S, N) and counts.dtype == np.int64 and carry.shape == (N,) and carry.dtype == np.float64
    assert pt.dtype == np.float64 and pn.dtype == np.int64 and off.dtype == np.int64 and off.shape == (S + 1,)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(pt) == len(pn) == counts.sum()
    assert 10 <= counts.sum(axis=1).mean() <= 30
    assert np.all(pt > T0) and np.all(pt <= T0 + h) and pn.min() >= 1 and pn.max() <= N
    for r in range(S):
        rt, rn = f.path(r)
        assert np.all(np.diff(rt) >= 0)
        assert np.array_equal(np.bincount(rn - 1, minlength=N), counts[r])
    assert np.all(carry > 0.0)
    # the device route: torch tensors on the context's device, the same values
    d = nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=3, return_paths=True, device=True)
    for x, dt in ((d.counts, torch.int64), (d.carry, torch.float64), (d.paths[0], torch.float64), (d.paths[1], torch.int64),
                  (d.paths[2], torch.int64)):
        assert x.dtype == dt and x.device.type == "cuda" and x.device.index == ctx.device
    assert same_forecast(f, d)
    # without paths: the same counts
    assert same_forecast(f, nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=3), paths=False)
    # a device-built dataset and a dataset given as device tensors
    dmax = float(proc.impulses.Δtmax)
    built = nhp.DeviceDataset(ctx, (t, n, T0), N, dmax, build="device")
    assert same_forecast(f, nhp.forecast(proc, built, h, nsamples=S, seed=3, return_paths=True))
    dev = torch.device("cuda", ctx.device)
    tensors = (torch.as_tensor(t, device=dev), torch.as_tensor(n, device=dev), T0)
    assert same_forecast(f, nhp.forecast(proc, tensors, h, nsamples=S, seed=3, return_paths=True))


# ---- determinism ------------------------------------------------------------------------------------------------------

def test_same_arguments_same_bits_other_seed_other_sample(nhp):
    proc = small(nhp, N=6, kind="logit-normal", network=True, seed=4, scale=0.25)
    data = history(nhp, proc, 150.0)
    kw = dict(nsamples=200, return_paths=True)
    a = nhp.forecast(proc, data, 3.0, seed=7, **kw)
    assert same_forecast(a, nhp.forecast(proc, data, 3.0, seed=7, **kw))
    n = int(a.counts.sum())
    for cap in (n, n + 1, 3 * n + 17):                           # any capacity that suffices
        assert same_forecast(a, nhp.forecast(proc, data, 3.0, seed=7, max_events=cap, **kw))
    assert not same_forecast(a, nhp.forecast(proc, data, 3.0, seed=8, **kw))
    e = small(nhp, N=6, kind="exponential", seed=4, scale=0.25)
    b = nhp.forecast(e, data, 3.0, seed=7, **kw)
    assert same_forecast(b, nhp.forecast(e, data, 3.0, seed=7, max_events=int(b.counts.sum()), **kw))


# ---- carry ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
@pytest.mark.parametrize("network", [False, True])
def test_carry_matches_the_restatement(nhp, kind, network):
    proc = small(nhp, N=6, kind=kind, network=network, seed=9, scale=0.2, dt_max=4.0)
    t, n, T0 = history(nhp, proc, 80.0)
    assert 300 <= len(t) <= 2000
    h = 2.5
    got = nhp.forecast(proc, (t, n, T0), h, nsamples=1, seed=0).carry
    want = fr.carry_expected(proc, t, n, T0, h)
    err = np.max(np.abs(got - want) / want)
    print(f"{kind} network={network}: carry {want}, max rel err {err:.2e}")
    assert np.all(want > 0.0) and err <= 1e-11


def test_carry_is_zero_without_weights_and_past_the_window(nhp):
    proc = small(nhp, N=4, kind="logit-normal", seed=1, dt_max=1.5)
    t, n, T0 = history(nhp, proc, 100.0)
    late = nhp.forecast(proc, (t, n, t[-1] + 2.0), 3.0, nsamples=5, seed=1)       # the history ends more than Δtmax before T0
    assert np.all(late.carry == 0.0)
    for kind in ("exponential", "logit-normal"):
        p = small(nhp, N=4, kind=kind, seed=1, dt_max=1.5)
        mute = make(nhp, p.baseline.λ, np.zeros((4, 4)), kind, theta=np.ones((4, 4)), mu=np.zeros((4, 4)), tau=np.ones((4, 4)), dt_max=1.5)
        assert np.all(nhp.forecast(mute, (t, n, T0), 3.0, nsamples=5, seed=1).carry == 0.0)


# ---- exact replay of the counter scheme (include/nhp.h) ----------------------------------------------------------------

@pytest.mark.parametrize("kind,network", [("exponential", True), ("logit-normal", True), ("exponential", False)])
def test_numpy_replay_reproduces_the_call(nhp, kind, network):
    W = np.array([[0.20, 0.30, 0.10], [0.25, 0.15, 0.20], [0.10, 0.30, 0.20]])
    A = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]]) if network else None
    proc = make(nhp, [1.0, 0.8, 1.2], W, kind, theta=[[1.0, 2.0, 3.0], [1.5, 2.5, 1.2], [2.2, 1.1, 1.7]],
                mu=[[0.3, -0.5, 1.0], [-1.0, 0.0, 0.5], [0.7, -0.2, -0.8]], tau=[[1.0, 0.5, 2.0], [1.5, 0.8, 1.2], [0.6, 1.9, 1.0]],
                A=A, dt_max=1.5)
    t, n, T0 = history(nhp, proc, 80.0)
    assert len(t) >= 300
    S, h, seed = 3, 4.0, 20261017
    wc, wt, wn, wo = fr.replay(proc, t, n, T0, h, S, seed)
    assert 10 <= wc.sum() / S <= 30
    counts, carry, (pt, pn, off) = nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=seed, return_paths=True)
    assert np.array_equal(counts, wc) and np.array_equal(off, wo) and np.array_equal(pn, wn)
    assert np.allclose(pt, wt, rtol=1e-12, atol=0.0)


# ---- laws -------------------------------------------------------------------------------------------------------------

def _poisson_chi2(x, lam):
    """The counts x against Poisson(lam): bins pooled at both tails until each expects at least 5."""
    S, kmax = len(x), int(max(x.max(), lam + 10 * math.sqrt(lam))) + 1
    k = np.arange(kmax + 1)
    pmf = np.exp(k * math.log(lam) - lam - np.array([math.lgamma(v + 1.0) for v in k]))
    cdf = np.cumsum(pmf)
    lo = int(np.argmax(S * cdf >= 5.0))
    hi = int(len(k) - 1 - np.argmax((S * (1.0 - np.concatenate([[0.0], cdf[:-1]])))[::-1] >= 5.0))
    obs = np.bincount(np.clip(x, lo, hi) - lo, minlength=hi - lo + 1).astype(float)
    exp = S * np.concatenate([[cdf[lo]], pmf[lo + 1:hi], [1.0 - cdf[hi - 1]]])
    return _chi2_ok(obs, exp)


@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_bipartite_closed_forms(nhp, kind):
    proc, t, n, T0 = bipartite(nhp, kind)
    S, h = 4000, 6.0
    counts = nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=11).counts
    lam0 = np.asarray(proc.baseline.λ)
    mean, se = counts.mean(axis=0), counts.std(axis=0, ddof=1) / math.sqrt(S)
    want, _ = sink_means(proc, t, n, T0, h)
    z_src, z_snk = (mean[:2] - lam0[:2] * h) / se[:2], (mean[2:] - want) / se[2:]
    print(f"{kind}: sink means {mean[2:]} vs {want}, z sources {z_src}, sinks {z_snk}")
    assert np.all(np.abs(z_src) < 4.5) and np.all(np.abs(z_snk) < 4.5)
    for p in (0, 1):
        assert _poisson_chi2(counts[:, p], lam0[p] * h), p


def test_carry_over_delays_of_a_one_link_model(nhp):
    # no baseline and one link 1 -> 2: every forecast event is a carry-over child on node 2, its delay Exp(θ) given <= h
    theta, h, S = 0.4, 3.0, 800
    proc = make(nhp, [0.0, 0.0], [[0.0, 0.7], [0.0, 0.0]], theta=np.full((2, 2), theta))
    r = np.random.default_rng(6)
    t, n, T0 = np.sort(r.uniform(0.0, 100.0, 300)), np.ones(300, np.int64), 100.0
    counts, carry, (pt, pn, off) = nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=13, return_paths=True)
    assert np.all(pn == 2) and np.all(counts[:, 0] == 0) and carry[0] == 0.0
    assert len(pt) > 2000 and abs(len(pt) - S * carry[1]) < 4.5 * math.sqrt(S * carry[1])
    u = -np.expm1(-theta * (pt - T0)) / -math.expm1(-theta * h)
    assert _ks_uniform(u) < KS_CRIT


@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_general_model_against_the_numpy_ensemble(nhp, kind):
    proc = small(nhp, N=5, kind=kind, network=True, seed=8, scale=0.4, dt_max=2.0)       # spectral radius 0.74: several generations
    t, n, T0 = history(nhp, proc, 70.0)
    assert 300 <= len(t) <= 2000
    S, h = 4000, 1.5
    dev = nhp.forecast(proc, (t, n, T0), h, nsamples=S, seed=17).counts
    ref = fr.ensemble(proc, t, n, T0, h, S, seed=18)
    assert 10 <= ref.sum(axis=1).mean() <= 30
    z = (dev.mean(axis=0) - ref.mean(axis=0)) / np.sqrt((dev.var(axis=0, ddof=1) + ref.var(axis=0, ddof=1)) / S)
    ks = _ks_two(dev.sum(axis=1).astype(float), ref.sum(axis=1).astype(float))
    print(f"{kind}: means {dev.mean(axis=0)} vs {ref.mean(axis=0)}, z {z}, KS of totals {ks:.3f}")
    assert np.all(np.abs(z) < 4.5) and ks < KS_CRIT


# ---- degenerate cases -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_degenerate_cases(nhp, kind):
    proc = small(nhp, N=4, kind=kind, seed=2)
    t, n, T0 = history(nhp, proc, 100.0)
    N = 4
    # horizon 0: zeros and empty paths
    z = nhp.forecast(proc, (t, n, T0), 0.0, nsamples=7, seed=1, return_paths=True)
    assert z.counts.shape == (7, N) and not z.counts.any() and not z.carry.any()
    assert len(z.paths[0]) == len(z.paths[1]) == 0 and np.array_equal(z.paths[2], np.zeros(8, np.int64))
    # an empty history: immigrants and their descendants only
    S, h = 500, 3.0
    e = nhp.forecast(proc, (np.empty(0), np.empty(0, np.int64), 50.0), h, nsamples=S, seed=1, return_paths=True)
    assert not e.carry.any() and np.all(e.paths[0] > 50.0) and np.all(e.paths[0] <= 50.0 + h)
    lam0 = np.asarray(proc.baseline.λ)
    assert np.all(e.counts.mean(axis=0) >= lam0 * h - 4.5 * np.sqrt(lam0 * h / S))       # at least the immigrants
    # one replica
    one = nhp.forecast(proc, (t, n, T0), h, nsamples=1, seed=1, return_paths=True)
    assert one.counts.shape == (1, N) and np.array_equal(one.paths[2], [0, one.counts.sum()])
    assert np.all(np.diff(one.paths[0]) >= 0) and np.array_equal(np.bincount(one.paths[1] - 1, minlength=N), one.counts[0])


def test_explosion_is_an_error_and_the_context_stays_usable(nhp):
    hot = make(nhp, [1.0, 1.0, 1.0], 0.8 * np.ones((3, 3)), theta=np.ones((3, 3)))        # spectral radius 2.4
    r = np.random.default_rng(3)
    data = (np.sort(r.uniform(0.0, 50.0, 300)), r.integers(1, 4, 300), 50.0)
    with pytest.raises(RuntimeError, match="exploded"):
        nhp.forecast(hot, data, 100.0, nsamples=2, seed=1, max_events=20_000, return_paths=True)
    with pytest.raises(RuntimeError, match="exploded"):                                  # the roots alone overflow
        nhp.forecast(hot, data, 100.0, nsamples=2, seed=1, max_events=100)
    proc = small(nhp, N=3, seed=3)
    f = nhp.forecast(proc, data, 3.0, nsamples=100, seed=2, return_paths=True)
    assert f.counts.sum() > 500 and f.paths[2][-1] == f.counts.sum()


# ---- round trip -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_history_plus_a_path_is_data(nhp, kind):
    import torch
    proc = small(nhp, N=4, kind=kind, seed=5)
    t, n, T0 = history(nhp, proc, 150.0)
    h = 5.0
    f = nhp.forecast(proc, (t, n, T0), h, nsamples=4, seed=9, return_paths=True)
    pt, pn = f.path(2)
    assert len(pt) > 5
    data = (np.concatenate([t, pt]), np.concatenate([n, pn]), T0 + h)
    ll = nhp.loglikelihood(proc, data, recursive=False)
    comp = nhp.compensator(proc, data)
    assert np.isfinite(ll) and np.all(np.isfinite(comp.total)) and np.all(comp.residuals >= 0.0)
    # the same on the device route
    ctx = nhp.default_context()
    dev = torch.device("cuda", ctx.device)
    d = nhp.forecast(proc, (t, n, T0), h, nsamples=4, seed=9, return_paths=True, device=True)
    dt_, dn = d.path(2)
    ddata = (torch.cat([torch.as_tensor(t, device=dev), dt_]), torch.cat([torch.as_tensor(n, device=dev), dn]), T0 + h)
    ll_dev = nhp.loglikelihood(proc, ddata, recursive=False)
    assert abs(ll_dev - ll) <= 1e-12 * abs(ll)
