"""The continuous variational fit's definition, checked without a GPU: the numpy/scipy restatement (tests/vb_ref.py) raises its
ELBO at every step, its normal-gamma KL is the integral it stands for, ContinuousVariational's summaries are scipy's, and the
argument errors are raised (and discrete processes still dispatched to the discrete driver) before any device work."""
import numpy as np
import pytest
from scipy import integrate, stats

import em_ref as er
import vb_ref as vr
from helpers import random_case

PRIORS = dict(alpha0=2.0, beta0=1.5, kappa=1.5, nu=2.0, a=2.0, b=0.7, mu_mu=-0.5, kappa_mu=2.0)


@pytest.mark.parametrize("kind,dt_max,recursive", [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)])
def test_restated_elbo_never_falls(nhp, kind, dt_max, recursive):
    """30 restated updates from a random guess.  Coordinate ascent guarantees L_{k+1} >= L_k in exact arithmetic; the sums are
    math.fsum, so what is left is the rounding of the ~1e3 terms' own evaluation: 1e-11·max(1, |L|), the bound of the EM trace."""
    N = 4
    c = random_case(N, 400, 40.0, kind, dt_max, seed=11, nhp=nhp)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive)
    guess = er.from_vector(np.random.default_rng(3).uniform(0.2, 0.8, len(c["proc"].params())), N, kind, dt_max)
    state, trace = vr.run(guess, pr, PRIORS, 30)
    assert len(trace) == 30 and np.all(np.isfinite(trace))
    rise = np.diff(trace)
    print(f"{kind} dt_max={dt_max} recursive={recursive}: L {trace[0]:.4f} -> {trace[-1]:.6f}, smallest rise {rise.min():.3e}")
    assert rise.min() >= -1e-11 * max(1.0, abs(trace[-1]))
    assert trace[-1] > trace[0]
    # the trace's last value is the ELBO of the state returned, and the planes round-trip
    assert trace[-1] == pytest.approx(vr.elbo(state, pr, PRIORS, dt_max), rel=1e-13)
    S, R = vr.planes(state)
    back = vr.from_planes(S, R, N, kind)
    assert all(np.array_equal(back[k], state[k]) for k in state)


def test_an_update_without_events_returns_the_prior_plus_exposure(nhp):
    """M = 0: bg = EM = S1 = S2 = 0, cnt = 0 -- every factor is its prior, but for the baseline's rate β0 + T."""
    for kind in ("exponential", "logitnormal"):
        N = 3
        c = random_case(N, 5, 10.0, kind, 1.0, seed=2, nhp=nhp)
        pr = er.Pairs(c["times"][:0], c["nodes"][:0], c["T"], N, 1.0)
        state, ll, _ = vr.step(er.Model.of(c["proc"]), pr, PRIORS)
        assert ll == 0.0
        assert np.all(state["alpha"] == 2.0) and np.all(state["beta"] == 11.5)
        assert np.all(state["kappa"] == 1.5) and np.all(state["nu"] == 2.0) and np.all(state["a"] == 2.0)
        assert np.allclose(state["b"], 0.7, rtol=1e-15)
        if kind == "logitnormal":
            assert np.all(state["k"] == 2.0) and np.allclose(state["m"], -0.5, rtol=1e-15)
        comp, kl0, klw, kli = vr.pieces(state, pr.cnt, pr.T, PRIORS)
        assert comp == pytest.approx(N * 10.0 * 2.0 / 11.5, rel=1e-14) and abs(klw) < 1e-14 and abs(kli) < 1e-13 and kl0 > 0


def test_normal_gamma_kl_against_quadrature():
    """KL(NormalGamma(m, k, a, b) ‖ NormalGamma(μμ, κμ, a0, b0)) = ∫∫ q log(q/p) dμ dτ, by scipy's dblquad."""
    def logpdf(mu, tau, m, k, a, b):
        return stats.gamma.logpdf(tau, a, scale=1.0 / b) + stats.norm.logpdf(mu, m, 1.0 / np.sqrt(k * tau))
    for (m, k, a, b), (m0, k0, a0, b0) in (((0.3, 5.5, 4.0, 2.5), (-0.5, 2.0, 2.0, 0.7)), ((-1.2, 2.25, 2.6, 0.9), (0.0, 1.0, 1.0, 1.0))):
        def f(mu, tau):
            lq = logpdf(mu, tau, m, k, a, b)
            return np.exp(lq) * (lq - logpdf(mu, tau, m0, k0, a0, b0))
        num, err = integrate.dblquad(f, 1e-9, 40.0, lambda t: m - 12.0 / np.sqrt(k * t) - 1.0, lambda t: m + 12.0 / np.sqrt(k * t) + 1.0,
                                     epsabs=1e-10, epsrel=1e-10)
        want = float(vr.kl_normal_gamma(m, k, a, b, m0, k0, a0, b0))
        print(f"normal-gamma KL: closed form {want:.9f}, quadrature {num:.9f} (± {err:.1e})")
        assert abs(num - want) <= 1e-6


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_summaries_agree_with_scipy(nhp, kind):
    N = 3
    st = vr.random_state(N, kind, seed=5)
    st["a"][0, 1] = 0.8                                        # a' <= 1: the Student-t marginal of μ has no variance
    S, R = vr.planes(st)
    res = nhp.ContinuousVariational(kind, N, S, R, prior_kappa=0.05)
    f = lambda v: v.ravel(order="F")
    g = [(st["alpha"], st["beta"])] + ([(f(st["a"]), f(st["b"]))] if kind == "exponential" else [None, (f(st["a"]), f(st["b"]))]) \
        + [(f(st["kappa"]), f(st["nu"]))]
    mean, sd, lo, hi = [], [], [], []
    for blk in g:
        if blk is None:                                        # μ ~ Student-t(2a', m', sqrt(b'/(a' k')))
            a, b, m, k = f(st["a"]), f(st["b"]), f(st["m"]), f(st["k"])
            d = stats.t(2.0 * a, loc=m, scale=np.sqrt(b / (a * k)))
            mean.append(m); sd.append(np.where(a > 1.0, d.std(), np.inf)); lo.append(d.ppf(0.05)); hi.append(d.ppf(0.95))
            continue
        d = stats.gamma(blk[0], scale=1.0 / blk[1])
        mean.append(d.mean()); sd.append(d.std()); lo.append(d.ppf(0.05)); hi.append(d.ppf(0.95))
    got_lo, got_hi = res.interval(0.90)
    for got, want in ((res.mean(), mean), (res.sd(), sd), (got_lo, lo), (got_hi, hi)):
        want = np.concatenate(want)
        assert got.shape == want.shape
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin) and np.allclose(got[fin], want[fin], rtol=1e-12, atol=0.0)
    if kind == "logitnormal":
        assert np.isinf(res.sd()[N + 1 * N + 0])               # μ[0, 1], column-major
    assert np.array_equal(res.expected_links(), st["kappa"] - 0.05)
    assert np.array_equal(res.kappa, st["kappa"]) and np.array_equal(res.b, st["b"]) and np.array_equal(res.beta, st["beta"])
    assert (res.m is None) == (kind == "exponential")
    with pytest.raises(ValueError):
        res.interval(1.0)
    with pytest.raises(ValueError, match="Parameter vector length"):
        nhp.ContinuousVariational(kind, N, S[:-1], R[:-1])


def test_argument_errors_are_raised_before_any_device_work(nhp):
    """Network process: TypeError; LGCP baseline and ShardedDataset: NotImplementedError; a guess of the wrong length, a
    non-positive hyper-parameter, a state of the other family: ValueError -- none of them touches a device."""
    std = random_case(3, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    net = random_case(3, 50, 10.0, "exponential", 1.0, network=True, seed=1, nhp=nhp)
    lgcp = random_case(3, 50, 10.0, "exponential", 1.0, lgcp=True, seed=1, nhp=nhp)
    shard = object.__new__(nhp.ShardedDataset)
    for fn in (nhp.vb_, nhp.update_):
        with pytest.raises(TypeError):
            fn(net["proc"], net["data"])
        with pytest.raises(NotImplementedError):
            fn(lgcp["proc"], lgcp["data"])
        with pytest.raises(NotImplementedError):
            fn(std["proc"], shard)
    with pytest.raises(ValueError, match="Parameter vector length"):
        nhp.vb_(std["proc"], std["data"], guess=np.full(7, 0.5))
    other = nhp.ContinuousVariational("logitnormal", 3, *vr.planes(vr.random_state(3, "logitnormal", 1)))
    for fn in (nhp.vb_, nhp.update_):
        with pytest.raises(ValueError, match="Parameter vector length"):
            fn(std["proc"], std["data"], init=other)
        with pytest.raises(TypeError):
            fn(std["proc"], std["data"], init=np.ones(21))
    with pytest.raises(ValueError):
        nhp.vb_(std["proc"], std["data"], max_steps=0)
    std["proc"].weights.κ = 0.0
    for fn in (nhp.vb_, nhp.update_):
        with pytest.raises(ValueError, match="kappa"):
            fn(std["proc"], std["data"])


def test_discrete_processes_still_reach_the_discrete_drivers(nhp, monkeypatch):
    """nhp.vb_ / nhp.update_ are dispatchers now: a discrete process goes to discrete.vb_ / discrete.update_ with its arguments
    untouched, and the discrete driver's own refusal (sparse weights on a standard process) still comes through."""
    from nhp_amd import discrete
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.ones(3), 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(np.full((3, 3, 2), 0.5), 4, 1.0),
                                             nhp.SparseWeightModel(np.full((3, 3), 0.1)), 1.0)
    data = np.zeros((3, 10), dtype=np.int64)
    with pytest.raises(NotImplementedError, match="vb!"):
        nhp.vb_(proc, data, max_steps=1)
    with pytest.raises(NotImplementedError, match="update!"):
        nhp.update_(proc, data, None)
    seen = []
    monkeypatch.setattr(discrete, "vb_", lambda *a, **k: seen.append(("vb", a, k)) or "vb")
    monkeypatch.setattr(discrete, "update_", lambda *a, **k: seen.append(("update", a, k)) or "update")
    assert nhp.vb_(proc, data, 7, keep_trace=False) == "vb" and nhp.update_(proc, data, None, n_steps=2) == "update"
    assert seen[0][0] == "vb" and seen[0][1][0] is proc and seen[0][1][2] == 7 and seen[0][2] == {"keep_trace": False}
    assert seen[1][0] == "update" and seen[1][1][2] is None and seen[1][2] == {"n_steps": 2}
