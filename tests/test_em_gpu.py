"""GPU tests of the EM fit (csrc/cont_em.hip): expected_statistics against the numpy restatement (tests/em_ref.py) and
against the library's own gradient, em_ against the restated M-step, the fit against the project's "this is a maximum"
criteria (tests/test_cont_inference_gpu.py), the MAP fit, and rand -> em_ -> time_rescaling_test on the device."""
import importlib
import os
import sys

import numpy as np
import pytest

import em_ref as er
from helpers import random_case

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

TOL = 1e-10          # |got - want| <= TOL·max(1, |want|) per entry: the bound the gradient holds for the same sums
TOL_LL = 1e-11


def _check(got, want, what):
    """Every statistic within its bound; returns the largest ratio of an error to its bound."""
    assert abs(got.ll - want[0]) <= TOL_LL * max(1.0, abs(want[0])), (what, got.ll, want[0])
    worst = abs(got.ll - want[0]) / (TOL_LL * max(1.0, abs(want[0])))
    for name, g, w in zip(("bg", "EM", "S1", "S2"), got[1:], want[1:]):
        if w is None:
            assert g is None, (what, name)
            continue
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        ratio = float(np.max(np.abs(g - w) / (TOL * np.maximum(1.0, np.abs(w))))) if w.size else 0.0
        print(f"{what} {name}: largest error / bound = {ratio:.3e}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, name, ratio)
    return worst


def _want(proc, data, recursive, exact=True):
    m = er.Model.of(proc)
    pr = er.Pairs(data[0], data[1], data[2], m.N, m.dt_max, recursive=recursive and m.theta is not None)
    return er.statistics(m, pr, exact), pr, m


def _routes(monkeypatch, nhp, proc, data, chunk="4096"):
    """The one-launch slices route (the default where it applies) and the two-pass route, as tests/test_cont_inference_gpu.py
    switches between them.  The one-launch route needs a dataset that keeps its child slices: with the default items of 32
    children the datasets of these tests drop them (half-empty slices; tests/slices_ref.py restates the rule), so the
    "default" leg builds its dataset with items of 4096 children.  After each leg the scalars of the dataset it ran on say
    which layout that was: slices where Δtmax is finite on the "default" leg, none on the two-pass leg.  chunk=None keeps the
    default items on both legs: no slices on either."""
    sliceable = chunk is not None and bool(np.isfinite(proc.impulses.Δtmax))
    for name, env in (("default", {"NHP_CHUNK": chunk} if chunk else {}), ("two-pass", {"NHP_GRAD_SLICES": "0"})):
        for k in ("NHP_GRAD_SLICES", "NHP_CHUNK"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        nhp.invalidate_device_datasets()
        yield name
        rows = nhp.device_dataset(proc, data).scalars()["sl_rows"]
        assert (rows > 0) == (name == "default" and sliceable), (name, rows)
    for k in ("NHP_GRAD_SLICES", "NHP_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    nhp.invalidate_device_datasets()


CASES = [("exponential", 0.5, False), ("exponential", 1.5, False), ("exponential", np.inf, False), ("exponential", np.inf, True),
         ("exponential", 1.5, True), ("logitnormal", 0.5, False), ("logitnormal", 1.5, False)]


@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_statistics_match_the_restatement(nhp, kind, dt_max, recursive, monkeypatch):
    case = random_case(7, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    want, pr, _ = _want(case["proc"], case["data"], recursive)
    for route in _routes(monkeypatch, nhp, case["proc"], case["data"]):
        got = nhp.expected_statistics(case["proc"], case["data"], recursive=recursive)
        _check(got, want, f"{kind} dt_max={dt_max} recursive={recursive} {route}")
        total = got.EM.sum(axis=0) + got.bg
        assert np.max(np.abs(total - pr.cnt) / pr.cnt) <= 1e-12 * 10          # (the sums of N + 1 rounded statistics)
    # device tensors in, device tensors out
    import torch
    ctx = nhp.default_context()
    dev = torch.device("cuda", ctx.device)
    tens = (torch.as_tensor(case["times"]).to(dev), torch.as_tensor(case["nodes"]).to(dev), case["T"])
    out = nhp.expected_statistics(case["proc"], tens, recursive=recursive, device=True)
    assert all(o.is_cuda and o.dtype == torch.float64 for o in out[1:] if o is not None)
    _check(out, want, f"{kind} dt_max={dt_max} recursive={recursive} device tensors")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_statistics_with_most_weights_on_the_lower_bound(nhp, kind, monkeypatch):
    """Three quarters of W at 1e-6: the statistics of those links are ~1e-6 of the others' and must still be right to the
    same bound -- nothing in the E-step divides by W."""
    case = random_case(7, 1500, 80.0, kind, 1.5, seed=4, nhp=nhp)
    W = case["proc"].weights.W
    W[np.random.default_rng(0).uniform(size=W.shape) < 0.75] = 1e-6
    assert (W == 1e-6).sum() >= 30
    want, _, _ = _want(case["proc"], case["data"], False)
    small = want[2][W == 1e-6]
    assert np.all(small > 0) and np.max(small) < 1e-2
    for route in _routes(monkeypatch, nhp, case["proc"], case["data"]):
        got = nhp.expected_statistics(case["proc"], case["data"], recursive=False)
        _check(got, want, f"{kind} sparse W {route}")
        # relative to the small entries themselves: the error bound of EM = W·(g_W + cnt_p) is cnt_p·ε·W
        rel = np.max(np.abs(got.EM[W == 1e-6] - small) / small)
        print(f"{kind} sparse W {route}: largest relative error of the EM of a link on the bound {rel:.2e}")
        assert rel <= 1e-9


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_statistics_of_20000_events(nhp, kind, monkeypatch):
    case = random_case(5, 20000, 2500.0, kind, 1.0, seed=12, nhp=nhp)
    want, _, _ = _want(case["proc"], case["data"], False)
    for route in _routes(monkeypatch, nhp, case["proc"], case["data"]):
        _check(nhp.expected_statistics(case["proc"], case["data"], recursive=False), want, f"{kind} M=20000 {route}")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_ties_and_a_node_without_events(nhp, kind, monkeypatch):
    """Every delay of this dataset is 0.  It stays on the default items, without child slices, and asserts so: the 6-byte slice
    records keep a delay of 0 as one step of 2^-45·Δtmax (0 marks padding), and over the 7 344 pairs here that alone puts
    S1 of the exponential kind at 1.27 times this file's bound (measured on the same data built with items of 4096; the other
    statistics hold).  The records' delay step is held to its own bound in tests/test_cont_grad_edges_gpu.py."""
    case = random_case(7, 1500, 150.0, kind, 1.0, seed=13, nhp=nhp)
    times = np.round(case["times"])                         # about ten events on each distinct time
    nodes = np.where(case["nodes"] == 4, 5, case["nodes"])  # node 4 has no events
    data = (times, nodes, case["T"])
    want, pr, _ = _want(case["proc"], data, False)
    assert pr.cnt[3] == 0
    for route in _routes(monkeypatch, nhp, case["proc"], data, chunk=None):
        got = nhp.expected_statistics(case["proc"], data, recursive=False)
        _check(got, want, f"{kind} ties {route}")
        assert got.bg[3] == 0.0 and np.all(got.EM[3] == 0.0) and np.all(got.EM[:, 3] == 0.0)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("M", [0, 1])
def test_no_event_and_one_event(nhp, kind, M):
    case = random_case(4, 10, 20.0, kind, 1.0, seed=2, nhp=nhp)
    data = (case["times"][:M], case["nodes"][:M], case["T"])
    for recursive in (False, True):
        want, pr, m = _want(case["proc"], data, recursive)
        _check(nhp.expected_statistics(case["proc"], data, recursive=recursive), want, f"{kind} M={M} recursive={recursive}")
    x0 = case["proc"].params()
    res = nhp.em_(case["proc"], data, guess=x0, max_steps=3, recursive=False)
    new = er.from_vector(res.maximizer, 4, kind, 1.0)
    if M == 0:                                              # λ0 -> the lower bound, the rest unchanged
        assert np.all(new.lam0 == 1e-6) and np.array_equal(res.maximizer[4:], np.clip(x0[4:], 1e-6, 10.0))
    else:
        c = int(data[1][0]) - 1
        assert new.lam0[c] == pytest.approx(1.0 / 20.0, rel=1e-12) and np.all(np.delete(new.lam0, c) == 1e-6)
        assert np.all(new.W[c] == 1e-6)                     # the one event has no children


def _stats_from_gradient(nhp, proc, data, recursive):
    """The statistics through the identities, from the library's own log-likelihood + gradient entry point."""
    ll, g = nhp.loglikelihood_gradient(proc, data, recursive=recursive)
    m = er.Model.of(proc)
    N, T = m.N, data[2]
    cnt = np.bincount(np.asarray(data[1], np.int64) - 1, minlength=N).astype(float)
    mat = [g[N + k * N * N:N + (k + 1) * N * N].reshape((N, N), order="F") for k in range(2 if m.theta is not None else 3)]
    EM = m.W * (mat[-1] + cnt[:, None])
    bg = m.lam0 * (g[:N] + T)
    if m.theta is not None:
        return ll, bg, EM, EM / m.theta - mat[0], None
    return ll, bg, EM, EM * m.mu + mat[0] / m.tau, EM / m.tau - 2.0 * mat[1]


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("N,M", [(64, 100_000), (1024, 1_000_000)])
def test_statistics_against_the_gradient_entry_point(nhp, kind, N, M):
    """Where numpy is not feasible: the same statistics from nhp_cont_loglik_grad (unchanged by this feature) through the
    identities, at N = 64 / M = 1e5 and at the metric size (N = 1024, M = 1e6, mean window 8)."""
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
    proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
    data = (times, nodes, T)
    want = _stats_from_gradient(nhp, proc, data, False)
    got = nhp.expected_statistics(proc, data, recursive=False)
    _check(got, want, f"{kind} N={N} M={M}")
    cnt = np.bincount(nodes - 1, minlength=N)
    live = cnt > 0
    assert np.max(np.abs((got.EM.sum(axis=0) + got.bg - cnt)[live] / cnt[live])) <= 1e-11


@pytest.mark.parametrize("regularize", [False, True])
@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_one_step_is_the_restated_mstep_and_the_trace_never_falls(nhp, kind, dt_max, recursive, regularize):
    N = 7
    def case():
        c = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
        b, w, imp = c["proc"].baseline, c["proc"].weights, c["proc"].impulses
        b.α0, b.β0, w.κ, w.ν = 2.0, 1.5, 1.5, 2.0
        if kind == "exponential":
            imp.α, imp.β = 2.0, 0.7
        else:
            imp.α0, imp.β0, imp.μμ, imp.κμ = 2.0, 0.7, 0.5, 2.0
        return c
    c = case()
    q = er.priors_of(c["proc"]) if regularize else None
    x0 = np.clip(c["proc"].params(), 1e-6, 10.0)            # (the logit-normal μ of random_case has negative entries: clamped)
    m0 = er.from_vector(x0, N, kind, dt_max)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive)
    want = er.params_vector(er.mstep(m0, er.statistics(m0, pr), pr.cnt, pr.T, q))
    one = nhp.em_(c["proc"], c["data"], guess=x0, max_steps=1, recursive=recursive, regularize=regularize, keep_trace=True)
    assert one.steps == 1 and len(one.trace) == 2 and np.array_equal(c["proc"].params(), one.maximizer)
    err = np.max(np.abs(one.maximizer - want) / np.abs(want))
    print(f"{kind} dt_max={dt_max} recursive={recursive} priors={regularize}: one step, largest relative error {err:.2e}")
    assert err <= 1e-10
    on = (want == 1e-6) | (want == 10.0)
    assert np.array_equal(one.maximizer[on], want[on])
    # 200 steps: the objective never falls, and it is ll (+ logprior) at the iterate
    c = case()
    res = nhp.em_(c["proc"], c["data"], guess=x0, max_steps=200, f_abstol=0.0, recursive=recursive, regularize=regularize, keep_trace=True)
    assert res.steps == 200 and len(res.trace) == 201 and res.status == "failure"
    f = res.trace
    drop = np.max((f[:-1] - f[1:]) / np.maximum(1.0, np.abs(f[1:])))
    print(f"  200 steps: {f[0]:.4f} -> {f[-1]:.6f}, largest relative drop {drop:.2e}")
    assert drop <= 1e-11
    assert f[0] == pytest.approx(er.statistics(m0, pr)[0] + (er.logprior(m0, q) if q else 0.0), rel=1e-11)
    # (log-likelihood parity 1e-11 plus the log prior's ~100..200 rounded terms of size <= 15: 2e-11 of |f| ~ 1e3 covers both)
    at_result = nhp.loglikelihood(c["proc"], c["data"], recursive=recursive) + (nhp.logprior(c["proc"]) if regularize else 0.0)
    assert abs(f[-1] - at_result) <= 2e-11 * max(1.0, abs(at_result))
    assert res.maximum == f[-1]


def _set(proc, x):
    proc.params_(x)
    return proc


def _maximum_criteria(nhp, make, data, x, value, recursive, regularize=False, what="", polish_steps=3000, f_abstol=1e-9):
    """The criteria of tests/test_cont_inference_gpu.py::test_device_mle_reaches_a_maximum...: inside the box, the projected
    gradient below 5e-2·scale, the host optimizer started there gains < 1e-3·scale and loses nothing beyond 1e-9·scale."""
    scale = max(1.0, abs(value)) ** 0.5
    assert np.all(x >= 1e-6) and np.all(x <= 10.0)
    proc = _set(make(), x)
    ll, g = nhp.loglikelihood_gradient(proc, data, recursive=recursive)
    if regularize:
        from nhp_amd import inference
        ll, g = ll + nhp.logprior(proc), g + inference._logprior_gradient(proc)
    assert ll == pytest.approx(value, rel=1e-12)
    pg = np.where(((x <= 1e-6) & (g < 0)) | ((x >= 10.0) & (g > 0)), 0.0, g)
    polish = nhp.mle_(make(), data, guess=x, recursive=recursive, regularize=regularize, f_abstol=f_abstol, max_steps=polish_steps)
    gain = polish.maximum - value
    print(f"{what}: value {value:.6f}, max |pg| {np.max(np.abs(pg)):.3e} (bound {5e-2 * scale:.3f}), host polish gains {gain:.3e} "
          f"(bound {1e-3 * scale:.3e}) in {polish.steps} steps")
    assert np.max(np.abs(pg)) < 5e-2 * scale
    assert -1e-9 * scale <= gain < 1e-3 * scale


# (restated iterations on these inputs, tests/test_em_host.py: exponential windowed 5329, logit-normal 1363; the budget is twice that)
@pytest.mark.parametrize("kind,recursive,max_steps", [("exponential", True, 11000), ("exponential", False, 11000),
                                                      ("logitnormal", False, 2700)])
def test_em_reaches_a_maximum(nhp, kind, recursive, max_steps):
    def make():
        return random_case(5, 3000, 250.0, kind, 1.5, seed=31, nhp=nhp)["proc"]
    c = random_case(5, 3000, 250.0, kind, 1.5, seed=31, nhp=nhp)
    guess = np.random.default_rng(5).uniform(0.2, 0.8, len(c["proc"].params()))
    ll0 = nhp.loglikelihood(_set(make(), guess), c["data"], recursive=recursive)
    res = nhp.em_(c["proc"], c["data"], guess=guess, recursive=recursive, f_abstol=1e-9, max_steps=max_steps, keep_trace=True)
    print(f"{kind} recursive={recursive}: EM {res.steps} iterations in {res.elapsed:.3f} s, {ll0:.3f} -> {res.maximum:.6f}")
    assert res.status == "success" and res.maximum > ll0
    assert np.array_equal(c["proc"].params(), res.maximizer)
    assert np.min(np.diff(res.trace)) >= -1e-11 * abs(res.maximum)
    _maximum_criteria(nhp, make, c["data"], res.maximizer, res.maximum, recursive, what=f"{kind} recursive={recursive}")


def _sparse_case(nhp):
    """The sparse truth of tests/test_cont_inference_gpu.py::test_device_mle_with_most_weights_on_the_lower_bound."""
    N, T = 8, 600.0
    rng = np.random.default_rng(12)
    W = rng.uniform(0.1, 0.4, (N, N)) * (rng.uniform(size=(N, N)) < 0.25)
    lam0, theta = rng.uniform(0.5, 1.0, N), rng.uniform(2.0, 4.0, (N, N))

    def make():
        return nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0.copy()), nhp.ExponentialImpulseResponse(theta.copy(), 1.0, 1.0, 2.0),
                                                   nhp.DenseWeightModel(W.copy()))
    data = nhp.synthetic.rand(make(), T, seed=4)
    guess = np.random.default_rng(6).uniform(0.3, 0.9, len(make().params()))
    return make, data, guess, N


def test_em_on_the_sparse_truth(nhp):
    """Three quarters of the true weights are zero: EM shrinks them multiplicatively towards the bound instead of clipping
    quasi-Newton steps.  Same criteria as above, from the guess of the device L-BFGS's test."""
    make, data, guess, N = _sparse_case(nhp)
    assert len(data[0]) > 3000
    proc = make()
    ll0 = nhp.loglikelihood(_set(make(), guess), data, recursive=False)
    res = nhp.em_(proc, data, guess=guess, recursive=False, f_abstol=1e-10, max_steps=40000)
    Wfit = res.maximizer[N + N * N:].reshape((N, N), order="F")
    print(f"sparse truth: EM {res.steps} iterations in {res.elapsed:.3f} s, {ll0:.3f} -> {res.maximum:.6f}; "
          f"{(Wfit == 1e-6).sum()} weights on the bound, {(Wfit < 1e-4).sum()} below 1e-4")
    assert res.status == "success" and res.maximum >= ll0
    _maximum_criteria(nhp, make, data, res.maximizer, res.maximum, False, what="sparse truth", f_abstol=1e-10)


@pytest.mark.parametrize("kind,recursive", [("exponential", True), ("exponential", False), ("logitnormal", False)])
def test_map_fit_is_one_the_host_optimizer_cannot_improve(nhp, kind, recursive):
    def make():
        p = random_case(5, 3000, 250.0, kind, 1.5, seed=31, nhp=nhp)["proc"]
        b, w, imp = p.baseline, p.weights, p.impulses
        b.α0, b.β0, w.κ, w.ν = 2.0, 1.5, 1.5, 2.0
        if kind == "exponential":
            imp.α, imp.β = 2.0, 0.7
        else:
            imp.α0, imp.β0, imp.μμ, imp.κμ = 2.0, 0.7, 0.5, 2.0
        return p
    c = random_case(5, 3000, 250.0, kind, 1.5, seed=31, nhp=nhp)
    guess = np.random.default_rng(5).uniform(0.2, 0.8, len(c["proc"].params()))
    proc = make()
    res = nhp.em_(proc, c["data"], guess=guess, recursive=recursive, regularize=True, f_abstol=1e-9, max_steps=11000)
    print(f"MAP {kind} recursive={recursive}: EM {res.steps} iterations in {res.elapsed:.3f} s -> {res.maximum:.6f}")
    assert res.status == "success"
    assert res.maximum == pytest.approx(nhp.loglikelihood(proc, c["data"], recursive=recursive) + nhp.logprior(proc), rel=1e-11)
    _maximum_criteria(nhp, make, c["data"], res.maximizer, res.maximum, recursive, regularize=True, what=f"MAP {kind} recursive={recursive}")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_device_simulated_data_end_to_end(nhp, kind):
    """rand(device=True) -> em_ -> time_rescaling_test with no host copy of the events: N = 64, about 1e5 events, seed 7 (the
    restatement is not feasible at this size, so the observed p is stated).  The truth lies inside the box [1e-6, 10]
    (θ <= 5 with θ·Δtmax >= 16: rand does not cut exponential delays at Δtmax, the intensity does; μ > 0: the box clamps μ as
    it does in mle!).  P = 8256 | 12352 parameters for 1e5 events is 12 | 8 events per parameter -- a dense link carries about
    7 -- so the fit that is checked is the MAP fit under the package's DEFAULT priors (all hyperparameters 1: Gamma(1, 1) on
    θ pulls a link without data away from the box's upper bound), regularize=True.  The unregularised maximum is printed
    beside it: it overfits and time rescaling sees that.  Observed on the MI355X: exponential 100119 events, MAP fit 5847
    iterations, pooled D = 0.00356, p = 0.158 (under the truth 0.447; unregularised 7631 iterations, ll 2050 above the
    truth's, p = 8.6e-5); logit-normal 100122 events, 5736 iterations, D = 0.00552, p = 0.0045 (truth 0.732; unregularised
    5877 iterations, ll 5797 above the truth's, p = 8.7e-3)."""
    N, T = 64, 2000.0
    r = np.random.default_rng(21)
    lam0 = r.uniform(.3, .8, N)
    W = r.uniform(0, 1, (N, N)) * 0.6 / N

    def make():
        if kind == "exponential":
            imp = nhp.ExponentialImpulseResponse(r0["p1"].copy(), 1.0, 1.0, 8.0)
        else:
            imp = nhp.LogitNormalImpulseResponse(r0["p1"].copy(), r0["p2"].copy(), 1.0)
        return nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0.copy()), imp, nhp.DenseWeightModel(W.copy()))
    r0 = {"p1": r.uniform(2, 5, (N, N))} if kind == "exponential" else {"p1": r.uniform(0.2, 1.5, (N, N)), "p2": r.uniform(.5, 2, (N, N))}
    true = make()
    data = nhp.rand(true, T, seed=7, device=True)
    assert data[0].is_cuda and 80_000 <= len(data[0]) <= 125_000
    truth = nhp.loglikelihood(true, data, recursive=False) + nhp.logprior(true)
    p_truth = nhp.time_rescaling_test(true, data).pvalue
    plain = make()
    res0 = nhp.em_(plain, data, seed=1, recursive=False, max_steps=40000)
    p_plain = nhp.time_rescaling_test(plain, data).pvalue
    proc = make()
    res = nhp.em_(proc, data, seed=1, recursive=False, max_steps=40000, regularize=True)
    test = nhp.time_rescaling_test(proc, data)
    print(f"{kind}: M={len(data[0])} MAP EM {res.steps} iterations in {res.elapsed:.3f} s, ll + logprior {res.maximum:.3f} (truth {truth:.3f}); "
          f"pooled KS D={test.statistic:.5f} p={test.pvalue:.4f} (under the truth p={p_truth:.4f}; unregularised: {res0.steps} iterations, "
          f"ll {res0.maximum:.3f}, p={p_plain:.2e})")
    assert res.status == "success" and res.maximum > truth
    assert test.pvalue > 1e-3


def test_the_example_runs():
    θ, res, stats, test = importlib.import_module("continuous_exponential_standard_hawkes_em").main(duration=4000.0)
    assert res.status == "success" and np.all(np.diff(res.trace) >= -1e-11 * abs(res.maximum))
    assert np.all(np.abs(res.maximizer[:2] - θ[:2]) / θ[:2] < 0.25)          # baseline rates
    assert np.max(np.abs(res.maximizer[-4:] - θ[-4:])) < 0.15                # weights
    assert stats.EM.shape == (2, 2) and test.pvalue > 1e-3
