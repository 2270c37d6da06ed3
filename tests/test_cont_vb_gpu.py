"""GPU tests of the continuous variational fit (csrc/cont_vb.hip): one nhp_cont_vb_step against the numpy/scipy restatement
(tests/vb_ref.py) over tests/test_em_gpu.py's cases and routes, the run against its own steps, tiny surrogate weights, trials,
resuming, rand -> vb_ -> loglikelihood on the device, and the refusals of the C entry points."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

import em_ref as er
import slices_ref
import vb_ref as vr
from helpers import random_case

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

TOL = 1e-10          # |got - want| <= TOL·max(1, |want|) per factor entry: the bound tests/test_em_gpu.py holds the statistics to
TOL_PIECE = 1e-11    # relative, per ELBO piece, plus the rounded-terms allowance of _allowance
EPS = 2.0 ** -52
CASES = [("exponential", 0.5, False), ("exponential", 1.5, False), ("exponential", np.inf, False), ("exponential", np.inf, True),
         ("exponential", 1.5, True), ("logitnormal", 0.5, False), ("logitnormal", 1.5, False)]
PRIORS = dict(alpha0=2.0, beta0=1.5, kappa=1.5, nu=2.0, a=2.0, b=0.7, mu_mu=0.5, kappa_mu=2.0)


def _with_priors(proc, q=PRIORS):
    b, w, imp = proc.baseline, proc.weights, proc.impulses
    b.α0, b.β0, w.κ, w.ν = q["alpha0"], q["beta0"], q["kappa"], q["nu"]
    if hasattr(imp, "θ"):
        imp.α, imp.β = q["a"], q["b"]
    else:
        imp.α0, imp.β0, imp.μμ, imp.κμ = q["a"], q["b"], q["mu_mu"], q["kappa_mu"]
    return proc


def _routes(monkeypatch, nhp, proc, data, chunk="4096"):
    """tests/test_em_gpu.py's _routes: the one-launch slices route (where the dataset, built with items of `chunk` children,
    keeps its child slices) and the two-pass route.  After each leg the scalars of the dataset it ran on say which layout that
    was; whether the slices are kept is tests/slices_ref.py's restated rule instead of a rule of thumb, because the shapes
    here go down to one event."""
    dt_max = float(proc.impulses.Δtmax)

    def kept(items):
        if len(data[0]) == 0 or not np.isfinite(dt_max):
            return False
        return bool(slices_ref.layout(data[0], data[1], proc.ndims(), dt_max, int(items) if items else None).kept)
    for name, env in (("default", {"NHP_CHUNK": chunk} if chunk else {}), ("two-pass", {"NHP_GRAD_SLICES": "0"})):
        for k in ("NHP_GRAD_SLICES", "NHP_CHUNK"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        nhp.invalidate_device_datasets()
        has_slices = kept(env.get("NHP_CHUNK"))              # (NHP_GRAD_SLICES=0 turns the route off, not the dataset's slices)
        yield name, has_slices and name == "default"
        rows = nhp.device_dataset(proc, data).scalars()["sl_rows"]
        assert (rows > 0) == has_slices, (name, rows, has_slices)
    for k in ("NHP_GRAD_SLICES", "NHP_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    nhp.invalidate_device_datasets()


def _state_object(nhp, state, kind, N, q=PRIORS):
    return nhp.ContinuousVariational(kind, N, *vr.planes(state), prior_kappa=q["kappa"])


def _kl_gamma_terms(a1, b1, a0, b0):
    """Σ over the entries of the magnitudes of the five terms a Gamma KL is added up from."""
    from scipy.special import digamma, gammaln
    return float(np.sum(np.abs((a1 - a0) * digamma(a1)) + np.abs(gammaln(a1)) + abs(gammaln(a0)) + np.abs(a0 * (np.log(b1) - np.log(b0)))
                        + np.abs(a1 * (b0 - b1) / b1)))


def _allowance(state, cnt, T, q):
    """The rounded-terms allowance of the four pieces of a state, as tests/test_em_gpu.py grants its log prior: a piece is a
    sum of n entries, each added up from a few terms that are rounded where they are formed (ψ and lnΓ by recurrence and
    series: a few ulp of their own size), so its error is a small multiple of ε·Σ|terms|, whatever the piece itself cancels
    to.  16 ulp per term covers the recurrences' ten divisions."""
    comp = float(np.sum(T * state["alpha"] / state["beta"]) + np.sum(cnt[:, None] * state["kappa"] / state["nu"]))
    kl0 = _kl_gamma_terms(state["alpha"], state["beta"], q["alpha0"], q["beta0"])
    klw = _kl_gamma_terms(state["kappa"], state["nu"], q["kappa"], q["nu"])
    kli = _kl_gamma_terms(state["a"], state["b"], q["a"], q["b"])
    if "m" in state:
        k, prec, dm = state["k"], state["a"] / state["b"], state["m"] - q["mu_mu"]
        kli += float(np.sum(0.5 * (q["kappa_mu"] / k + 1.0 + np.abs(np.log(k / q["kappa_mu"])) + q["kappa_mu"] * prec * dm ** 2)))
    return [16.0 * EPS * v for v in (comp, kl0, klw, kli)]


def _check_state(got, want, what, tol=TOL):
    gS, gR = got.S, got.R
    wS, wR = vr.planes(want)
    worst = 0.0
    for name, g, w in (("S", gS, wS), ("R", gR, wR)):
        assert g.shape == w.shape and np.all(np.isfinite(g)), (what, name)
        ratio = float(np.max(np.abs(g - w) / (tol * np.maximum(1.0, np.abs(w)))))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, name, ratio)
    return worst


def _check_pieces(got4, want_state, cnt, T, q, what):
    want4 = vr.pieces(want_state, cnt, T, q)
    for name, g, w, al in zip(("compensator", "KL_lambda0", "KL_W", "KL_imp"), got4, want4, _allowance(want_state, cnt, T, q)):
        bound = TOL_PIECE * max(1.0, abs(w)) + al
        print(f"{what} {name}: got {g:.12g} want {w:.12g}, error / bound = {abs(g - w) / bound:.3e}")
        assert abs(g - w) <= bound, (what, name, g, w)


def _one_step_against_the_restatement(nhp, proc, data, kind, dt_max, recursive, what, seed=1, q=PRIORS):
    """update_ from a random positive state: the new factors, Σ log λ̃ and the pieces of both states against vb_ref."""
    N = proc.ndims()
    state = vr.random_state(N, kind, seed)
    pr = er.Pairs(data[0], data[1], data[2], N, dt_max, recursive=recursive and kind == "exponential")
    model = vr.surrogate(state, dt_max)
    want, loglam, stats = vr.step(model, pr, q)
    got = nhp.update_(proc, data, init=_state_object(nhp, state, kind, N, q), recursive=recursive)
    worst = _check_state(got, want, what)
    # Σ log λ̃ = ll(x̃) + T Σ λ̃0 + Σ cnt W̃: the rounded terms are those of ll(x̃) itself and, twice (charged and undone), the fixed ones
    fix = float(pr.T * np.sum(model.lam0) + np.sum(pr.cnt[:, None] * model.W))
    bound = TOL_PIECE * max(1.0, abs(loglam)) + 16.0 * EPS * (abs(stats[0]) + 2.0 * fix)
    print(f"{what}: factors' largest error / bound = {worst:.3e}; loglam got {got.pieces['loglam']:.12g} want {loglam:.12g}, "
          f"error / bound = {abs(got.pieces['loglam'] - loglam) / bound:.3e}")
    assert abs(got.pieces["loglam"] - loglam) <= bound
    _check_pieces(got.pieces["before"], state, pr.cnt, pr.T, q, what + " before")
    _check_pieces(got.pieces["after"], want, pr.cnt, pr.T, q, what + " after")
    assert got.elbo == got.pieces["loglam"] - got.pieces["before"][0] - got.pieces["before"][1] - got.pieces["before"][2] - got.pieces["before"][3]
    return got, want, pr


@pytest.mark.parametrize("N,M,T", [(3, 300, 30.0), (70, 2000, 100.0)])
@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_one_step_matches_the_restatement(nhp, kind, dt_max, recursive, N, M, T, monkeypatch):
    """N = 3: the dataset keeps its child slices where Δtmax is finite (asserted).  N = 70: more than one wave of nodes,
    P = 9870 | 14770 is no multiple of the passes' 256 threads."""
    case = random_case(N, M, T, kind, dt_max, seed=3, nhp=nhp)
    proc = _with_priors(case["proc"])
    sliced = []
    for route, on_slices in _routes(monkeypatch, nhp, proc, case["data"]):
        sliced.append(on_slices)
        _one_step_against_the_restatement(nhp, proc, case["data"], kind, dt_max, recursive, f"{kind} dt_max={dt_max} rec={recursive} N={N} {route}")
    if N == 3 and np.isfinite(dt_max):
        assert sliced[0]


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_step_with_one_node(nhp, kind, monkeypatch):
    case = random_case(1, 200, 40.0, kind, 1.0, seed=5, nhp=nhp)
    proc = _with_priors(case["proc"])
    for route, _ in _routes(monkeypatch, nhp, proc, case["data"]):
        _one_step_against_the_restatement(nhp, proc, case["data"], kind, 1.0, False, f"{kind} N=1 {route}")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_step_with_ties_and_a_node_without_events(nhp, kind, monkeypatch):
    """tests/test_em_gpu.py's tied dataset (default items, no child slices: its docstring).  The node without events keeps the
    prior on its column and row, its baseline factor is prior + exposure."""
    case = random_case(7, 1500, 150.0, kind, 1.0, seed=13, nhp=nhp)
    proc = _with_priors(case["proc"])
    data = (np.round(case["times"]), np.where(case["nodes"] == 4, 5, case["nodes"]), case["T"])
    for route, _ in _routes(monkeypatch, nhp, proc, data, chunk=None):
        got, want, pr = _one_step_against_the_restatement(nhp, proc, data, kind, 1.0, False, f"{kind} ties {route}")
        assert pr.cnt[3] == 0
        assert got.alpha[3] == PRIORS["alpha0"] and got.beta[3] == PRIORS["beta0"] + case["T"]
        assert np.all(got.kappa[3] == PRIORS["kappa"]) and np.all(got.kappa[:, 3] == PRIORS["kappa"]) and np.all(got.nu[3] == PRIORS["nu"])
        assert np.all(got.expected_links()[3] == 0.0)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("M", [0, 1])
def test_no_event_and_one_event(nhp, kind, M):
    case = random_case(4, 10, 20.0, kind, 1.0, seed=2, nhp=nhp)
    proc = _with_priors(case["proc"])
    data = (case["times"][:M], case["nodes"][:M], case["T"])
    for recursive in (False, True):
        got, want, pr = _one_step_against_the_restatement(nhp, proc, data, kind, 1.0, recursive, f"{kind} M={M} rec={recursive}")
        assert np.all(got.kappa == PRIORS["kappa"]) and np.all(got.beta == PRIORS["beta0"] + 20.0)     # no event has a parent
        if M == 0:
            assert got.pieces["loglam"] == 0.0 and np.all(got.alpha == PRIORS["alpha0"]) and np.all(got.nu == PRIORS["nu"])
    # the run on the same data: prior + exposure, a finite ELBO that does not fall
    res = nhp.vb_(proc, data, max_steps=3, f_abstol=0.0, recursive=False)
    assert res.steps == 3 and np.all(np.isfinite(res.trace)) and np.min(np.diff(res.trace)) >= -1e-11 * abs(res.elbo)
    assert np.all(res.kappa == PRIORS["kappa"]) and np.array_equal(proc.params(), res.mean())


def _steps_of(nhp, proc, data, guess, steps, recursive):
    """`steps` calls of nhp_cont_vb_step from the guess: the states, and the ELBO of every state stepped from."""
    proc.params_(guess)
    out, trace = [], []
    state = None
    for _ in range(steps):
        state = nhp.update_(proc, data, init=state, recursive=recursive)
        out.append(state)
        trace.append(state.elbo)
    return out, np.array(trace[1:])


def _fixed_order_recursion(monkeypatch, kind, recursive):
    """A recursive evaluation through the recursion itself (fixed summation order), not its truncated window."""
    if not (recursive and kind == "exponential"):
        return False
    monkeypatch.setenv("NHP_REC_WINDOW", "0")
    return True


def _same(a, b, exact, what):
    if exact:
        assert np.array_equal(a.S, b.S) and np.array_equal(a.R, b.R), what
    else:
        for g, w in ((a.S, b.S), (a.R, b.R)):
            assert np.max(np.abs(g - w) / (TOL * np.maximum(1.0, np.abs(w)))) <= 1.0, what


@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_the_trace_never_falls_and_the_run_is_its_steps(nhp, kind, dt_max, recursive, monkeypatch):
    """40 updates: min(diff(trace)) >= -1e-11·|L| (the EM trace's bound), and 40 calls of nhp_cont_vb_step reproduce the run's
    factors -- bit for bit on the fixed-order routes, within the factor bound on the two-pass route, whose LDS atomics
    csrc/cont_em.hip documents.  Fixed order: the one-launch child-slices route (exponential impulses on a dataset that keeps
    its slices) and the O(M·N) recursion, which NHP_REC_WINDOW=0 selects for every recursive evaluation (otherwise the
    gradient may go through the truncated window, on the two-pass kernels)."""
    N = 7
    exact_rec = _fixed_order_recursion(monkeypatch, kind, recursive)
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data = case["data"]
    guess = case["proc"].params()
    for route, on_slices in _routes(monkeypatch, nhp, case["proc"], data):
        proc = _with_priors(random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"])
        res = nhp.vb_(proc, data, max_steps=40, f_abstol=0.0, guess=guess, recursive=recursive)
        assert res.steps == 40 and res.status == "failure" and len(res.trace) == 40 and res.elbo == res.trace[-1]
        rise = np.diff(res.trace)
        print(f"{kind} dt_max={dt_max} rec={recursive} {route}: L {res.trace[0]:.4f} -> {res.elbo:.6f}, smallest rise {rise.min():.3e}")
        assert np.all(np.isfinite(res.trace)) and rise.min() >= -1e-11 * abs(res.elbo)
        assert np.array_equal(proc.params(), res.mean())
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        states, trace = _steps_of(nhp, _with_priors(random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"]), data, guess, 40, recursive)
        _same(states[-1], res, exact, (kind, dt_max, recursive, route))
        if exact:
            assert np.array_equal(trace, res.trace[:-1])
        else:
            assert np.max(np.abs(trace - res.trace[:-1]) / np.abs(res.trace[:-1])) <= 1e-10
    # the first restated steps from the same guess (numpy's sums): the same trace
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, dt_max, recursive=recursive)
    _, want = vr.run(er.from_vector(guess, N, kind, dt_max), pr, PRIORS, 3, exact=False)
    assert np.max(np.abs(res.trace[:3] - want) / np.maximum(1.0, np.abs(want))) <= 1e-9


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_step_with_most_surrogate_weights_tiny(nhp, kind, monkeypatch):
    """A prior κ = 0.05 and a state whose κ' is that prior on three quarters of the links: their surrogate weights are
    exp(ψ(0.05) - ...) ~ 1e-10, far below the 1e-6 of mle_'s box.  The statistics there stay finite and positive and right to
    1e-9 of themselves (nothing in the E-step divides by W̃), and the step matches the restatement on those links to 1e-9
    relative.  Mirrors tests/test_em_gpu.py::test_statistics_with_most_weights_on_the_lower_bound."""
    q = dict(PRIORS, kappa=0.05)
    N = 7
    case = random_case(N, 1500, 80.0, kind, 1.5, seed=4, nhp=nhp)
    proc = _with_priors(case["proc"], q)
    state = vr.random_state(N, kind, seed=2)
    tiny = np.random.default_rng(0).uniform(size=(N, N)) < 0.75
    state["kappa"][tiny] = 0.05
    assert tiny.sum() >= 30
    model = vr.surrogate(state, 1.5)
    assert np.max(model.W[tiny]) < 1e-8
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, 1.5)
    want, _, stats = vr.step(model, pr, q)
    small = stats[2][tiny]
    assert np.all(small > 0) and np.max(small) < 1e-5
    for route, _ in _routes(monkeypatch, nhp, proc, case["data"]):
        at = _with_priors(random_case(N, 1500, 80.0, kind, 1.5, seed=4, nhp=nhp)["proc"], q)
        at.params_(er.params_vector(model))
        es = nhp.expected_statistics(at, case["data"], recursive=False)
        assert np.all(np.isfinite(es.EM)) and np.all(es.EM[tiny] > 0)
        rel = np.max(np.abs(es.EM[tiny] - small) / small)
        print(f"{kind} tiny weights {route}: largest relative error of the EM of a tiny link {rel:.2e}")
        assert rel <= 1e-9
        got = nhp.update_(proc, case["data"], init=_state_object(nhp, state, kind, N, q), recursive=False)
        _check_state(got, want, f"{kind} tiny weights {route}")
        for name in ("kappa", "nu", "a", "b") + (("m", "k") if kind == "logitnormal" else ()):
            g, w = getattr(got, name)[tiny], want[name][tiny]
            assert np.all(np.isfinite(g)) and np.max(np.abs(g - w) / np.abs(w)) <= 1e-9, (route, name)
        assert np.all(got.kappa > 0) and np.all(got.b > 0) and np.all(got.a > 0)


@pytest.mark.parametrize("kind,recursive", [("exponential", False), ("exponential", True), ("logitnormal", False)])
def test_three_trials_are_the_sum_of_their_statistics(nhp, kind, recursive):
    """A list of three trials: one step is the update from the three trials' separately restated statistics added up, with
    summed cnt and T (no window crosses a trial's end; the recursion restarts)."""
    N, dt_max = 4, 1.5
    q = PRIORS
    trials = []
    for s, (M, T) in enumerate(((300, 30.0), (180, 25.0), (40, 12.0))):
        c = random_case(N, M, T, kind, dt_max, seed=20 + s, nhp=nhp)
        trials.append((c["times"] + (0.0 if not recursive else 1e-3), c["nodes"], T + 1.0))
    proc = _with_priors(random_case(N, 10, 10.0, kind, dt_max, seed=1, nhp=nhp)["proc"])
    state = vr.random_state(N, kind, seed=6)
    model = vr.surrogate(state, dt_max)
    parts = [(er.statistics(model, p), p) for p in (er.Pairs(t, n, T, N, dt_max, recursive=recursive) for t, n, T in trials)]
    summed = [sum(s[i] for s, _ in parts) if parts[0][0][i] is not None else None for i in range(5)]
    cnt, T = sum(p.cnt for _, p in parts), sum(p.T for _, p in parts)
    want = vr.update(model, summed, cnt, T, q)
    got = nhp.update_(proc, trials, init=_state_object(nhp, state, kind, N), recursive=recursive)
    worst = _check_state(got, want, f"{kind} trials rec={recursive}")
    print(f"{kind} three trials recursive={recursive}: largest error / bound = {worst:.3e}")
    assert np.all(got.beta == q["beta0"] + T)
    _check_pieces(got.pieces["after"], want, cnt, T, q, f"{kind} trials")


@pytest.mark.parametrize("kind,dt_max,recursive", [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)])
def test_resuming_continues_the_run(nhp, kind, dt_max, recursive, monkeypatch):
    """init=res: 10 + 10 updates are 20 updates, under the equality rule of the run against its steps."""
    N = 7
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    guess = case["proc"].params()
    exact_rec = _fixed_order_recursion(monkeypatch, kind, recursive)
    fresh = lambda: _with_priors(random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"])
    for route, on_slices in _routes(monkeypatch, nhp, case["proc"], case["data"]):
        kw = dict(f_abstol=0.0, recursive=recursive)
        whole = nhp.vb_(fresh(), case["data"], max_steps=20, guess=guess, **kw)
        first = nhp.vb_(fresh(), case["data"], max_steps=10, guess=guess, **kw)
        proc = fresh()
        second = nhp.vb_(proc, case["data"], max_steps=10, init=first, **kw)
        assert second.steps == 10 and len(second.trace) == 11 and np.array_equal(proc.params(), second.mean())
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        _same(second, whole, exact, (kind, route))
        joined = np.concatenate([first.trace, second.trace[1:]])
        if exact:
            assert second.trace[0] == first.trace[-1] and np.array_equal(joined, whole.trace)
        else:
            assert np.max(np.abs(joined - whole.trace) / np.abs(whole.trace)) <= 1e-10
    with pytest.raises(ValueError):
        nhp.vb_(fresh(), case["data"], init=first, guess=guess)


def test_device_simulated_data_end_to_end(nhp):
    """rand(device=True) -> vb_ with no host copy of the events: N = 4, about 5000 events."""
    N, T = 4, 1600.0
    r = np.random.default_rng(21)
    lam0, W, theta = r.uniform(.3, .8, N), r.uniform(0, 1, (N, N)) * 0.6 / N, r.uniform(2, 5, (N, N))

    def make():
        return nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0.copy()), nhp.ExponentialImpulseResponse(theta.copy(), 1.0, 1.0, 8.0),
                                                   nhp.DenseWeightModel(W.copy()))
    data = nhp.rand(make(), T, seed=7, device=True)
    assert data[0].is_cuda and 3000 <= len(data[0]) <= 8000
    guess = np.random.default_rng(5).uniform(0.2, 0.8, len(make().params()))
    at_guess = make()
    at_guess.params_(guess)
    ll0 = nhp.loglikelihood(at_guess, data, recursive=False)
    proc = make()
    res = nhp.vb_(proc, data, guess=guess, recursive=False, max_steps=2000)
    ll1 = nhp.loglikelihood(proc, data, recursive=False)
    lo, hi = res.interval(0.95)
    truth = make().params()
    print(f"M={len(data[0])}: {res.steps} updates in {res.elapsed:.3f} s, ELBO {res.elbo:.3f}; ll {ll0:.3f} -> {ll1:.3f}; "
          f"{int(np.sum((lo <= truth) & (truth <= hi)))} of {len(truth)} true parameters inside their 95% intervals")
    assert res.status == "success" and np.isfinite(res.elbo) and np.min(np.diff(res.trace)) >= -1e-11 * abs(res.elbo)
    assert ll1 >= ll0
    assert np.array_equal(proc.params(), res.mean())
    assert res.expected_links().shape == (N, N) and np.all(res.sd() > 0) and np.all(lo < res.mean()) and np.all(res.mean() < hi)
    cnt = np.bincount(data[1].cpu().numpy() - 1, minlength=N)
    assert np.allclose(res.expected_links().sum(axis=0) + (res.alpha - proc.baseline.α0), cnt, rtol=1e-10)


def test_the_example_runs():
    truth, res, lo, hi = importlib.import_module("continuous_exponential_standard_hawkes_vb").main(duration=2000.0)
    assert res.status == "success" and np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo))
    assert lo.shape == truth.shape and np.all(lo < res.mean()) and np.all(res.mean() < hi)
    # the criteria of tests/test_em_gpu.py's example test, on the posterior means (mean-field intervals are too narrow to ask
    # them to cover the truth: they ignore the dependence between a link's weight and the baseline)
    assert np.all(np.abs(res.mean()[:2] - truth[:2]) / truth[:2] < 0.25)      # baseline rates
    assert np.max(np.abs(res.mean()[-4:] - truth[-4:])) < 0.15                # weights


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_a_step_on_device_planes_is_the_step_on_host_planes(nhp, kind):
    """output_on_device = 1: S and R are device pointers, read and overwritten in place; the same numbers as through host
    arrays (within the factor bound: the route of this dataset adds with LDS atomics), the same nine scalars likewise."""
    import torch
    from nhp_amd import _lib, inference
    N = 5
    case = random_case(N, 600, 60.0, kind, 1.0, seed=8, nhp=nhp)
    proc = _with_priors(case["proc"])
    state = _state_object(nhp, vr.random_state(N, kind, 3), kind, N)
    host = nhp.update_(proc, case["data"], init=state, recursive=False)
    ctx = nhp.default_context()
    dev = torch.device("cuda", ctx.device)
    dS, dR = torch.as_tensor(state.S).to(dev), torch.as_tensor(state.R).to(dev)
    torch.cuda.current_stream(dev).synchronize()
    stats, pr = np.empty(9), inference._priors(proc)
    ds, model = nhp.device_dataset(proc, case["data"], ctx), proc.device_model(ctx)
    _lib.check(_lib.lib().nhp_cont_vb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), dS.data_ptr(), dR.data_ptr(), len(state.S), 1, _lib.dptr(stats)),
               ctx.h)
    for g, w in ((dS.cpu().numpy(), host.S), (dR.cpu().numpy(), host.R)):
        assert np.max(np.abs(g - w) / (TOL * np.maximum(1.0, np.abs(w)))) <= 1.0
    want = np.array([host.pieces["loglam"], *host.pieces["before"], *host.pieces["after"]])
    assert np.array_equal(stats[1:5], want[1:5])                     # the pieces of the state stepped from: no statistics in them
    assert np.max(np.abs(stats - want) / np.maximum(1.0, np.abs(want))) <= 1e-10


def test_refusals_of_the_device_entry_points(nhp):
    """nhp_cont_vb_step / nhp_cont_vb_run themselves: NHP_ENOTIMPL (6) for a model with A and for an LGCP baseline, NHP_EINVAL (1)
    for missing priors or a hyper-parameter that is not positive, NHP_ESHAPE (3) for a wrong length -- and nothing written."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    good = _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)

    def calls(proc, data, pr, P=None):
        ds, model = nhp.device_dataset(proc, data, ctx), proc.device_model(ctx)
        P = len(proc.params()) if P is None else P
        S, R, x, stats = np.full(P, 7.0), np.full(P, 7.0), np.full(P, 0.5), np.full(9, 7.0)
        e, st, cv = C.c_double(), C.c_int32(), C.c_int32()
        prp = C.byref(pr) if pr is not None else None
        rc = (lib.nhp_cont_vb_step(ctx.h, ds.h, model.h, 0, prp, S.ctypes.data, R.ctypes.data, P, 0, _lib.dptr(stats)),
              lib.nhp_cont_vb_run(ctx.h, ds.h, model.h, 0, prp, 1e-6, 5, _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P, C.byref(e), C.byref(st),
                                  C.byref(cv), None))
        assert np.all(S == 7.0) and np.all(R == 7.0) and np.all(stats == 7.0) and np.all(x == 0.5)
        return rc
    std = random_case(3, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    net = random_case(3, 50, 10.0, "exponential", 1.0, network=True, seed=1, nhp=nhp)
    lgcp = random_case(3, 50, 10.0, "exponential", 1.0, lgcp=True, seed=1, nhp=nhp)
    assert calls(net["proc"], net["data"], good) == (6, 6)
    assert calls(lgcp["proc"], lgcp["data"], good) == (6, 6)
    assert calls(std["proc"], std["data"], None) == (1, 1)
    for field in ("alpha0", "beta0", "kappa", "nu", "a", "b"):
        for bad in (0.0, -1.0, np.nan, np.inf):
            pr = _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)
            setattr(pr, field, bad)
            assert calls(std["proc"], std["data"], pr) == (1, 1), (field, bad)
    ln = random_case(3, 50, 10.0, "logitnormal", 1.0, seed=1, nhp=nhp)
    assert calls(ln["proc"], ln["data"], _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 0.0)) == (1, 1)
    assert calls(ln["proc"], ln["data"], _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, np.inf, 1.0)) == (1, 1)
    assert calls(std["proc"], std["data"], good, P=20) == (3, 3)


def test_a_refused_step_leaves_the_host_planes_alone(nhp):
    """nhp_cont_vb_step itself on host planes, N = 2 and three events, from a state whose baseline shapes are 1e-300: the
    surrogate λ̃0 = exp(ψ(α') - log β') underflows to zero, the first event has no parent, so its intensity is zero:
    NHP_EDOMAIN (2), and S, R are byte for byte what was passed in."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    N = 2
    case = random_case(N, 3, 2.0, "exponential", 1.0, seed=1, nhp=nhp)
    P = N + 2 * N * N
    S, R, stats = np.full(P, 2.0), np.full(P, 1.5), np.full(9, 7.0)
    S[:N] = 1e-300
    keep = S.tobytes(), R.tobytes()
    pr = _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)
    ds, model = nhp.device_dataset(case["proc"], case["data"], ctx), case["proc"].device_model(ctx)
    rc = lib.nhp_cont_vb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), S.ctypes.data, R.ctypes.data, P, 0, _lib.dptr(stats))
    assert rc == 2
    assert (S.tobytes(), R.tobytes()) == keep
