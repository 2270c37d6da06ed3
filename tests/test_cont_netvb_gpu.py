"""GPU tests of the continuous network variational fit (csrc/cont_netvb.hip): one nhp_cont_netvb_step against the numpy/scipy
restatement (tests/cnetvb_ref.py) over tests/test_cont_vb_gpu.py's shapes, cases and routes, the dense network against the
standard fit, the run against its own steps, resuming, edge shapes, trials, device planes, the refusals of the C entry
points and the example.

Bounds.  Factor entries (S, R, κv0, νv0, αv, βv): the project's TOL = 1e-10.  ELBO pieces: TOL_PIECE = 1e-11 relative plus 16 ulp
per rounded term of Σ|terms| (tests/test_cont_vb_gpu.py's allowance, extended to the spike's share of KL_W and to KL_net by the
same rule).  The link layer is held as tests/test_disc_netvb_gpu.py holds the discrete one: at the tables the device itself
wrote and the network parameters it read, ρv within 1 x the restatement's own rounding error against 50-digit arithmetic
(cr.measured_logit_error(), 4.9e-15 where it was written) and the logit within 4 x that where 1e-3 < ρv < 1 - 1e-3, plus the
rounding of ρv to a double seen through the inverse."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
from scipy.special import digamma, gammaln

import cnetvb_ref as cr
import disc_netvb_ref as dn
import em_ref as er
import slices_ref
import vb_ref as vr
from helpers import random_case

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

TOL = 1e-10
TOL_PIECE = 1e-11
EPS = 2.0 ** -52
CASES = [("exponential", 0.5, False), ("exponential", 1.5, False), ("exponential", np.inf, False), ("exponential", np.inf, True),
         ("exponential", 1.5, True), ("logitnormal", 0.5, False), ("logitnormal", 1.5, False)]
PRIORS = cr.PRIORS
Q_BERNOULLI, Q_DENSE = cr.priors(), cr.priors(net=None)


def _with_priors(proc, q=PRIORS):
    b, w, imp = proc.baseline, proc.weights, proc.impulses
    b.α0, b.β0, w.κ, w.ν = q["alpha0"], q["beta0"], q["kappa"], q["nu"]
    if hasattr(imp, "θ"):
        imp.α, imp.β = q["a"], q["b"]
    else:
        imp.α0, imp.β0, imp.μμ, imp.κμ = q["a"], q["b"], q["mu_mu"], q["kappa_mu"]
    return proc


def _network(nhp, std, q=Q_BERNOULLI, start=cr.NET_START):
    """The network process on the components of the standard process `std`: SparseWeightModel(spike, slab), every link in A,
    a Bernoulli network Beta(α, β) with the start (αv, βv), or a dense one where q["net"] is None."""
    _with_priors(std, q)
    N = std.ndims()
    w = nhp.SparseWeightModel(std.weights.W, q["kappa0"], q["nu0"], q["kappa"], q["nu"])
    net = nhp.DenseNetworkModel(N) if q["net"] is None else nhp.BernoulliNetworkModel(0.5, N, q["net"][0], q["net"][1], start[0], start[1])
    return nhp.ContinuousNetworkHawkesProcess(std.baseline, std.impulses, w, np.ones((N, N)), net)


def _device_guess(proc):
    return np.concatenate([proc.baseline.params(), proc.impulses.params(), proc.weights.params()])


def _routes(monkeypatch, nhp, proc, data, chunk="4096"):
    """tests/test_cont_vb_gpu.py's _routes: the one-launch slices route (where the dataset, built with items of `chunk`
    children, keeps its child slices) and the two-pass route; after each leg the dataset's scalars say which layout ran."""
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
        has_slices = kept(env.get("NHP_CHUNK"))
        yield name, has_slices and name == "default"
        rows = nhp.device_dataset(proc, data).scalars()["sl_rows"]
        assert (rows > 0) == has_slices, (name, rows, has_slices)
    for k in ("NHP_GRAD_SLICES", "NHP_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    nhp.invalidate_device_datasets()


def _state_object(nhp, state, kind, N, q):
    return nhp.ContinuousNetworkVariational(kind, N, *cr.planes(state), prior_kappa=q["kappa"], dense=q["net"] is None)


def _kl_gamma_terms(a1, b1, a0, b0, weight=1.0):
    return float(np.sum(weight * (np.abs((a1 - a0) * digamma(a1)) + np.abs(gammaln(a1)) + abs(gammaln(a0)) + np.abs(a0 * (np.log(b1) - np.log(b0)))
                                  + np.abs(a1 * (b0 - b1) / b1))))


def _allowance(state, cnt, T, q):
    """tests/test_cont_vb_gpu.py's rounded-terms allowance for the five pieces of a network state: 16 ulp per term of Σ|terms|."""
    rho = state["rho"]
    comp = float(np.sum(T * state["alpha"] / state["beta"])
                 + np.sum(cnt[:, None] * ((1.0 - rho) * state["kappa0"] / state["nu0"] + rho * state["kappa"] / state["nu"])))
    kl0 = _kl_gamma_terms(state["alpha"], state["beta"], q["alpha0"], q["beta0"])
    klw = _kl_gamma_terms(state["kappa0"], state["nu0"], q["kappa0"], q["nu0"], 1.0 - rho) + _kl_gamma_terms(state["kappa"], state["nu"], q["kappa"], q["nu"], rho)
    kli = _kl_gamma_terms(state["a"], state["b"], q["a"], q["b"])
    if "m" in state:
        k, prec, dm = state["k"], state["a"] / state["b"], state["m"] - q["mu_mu"]
        kli += float(np.sum(0.5 * (q["kappa_mu"] / k + 1.0 + np.abs(np.log(k / q["kappa_mu"])) + q["kappa_mu"] * prec * dm ** 2)))
    return [16.0 * EPS * v for v in (comp, kl0, klw, kli, cr.net_terms(state, q))]


def _ratio(g, w, tol=TOL):
    return float(np.max(np.abs(g - w) / (tol * np.maximum(1.0, np.abs(w)))))


def _check_state(got, want, what, tol=TOL):
    """Every factor entry but ρv (the link layer's, held by _check_link_layer) within tol."""
    NN = got.N * got.N
    wS, wR, wQ = cr.planes(want)
    worst = 0.0
    for name, g, w in (("S", got.S, wS), ("R", got.R, wR), ("kappa0, nu0", got.Q[:2 * NN], wQ[:2 * NN]), ("alpha_v, beta_v", got.Q[-2:], wQ[-2:])):
        assert g.shape == w.shape and np.all(np.isfinite(g)), (what, name)
        worst = max(worst, _ratio(g, w, tol))
        assert _ratio(g, w, tol) <= 1.0, (what, name, _ratio(g, w, tol))
    return worst


def _check_pieces(got5, want_state, cnt, T, q, what):
    want5 = cr.pieces(want_state, cnt, T, q)
    for name, g, w, al in zip(("compensator", "KL_lambda0", "KL_W", "KL_imp", "KL_net"), got5, want5, _allowance(want_state, cnt, T, q)):
        bound = TOL_PIECE * max(1.0, abs(w)) + al
        print(f"{what} {name}: got {g:.12g} want {w:.12g}, error / bound = {abs(g - w) / bound:.3e}")
        assert abs(g - w) <= bound, (what, name, g, w)


def _check_link_layer(got, old_net, q, what):
    """ρv and the network pair of the device against the restated logit at the device's own tables (module docstring)."""
    err = cr.measured_logit_error()
    own = dict(kappa0=got.kappa0, nu0=got.nu0, nu=got.nu)
    lo_want = cr.logit(own, old_net[0], old_net[1], q)
    rho = got.rho
    assert np.all(np.isfinite(rho)) and np.all((rho >= 0.0) & (rho <= 1.0))
    d = float(np.max(np.abs(rho - dn.sigmoid(lo_want))))
    inner = (rho > 1e-3) & (rho < 1.0 - 1e-3)
    dl = 0.0
    if inner.any():
        back = 4 * 2.2e-16 / (rho[inner] * (1.0 - rho[inner]))             # rounding ρv to a double, seen through the inverse
        gap = np.abs(np.log(rho[inner] / (1.0 - rho[inner])) - lo_want[inner])
        dl = float(gap.max())
        assert np.all(gap <= 4 * err + back), (what, dl, err)
    NN = rho.size
    da = abs(got.net_alpha - (q["net"][0] + float(np.sum(rho)))), abs(got.net_beta - (q["net"][1] + float(np.sum(1.0 - rho))))
    print(f"{what}: max |Δρv| {d:.2e} (bound {err:.2e}); max |Δlogit| inside {dl:.2e} (bound {4 * err:.2e}); {int(inner.sum())} of {NN} links inside; "
          f"network |Δαv| {da[0]:.2e} |Δβv| {da[1]:.2e}")
    assert d <= err, (what, d, err)
    assert max(da) <= TOL * max(1.0, got.net_alpha + got.net_beta)
    return inner


def _one_step(nhp, proc, data, kind, dt_max, recursive, what, q=Q_BERNOULLI, seed=1):
    """update_ from a random state (ρv uniform in [0.05, 0.95], (αv, βv) = (2, 3)): the new factors, Σ log λ̃ and the pieces of
    both states against cnetvb_ref, the link layer at the device's own tables."""
    N = proc.ndims()
    state = cr.random_state(N, kind, seed, dense=q["net"] is None)
    pr = er.Pairs(data[0], data[1], data[2], N, dt_max, recursive=recursive and kind == "exponential")
    model = cr.surrogate(state, dt_max)
    want, loglam, stats = cr.step(model, pr, q, state["na"], state["nb"])
    got = nhp.update_(proc, data, init=_state_object(nhp, state, kind, N, q), recursive=recursive)
    worst = _check_state(got, want, what)
    fix = float(pr.T * np.sum(model.lam0) + np.sum(pr.cnt[:, None] * model.W))
    bound = TOL_PIECE * max(1.0, abs(loglam)) + 16.0 * EPS * (abs(stats[0]) + 2.0 * fix)
    print(f"{what}: factors' largest error / bound = {worst:.3e}; loglam got {got.pieces['loglam']:.12g} want {loglam:.12g}, "
          f"error / bound = {abs(got.pieces['loglam'] - loglam) / bound:.3e}")
    assert abs(got.pieces["loglam"] - loglam) <= bound
    _check_pieces(got.pieces["before"], state, pr.cnt, pr.T, q, what + " before")
    _check_pieces(got.pieces["after"], want, pr.cnt, pr.T, q, what + " after")
    b = got.pieces["before"]
    assert got.elbo == got.pieces["loglam"] - b[0] - b[1] - b[2] - b[3] - b[4]
    if q["net"] is not None:
        _check_link_layer(got, (state["na"], state["nb"]), q, what)
        # against the restatement's own trajectory ρv inherits the tables' bound through the logit's slope (|dρ/dlogit| <= 1/4)
        slope = np.abs(digamma(want["kappa"]) - digamma(want["kappa0"]) - np.log(want["nu"] / want["nu0"]))
        assert np.all(np.abs(got.rho - want["rho"]) <= 0.25 * slope * TOL * np.maximum(1.0, want["kappa0"]) + cr.measured_logit_error())
    else:
        assert np.all(got.rho == 1.0) and (got.net_alpha, got.net_beta) == (state["na"], state["nb"]) and got.pieces["after"][4] == 0.0
    return got, want, pr, stats


@pytest.mark.parametrize("N,M,T", cr.SHAPES)
@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_one_step_matches_the_restatement(nhp, kind, dt_max, recursive, N, M, T, monkeypatch):
    """N = 3: the dataset keeps its child slices where Δtmax is finite (asserted), EM reaches 50, so both branches of the lnΓ
    difference are taken (asserted).  N = 70: more than one wave of nodes, P is no multiple of the passes' 256 threads.
    Condition of the link layer's check: under the restatement at least half of the links have 1e-3 < ρv < 1 - 1e-3."""
    case = random_case(N, M, T, kind, dt_max, seed=3, nhp=nhp)
    proc = _network(nhp, case["proc"])
    sliced = []
    for route, on_slices in _routes(monkeypatch, nhp, proc, case["data"]):
        sliced.append(on_slices)
        got, want, pr, stats = _one_step(nhp, proc, case["data"], kind, dt_max, recursive, f"{kind} dt_max={dt_max} rec={recursive} N={N} {route}")
    inside = np.mean((want["rho"] > 1e-3) & (want["rho"] < 1.0 - 1e-3))
    print(f"N={N}: {inside:.3f} of the links inside (1e-3, 1 - 1e-3); largest EM {stats[2].max():.1f}")
    assert inside >= 0.5
    if N == 3:
        assert np.any(want["kappa0"] >= 16.0) and np.any(want["kappa0"] < 16.0)
        if np.isfinite(dt_max):
            assert sliced[0]


def _fixed_order_recursion(monkeypatch, kind, recursive):
    if not (recursive and kind == "exponential"):
        return False
    monkeypatch.setenv("NHP_REC_WINDOW", "0")
    return True


def _same(a, b, exact, what, q=True):
    planes = [(a.S, b.S), (a.R, b.R)] + ([(a.Q, b.Q)] if q else [])
    for g, w in planes:
        if exact:
            assert np.array_equal(g, w), what
        else:
            assert _ratio(g, w) <= 1.0, what


@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_a_dense_network_is_the_standard_fit(nhp, kind, dt_max, recursive, monkeypatch):
    """DenseNetworkModel + SparseWeightModel(spike, slab = (κ, ν)) against the standard process with DenseWeightModel(κ, ν): same
    data, same guess, 5 steps of update_ and a 5-step vb_.  ρv = 1 gives the slab's E log W exactly, so the S, R planes agree
    bit for bit on the fixed-order routes (within TOL on the two-pass route, whose LDS atomics csrc/cont_em.hip documents);
    the final ELBO within the piece bound of the one-step test summed over its terms -- TOL_PIECE·max(1, |term|) for Σ log λ̃ and
    each of the four pieces, their rounded-terms allowances, and 16 ulp of |Σ log λ̃| + 3·E_q[comp] for the log-likelihood and
    the part of it charged and undone (that part is at most E_q[comp], since exp(ψ(a)) <= a) -- because the network pass adds a
    thread's terms with two more products in them; the earlier entries of the trace within 1e-10 relative, the rule the run is
    held to against its steps off the fixed-order routes."""
    N = 7
    exact_rec = _fixed_order_recursion(monkeypatch, kind, recursive)
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data, guess = case["data"], case["proc"].params()
    fresh = lambda: _with_priors(random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"])
    for route, on_slices in _routes(monkeypatch, nhp, case["proc"], data):
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        std = fresh()
        want = nhp.vb_(std, data, max_steps=5, f_abstol=0.0, guess=guess, recursive=recursive)
        net = _network(nhp, fresh(), Q_DENSE)
        got = nhp.vb_(net, data, max_steps=5, f_abstol=0.0, guess=guess, recursive=recursive)
        assert got.steps == 5 and got.dense and np.all(got.rho == 1.0)
        _same(got, want, exact, (kind, dt_max, recursive, route), q=False)
        pr = er.Pairs(case["times"], case["nodes"], case["T"], N, dt_max, recursive=recursive and kind == "exponential")
        state = cr.from_planes(got.S, got.R, got.Q, N, kind)
        terms = cr.pieces(state, pr.cnt, pr.T, Q_DENSE)[:4]
        loglam = want.elbo + sum(terms)
        bound = TOL_PIECE * sum(max(1.0, abs(v)) for v in (loglam, *terms)) + sum(_allowance(state, pr.cnt, pr.T, Q_DENSE)) \
            + 16.0 * EPS * (abs(loglam) + 3.0 * terms[0])
        print(f"{kind} dt_max={dt_max} rec={recursive} {route}: ELBO dense network {got.elbo:.12g} standard {want.elbo:.12g}, "
              f"difference / bound {abs(got.elbo - want.elbo) / bound:.3e}")
        assert abs(got.elbo - want.elbo) <= bound
        assert np.max(np.abs(got.trace - want.trace) / np.abs(want.trace)) <= 1e-10
        assert np.array_equal(net.weights.W, std.weights.W) if exact else np.allclose(net.weights.W, std.weights.W, rtol=1e-9)
        assert np.all(net.adjacency_matrix == 1.0)
        # the same through update_: five steps of each
        s_std, s_net = None, None
        p_std, p_net = fresh(), _network(nhp, fresh(), Q_DENSE)
        p_std.params_(guess)
        p_net.baseline.λ, p_net.weights.W = p_std.baseline.λ.copy(), p_std.weights.W.copy()
        p_net.impulses.params_(p_std.impulses.params())
        for _ in range(5):
            s_std = nhp.update_(p_std, data, init=s_std, recursive=recursive)
            s_net = nhp.update_(p_net, data, init=s_net, recursive=recursive)
        _same(s_net, s_std, exact, (kind, route, "update_"), q=False)
        _same(s_net, got, exact, (kind, route, "update_ against vb_"))


@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_the_trace_never_falls_and_the_run_is_its_steps(nhp, kind, dt_max, recursive, monkeypatch):
    """25 updates under the Bernoulli network: min(diff(trace)) >= -1e-11·|L|; 25 calls of update_ reproduce the run's state and
    trace, and two identical runs agree -- bit for bit on the fixed-order routes, within TOL on the two-pass route.  The
    process is overwritten as vb_ documents."""
    N, steps = 7, 25
    exact_rec = _fixed_order_recursion(monkeypatch, kind, recursive)
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data, guess = case["data"], case["proc"].params()
    fresh = lambda: _network(nhp, random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"])
    for route, on_slices in _routes(monkeypatch, nhp, case["proc"], data):
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        proc = fresh()
        res = nhp.vb_(proc, data, max_steps=steps, f_abstol=0.0, guess=guess, recursive=recursive)
        assert res.steps == steps and res.status == "failure" and len(res.trace) == steps and res.elbo == res.trace[-1]
        rise = np.diff(res.trace)
        print(f"{kind} dt_max={dt_max} rec={recursive} {route}: L {res.trace[0]:.4f} -> {res.elbo:.6f}, smallest rise {rise.min():.3e}; "
              f"links with ρv > 1/2: {int(np.sum(res.rho > 0.5))} of {N * N}")
        assert np.all(np.isfinite(res.trace)) and rise.min() >= -1e-11 * abs(res.elbo)
        # what vb_ leaves in the process
        assert np.array_equal(_device_guess(proc), res.mean()) and np.array_equal(proc.weights.W, res.kappa / res.nu)
        assert np.array_equal(proc.adjacency_matrix, (res.rho > 0.5).astype(float)) and np.array_equal(proc.weights.ρv, res.rho)
        assert (proc.network.αv, proc.network.βv) == (res.net_alpha, res.net_beta)
        assert proc.network.ρ == res.net_alpha / (res.net_alpha + res.net_beta)
        assert np.array_equal(proc.weights.κv0, res.kappa0) and np.array_equal(proc.weights.νv1, res.nu)
        assert res.net_alpha + res.net_beta == pytest.approx(sum(cr.NET) + N * N, rel=1e-13)
        again = nhp.vb_(fresh(), data, max_steps=steps, f_abstol=0.0, guess=guess, recursive=recursive)
        _same(again, res, exact, (kind, route, "twice"))
        if exact:
            assert np.array_equal(again.trace, res.trace)
        # the run is its steps: update_ from the guess, then from each state
        p = fresh()
        std = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"]
        std.params_(guess)
        p.baseline.λ, p.weights.W = std.baseline.λ.copy(), std.weights.W.copy()
        p.impulses.params_(std.impulses.params())
        state, trace = None, []
        for _ in range(steps):
            state = nhp.update_(p, data, init=state, recursive=recursive)
            trace.append(state.elbo)
        _same(state, res, exact, (kind, route, "steps"))
        trace = np.array(trace[1:])
        if exact:
            assert np.array_equal(trace, res.trace[:-1])
        else:
            assert np.max(np.abs(trace - res.trace[:-1]) / np.abs(res.trace[:-1])) <= 1e-10
    # the first restated steps from the same guess: the same trace
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, dt_max, recursive=recursive)
    _, want = cr.run(er.from_vector(guess, N, kind, dt_max), pr, Q_BERNOULLI, 3, *cr.NET_START, exact=False)
    assert np.max(np.abs(res.trace[:3] - want) / np.maximum(1.0, np.abs(want))) <= 1e-9


@pytest.mark.parametrize("kind,dt_max,recursive", [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)])
def test_resuming_continues_the_run(nhp, kind, dt_max, recursive, monkeypatch):
    """init=res: 6 + 6 updates are 12 updates, under the equality rule of the run against its steps."""
    N = 7
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    guess = case["proc"].params()
    exact_rec = _fixed_order_recursion(monkeypatch, kind, recursive)
    fresh = lambda: _network(nhp, random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"])
    for route, on_slices in _routes(monkeypatch, nhp, case["proc"], case["data"]):
        kw = dict(f_abstol=0.0, recursive=recursive)
        whole = nhp.vb_(fresh(), case["data"], max_steps=12, guess=guess, **kw)
        first = nhp.vb_(fresh(), case["data"], max_steps=6, guess=guess, **kw)
        proc = fresh()
        second = nhp.vb_(proc, case["data"], max_steps=6, init=first, **kw)
        assert second.steps == 6 and len(second.trace) == 7 and np.array_equal(_device_guess(proc), second.mean())
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        _same(second, whole, exact, (kind, route))
        joined = np.concatenate([first.trace, second.trace[1:]])
        if exact:
            assert second.trace[0] == first.trace[-1] and np.array_equal(joined, whole.trace)
        else:
            assert np.max(np.abs(joined - whole.trace) / np.abs(whole.trace)) <= 1e-10


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_step_with_one_node(nhp, kind, monkeypatch):
    case = random_case(1, 200, 40.0, kind, 1.0, seed=5, nhp=nhp)
    proc = _network(nhp, case["proc"])
    for route, _ in _routes(monkeypatch, nhp, proc, case["data"]):
        got, want, _, _ = _one_step(nhp, proc, case["data"], kind, 1.0, False, f"{kind} N=1 {route}")
        assert got.rho.shape == (1, 1) and got.net_alpha + got.net_beta == pytest.approx(sum(cr.NET) + 1.0, rel=1e-15)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_step_with_ties_and_a_node_without_events(nhp, kind, monkeypatch):
    """tests/test_cont_vb_gpu.py's tied dataset.  The node without events keeps both priors on its row and column; on its row
    (cnt = 0 too) the logit is the network's term plus prior terms that cancel to rounding: ρv = sigmoid(ψ(αv) - ψ(βv)) within
    the link layer's bound, and as the restatement has it."""
    case = random_case(7, 1500, 150.0, kind, 1.0, seed=13, nhp=nhp)
    proc = _network(nhp, case["proc"])
    data = (np.round(case["times"]), np.where(case["nodes"] == 4, 5, case["nodes"]), case["T"])
    net = dn.sigmoid(digamma(cr.NET_START[0]) - digamma(cr.NET_START[1]))
    for route, _ in _routes(monkeypatch, nhp, proc, data, chunk=None):
        got, want, pr, _ = _one_step(nhp, proc, data, kind, 1.0, False, f"{kind} ties {route}")
        assert pr.cnt[3] == 0
        assert got.alpha[3] == PRIORS["alpha0"] and got.beta[3] == PRIORS["beta0"] + case["T"]
        for tab, prior in ((got.kappa, PRIORS["kappa"]), (got.kappa0, cr.SPIKE[0])):
            assert np.all(tab[3] == prior) and np.all(tab[:, 3] == prior)
        assert np.all(got.nu[3] == PRIORS["nu"]) and np.all(got.nu0[3] == cr.SPIKE[1])
        assert np.all(np.abs(got.rho[3] - net) <= cr.measured_logit_error())
        assert np.all(np.abs(got.rho[3] - want["rho"][3]) <= cr.measured_logit_error())


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("M", [0, 1])
def test_no_event_and_one_event(nhp, kind, M):
    case = random_case(4, 10, 20.0, kind, 1.0, seed=2, nhp=nhp)
    proc = _network(nhp, case["proc"])
    data = (case["times"][:M], case["nodes"][:M], case["T"])
    for recursive in (False, True):
        got, want, pr, _ = _one_step(nhp, proc, data, kind, 1.0, recursive, f"{kind} M={M} rec={recursive}")
        assert np.all(got.kappa == PRIORS["kappa"]) and np.all(got.kappa0 == cr.SPIKE[0]) and np.all(got.beta == PRIORS["beta0"] + 20.0)
        if M == 0:
            assert got.pieces["loglam"] == 0.0 and np.all(got.alpha == PRIORS["alpha0"]) and np.all(got.nu0 == cr.SPIKE[1])
    res = nhp.vb_(proc, data, max_steps=3, f_abstol=0.0, recursive=False)
    assert res.steps == 3 and np.all(np.isfinite(res.trace)) and np.min(np.diff(res.trace)) >= -1e-11 * abs(res.elbo)
    assert np.all(res.kappa == PRIORS["kappa"]) and np.all(np.isfinite(res.rho))


def test_saturating_and_symmetric_links(nhp):
    """N = 3 at 300 events: the busiest link has EM near 50.  A spike of tiny mean (0.3, 3e4) drives it to ρv = 1 exactly (its
    logit is past 37) and a slab that cannot explain it (κ1 = 0.3, ν1 = 3e4 against a spike (1.5, 2)) below 1e-3, without NaN.
    Symmetric priors (spike = slab) give ρv = sigmoid(ψ(αv) - ψ(βv)) exactly on every link."""
    N, kind = 3, "exponential"
    case = random_case(N, 300, 30.0, kind, 1.5, seed=3, nhp=nhp)
    state = cr.random_state(N, kind, 1)
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, 1.5)
    for spike, slab, check in (((0.3, 3e4), (1.5, 2.0), lambda r: r == 1.0), ((1.5, 2.0), (0.3, 3e4), lambda r: r < 1e-3)):
        q = cr.priors(spike=spike, base=dict(PRIORS, kappa=slab[0], nu=slab[1]))
        want, _, stats = cr.step(cr.surrogate(state, 1.5), pr, q, state["na"], state["nb"])
        p, c = np.unravel_index(np.argmax(stats[2]), (N, N))
        assert stats[2][p, c] >= 40.0
        proc = _network(nhp, random_case(N, 300, 30.0, kind, 1.5, seed=3, nhp=nhp)["proc"], q)
        got = nhp.update_(proc, case["data"], init=_state_object(nhp, state, kind, N, q), recursive=False)
        print(f"spike {spike} slab {slab}: EM {stats[2][p, c]:.1f}, ρv {got.rho[p, c]!r} (restated {want['rho'][p, c]!r})")
        assert np.all(np.isfinite(got.rho)) and np.all(np.isfinite(got.pieces["after"])) and check(got.rho[p, c]) and check(want["rho"][p, c])
        _check_state(got, want, f"saturating {spike}")
        _check_pieces(got.pieces["after"], want, pr.cnt, pr.T, q, f"saturating {spike}")
    q = cr.priors(spike=(PRIORS["kappa"], PRIORS["nu"]))
    proc = _network(nhp, random_case(N, 300, 30.0, kind, 1.5, seed=3, nhp=nhp)["proc"], q)
    got = nhp.update_(proc, case["data"], init=_state_object(nhp, state, kind, N, q), recursive=False)
    assert np.array_equal(got.kappa0, got.kappa) and np.array_equal(got.nu0, got.nu)
    # the device's own ψ(αv) - ψ(βv): nhp_digamma_lgamma at (2, 3) against scipy's, a few ulp of the logit
    net = digamma(cr.NET_START[0]) - digamma(cr.NET_START[1])
    assert np.all(got.rho == got.rho[0, 0]) and abs(got.rho[0, 0] - dn.sigmoid(net)) <= 8 * EPS


@pytest.mark.parametrize("kind,recursive", [("exponential", False), ("exponential", True), ("logitnormal", False)])
def test_three_trials_are_the_sum_of_their_statistics(nhp, kind, recursive):
    N, dt_max, q = 4, 1.5, Q_BERNOULLI
    trials = []
    for s, (M, T) in enumerate(((300, 30.0), (180, 25.0), (40, 12.0))):
        c = random_case(N, M, T, kind, dt_max, seed=20 + s, nhp=nhp)
        trials.append((c["times"] + (0.0 if not recursive else 1e-3), c["nodes"], T + 1.0))
    proc = _network(nhp, random_case(N, 10, 10.0, kind, dt_max, seed=1, nhp=nhp)["proc"])
    state = cr.random_state(N, kind, seed=6)
    model = cr.surrogate(state, dt_max)
    parts = [(er.statistics(model, p), p) for p in (er.Pairs(t, n, T, N, dt_max, recursive=recursive) for t, n, T in trials)]
    summed = [sum(s[i] for s, _ in parts) if parts[0][0][i] is not None else None for i in range(5)]
    cnt, T = sum(p.cnt for _, p in parts), sum(p.T for _, p in parts)
    want = cr.update(model, summed, cnt, T, q, state["na"], state["nb"])
    got = nhp.update_(proc, trials, init=_state_object(nhp, state, kind, N, q), recursive=recursive)
    worst = _check_state(got, want, f"{kind} trials rec={recursive}")
    print(f"{kind} three trials recursive={recursive}: largest error / bound = {worst:.3e}")
    assert np.all(got.beta == q["beta0"] + T)
    _check_pieces(got.pieces["after"], want, cnt, T, q, f"{kind} trials")
    _check_link_layer(got, (state["na"], state["nb"]), q, f"{kind} trials")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_a_step_on_device_planes_is_the_step_on_host_planes(nhp, kind):
    """output_on_device = 1: S, R and Q are device pointers, read and overwritten; the same numbers as through host arrays
    (within the factor bound: this dataset's route adds with LDS atomics), the same eleven scalars likewise."""
    import torch
    from nhp_amd import _lib, inference
    N, q = 5, Q_BERNOULLI
    case = random_case(N, 600, 60.0, kind, 1.0, seed=8, nhp=nhp)
    proc = _network(nhp, case["proc"])
    state = _state_object(nhp, cr.random_state(N, kind, 3), kind, N, q)
    host = nhp.update_(proc, case["data"], init=state, recursive=False)
    ctx = nhp.default_context()
    dev = torch.device("cuda", ctx.device)
    dS, dR, dQ = (torch.as_tensor(v).to(dev) for v in (state.S, state.R, state.Q))
    torch.cuda.current_stream(dev).synchronize()
    stats = np.empty(11)
    pr, netp, dense = inference._netvb_check(proc, case["data"], "update!")
    ds, model = nhp.device_dataset(proc, case["data"], ctx), proc.device_model(ctx)
    _lib.check(_lib.lib().nhp_cont_netvb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), _lib.dptr(netp), dS.data_ptr(), dR.data_ptr(), len(state.S),
                                              dQ.data_ptr(), 1, _lib.dptr(stats)), ctx.h)
    for g, w in ((dS.cpu().numpy(), host.S), (dR.cpu().numpy(), host.R), (dQ.cpu().numpy(), host.Q)):
        assert _ratio(g, w) <= 1.0
    want = np.array([host.pieces["loglam"], *host.pieces["before"], *host.pieces["after"]])
    assert np.array_equal(stats[1:6], want[1:6])                     # the pieces of the state stepped from: no statistics in them
    assert np.max(np.abs(stats - want) / np.maximum(1.0, np.abs(want))) <= 1e-10


def test_refusals_of_the_device_entry_points(nhp):
    """nhp_cont_netvb_step / nhp_cont_netvb_run themselves: NHP_ENOTIMPL (6) for a model without A, an LGCP baseline, a column
    shard and a block or latent distance network attached to the model; NHP_EINVAL (1) for missing priors or net, a hyper-parameter, network parameter or
    entry of the state that cannot be; NHP_ESHAPE (3) for a wrong length -- and nothing written."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    good = lambda: _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)
    N = 3
    NN = N * N

    def calls(proc, data, pr, net=(0.3, 30.0, 1.5, 2.5), P=None, flags=0, edit=None, ds_h=None):
        model = proc.device_model(ctx)
        ds = nhp.device_dataset(proc, data, ctx) if ds_h is None else None
        ds_h = ds.h if ds_h is None else ds_h
        P = N + 2 * NN if P is None else P
        S, R, x, stats = np.full(P, 7.0), np.full(P, 7.0), np.full(P, 0.5), np.full(11, 7.0)
        Q = np.concatenate([np.full(2 * NN, 7.0), np.full(NN, 0.5), [2.0, 3.0]])
        if edit:
            edit(S, R, Q)
        keep = [v.copy() for v in (S, R, Q, x, stats)]
        netp = None if net is None else np.array(net, dtype=np.float64)
        e, st, cv = C.c_double(), C.c_int32(), C.c_int32()
        prp = C.byref(pr) if pr is not None else None
        rc = (lib.nhp_cont_netvb_step(ctx.h, ds_h, model.h, flags, prp, _lib.dptr(netp), S.ctypes.data, R.ctypes.data, P, Q.ctypes.data, 0,
                                      _lib.dptr(stats)),
              lib.nhp_cont_netvb_run(ctx.h, ds_h, model.h, flags | 256, prp, _lib.dptr(netp), 1e-6, 5, _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P,
                                     _lib.dptr(Q), C.byref(e), C.byref(st), C.byref(cv), None))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, (S, R, Q, x, stats)))
        return rc
    std = random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    net = _network(nhp, random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    data = std["data"]
    lgcp = random_case(N, 50, 10.0, "exponential", 1.0, lgcp=True, seed=1, nhp=nhp)
    lgcp_net = nhp.ContinuousNetworkHawkesProcess(lgcp["proc"].baseline, lgcp["proc"].impulses, net.weights, np.ones((N, N)), net.network)
    assert calls(std["proc"], data, good()) == (6, 6)                # no adjacency matrix
    assert calls(lgcp_net, lgcp["data"], good()) == (6, 6)
    assert calls(net, data, None) == (1, 1) and calls(net, data, good(), net=None) == (1, 1)
    for field in ("alpha0", "beta0", "kappa", "nu", "a", "b"):
        for bad in (0.0, -1.0, np.nan, np.inf):
            pr = good()
            setattr(pr, field, bad)
            assert calls(net, data, pr) == (1, 1), (field, bad)
    for j in range(4):
        for bad in (0.0, -1.0, np.nan, np.inf):
            netp = [0.3, 30.0, 1.5, 2.5]
            netp[j] = bad
            assert calls(net, data, good(), net=netp) == (1, 1), (j, bad)
            if j >= 2:                                               # a dense network ignores α, β: these calls would run
                continue
            assert calls(net, data, good(), net=netp, flags=1024) == (1, 1)

    def put(plane, at, v):
        def edit(S, R, Q):
            {"S": S, "R": R, "Q": Q}[plane][at] = v
        return edit
    for bad in (0.0, -1.0, np.nan, np.inf):
        for plane, at in (("Q", 3 * NN), ("Q", 3 * NN + 1), ("Q", 0), ("Q", 2 * NN - 1), ("S", N + NN), ("R", N + 2 * NN - 1)):
            assert calls(net, data, good(), edit=put(plane, at, bad)) == (1, 1), (plane, at, bad)
    for bad in (-1e-9, 1.0 + 1e-9, np.nan):
        assert calls(net, data, good(), edit=put("Q", 2 * NN + 4, bad)) == (1, 1)
    assert calls(net, data, good(), P=20) == (3, 3)
    # a block network attached to the device model, as mcmc_ attaches it
    blocks = nhp.StochasticBlockNetworkModel(N, 2)
    sbm = nhp.ContinuousNetworkHawkesProcess(net.baseline, net.impulses, net.weights, np.ones((N, N)), blocks)
    z = np.ascontiguousarray(blocks.z, dtype=np.int32)
    _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, sbm.device_model(ctx).h, blocks.nblocks, z.ctypes.data, _lib.dptr(_lib.colmajor(blocks.ρ)),
                                          _lib.dptr(_lib.f64(blocks.π)), blocks.α, blocks.β, blocks.γ), ctx.h)
    assert calls(sbm, data, good()) == (6, 6)
    # ... and a latent distance network
    lat = _network(nhp, random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    _lib.check(lib.nhp_cont_model_set_latent(ctx.h, lat.device_model(ctx).h, 2, _lib.dptr(_lib.colmajor(np.zeros((N, 2)))), 0.1, 1.0, 0.0, 1.0),
               ctx.h)
    assert calls(lat, data, good()) == (6, 6)
    # a column shard (the children on nodes 1 and 2 of 3): it would be fitted on its own columns alone
    times, nodes, T = data
    h = C.c_void_p()
    _lib.check(lib.nhp_cont_dataset_create_columns(ctx.h, _lib.dptr(_lib.f64(times)), _lib.iptr(np.ascontiguousarray(nodes, dtype=np.int64)),
                                                   len(times), N, T, 1.0, 0, 2, C.byref(h)), ctx.h)
    try:
        assert calls(net, data, good(), ds_h=h) == (6, 6)
        assert calls(net, data, good(), flags=1024, ds_h=h) == (6, 6)
    finally:
        lib.nhp_cont_dataset_destroy(h)


def test_a_refused_step_leaves_the_host_planes_alone(nhp):
    """nhp_cont_netvb_step itself on host planes, N = 2 and three events, from a state whose baseline shapes are 1e-300: the
    surrogate λ̃0 = exp(ψ(α') - log β') underflows to zero, the first event has no parent, so its intensity is zero:
    NHP_EDOMAIN (2), and S, R, Q are byte for byte what was passed in."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    N = 2
    NN = N * N
    case = random_case(N, 3, 2.0, "exponential", 1.0, seed=1, nhp=nhp)
    proc = _network(nhp, case["proc"])
    P = N + 2 * NN
    S, R, stats = np.full(P, 2.0), np.full(P, 1.5), np.full(11, 7.0)
    Q = np.concatenate([np.full(NN, 0.5), np.full(NN, 20.0), np.full(NN, 0.5), [2.0, 3.0]])
    S[:N] = 1e-300
    keep = S.tobytes(), R.tobytes(), Q.tobytes()
    pr, netp = _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0), np.array([0.3, 30.0, 1.0, 1.0])
    ds, model = nhp.device_dataset(proc, case["data"], ctx), proc.device_model(ctx)
    rc = lib.nhp_cont_netvb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), _lib.dptr(netp), S.ctypes.data, R.ctypes.data, P, Q.ctypes.data, 0,
                                 _lib.dptr(stats))
    assert rc == 2
    assert (S.tobytes(), R.tobytes(), Q.tobytes()) == keep


def test_the_example_runs():
    truth_A, res, events = importlib.import_module("continuous_exponential_network_hawkes_vb").main()
    assert np.all(np.isfinite(res.trace)) and np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo))
    present = truth_A == 1.0
    enough = events >= 300.0                                          # the example's "enough" for its seed (its docstring)
    assert present.sum() == 8 and (present & enough).sum() == 8
    print(f"{res.steps} updates ({res.status}); smallest ρv of a present link {res.rho[present].min():.3f}, largest of an absent one {res.rho[~present].max():.3f}")
    assert np.all(res.rho[present & enough] > 0.5) and np.all(res.rho[~present] < 0.5)
