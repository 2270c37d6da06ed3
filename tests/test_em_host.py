"""The EM fit's definition, checked without a GPU: the numpy restatement (tests/em_ref.py) against the CPU oracle's
log-likelihood along its own iteration, the identities the statistics satisfy, the inputs of the GPU fit test, and the argument
errors raised before any device work."""
import numpy as np
import pytest

import em_ref as er
from helpers import random_case

PRIORS = dict(alpha0=2.0, beta0=1.5, kappa=1.5, nu=2.0, a=2.0, b=0.7, mu_mu=-0.5, kappa_mu=2.0)


def _oracle_model(orc, m):
    kw = dict(theta=m.theta) if m.theta is not None else dict(mu=m.mu, tau=m.tau)
    return orc.ContModel(m.lam0, m.W, dt_max=m.dt_max, **kw)


def _oracle_ll(orc, m, c, recursive):
    return orc.loglik(_oracle_model(orc, m), c["times"], c["nodes"], c["T"], recursive=recursive)


CASES = [("exponential", 0.5, False), ("exponential", 1.5, False), ("exponential", np.inf, False), ("exponential", np.inf, True),
         ("exponential", 1.5, True), ("logitnormal", 0.5, False), ("logitnormal", 1.5, False)]


@pytest.mark.parametrize("regularize", [False, True])
@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_restated_em_never_lowers_the_oracle_objective(nhp, orc, kind, dt_max, recursive, regularize):
    """50 restated iterations from a random start: the restatement's log-likelihood is the oracle's at every iterate, the
    oracle's objective (+ log prior) never falls by more than the project's log-likelihood parity tolerance 1e-11·max(1, |f|)
    (EM guarantees >= 0 in exact arithmetic), and the responsibilities of every event add up to one:
    Σ_p EM[p, c] + bg[c] = cnt_c to 1e-12·cnt_c."""
    N = 4
    c = random_case(N, 400, 40.0, kind, dt_max, seed=11, nhp=nhp)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive)
    q = PRIORS if regularize else None
    P = len(c["proc"].params())
    m = er.from_vector(np.random.default_rng(3).uniform(0.2, 0.8, P), N, kind, dt_max)
    prev, worst_drop, worst_ll, worst_sum = None, 0.0, 0.0, 0.0
    for k in range(51):
        st = er.statistics(m, pr)
        oll = _oracle_ll(orc, m, c, recursive)
        worst_ll = max(worst_ll, abs(st[0] - oll) / max(1.0, abs(oll)))
        f = oll + (er.logprior(m, q) if q else 0.0)
        if prev is not None:
            worst_drop = max(worst_drop, (prev - f) / max(1.0, abs(f)))
        prev = f
        worst_sum = max(worst_sum, np.max(np.abs(st[2].sum(axis=0) + st[1] - pr.cnt) / pr.cnt))
        m = er.mstep(m, st, pr.cnt, pr.T, q)
    print(f"{kind} dt_max={dt_max} recursive={recursive} priors={regularize}: f={prev:.6f} largest drop {worst_drop:.2e}, "
          f"|ll - oracle| {worst_ll:.2e}, responsibilities {worst_sum:.2e}")
    assert worst_ll <= 1e-11
    assert worst_drop <= 1e-11
    assert worst_sum <= 1e-12


@pytest.mark.parametrize("kind,dt_max,recursive", CASES)
def test_gradient_identities_against_central_differences_of_the_oracle(nhp, orc, kind, dt_max, recursive):
    """g_λ0 = bg/λ0 - T, g_W = EM/W - cnt_p, g_θ = EM/θ - ES, g_μ = τ·(EZ - μ·EM), g_τ = (EM/τ - S2)/2 -- the identities the
    device E-step reads backwards -- against central differences of the oracle's log-likelihood (step h = 1e-5: truncation
    ~h²·|f'''| ~ 1e-8, rounding ~ε·|ll|/h ~ 1e-8 at |ll| ~ 1e3, so 1e-6·max(1, |g|) leaves two digits), and against the
    oracle's analytic gradient at the project's gradient tolerance 1e-9."""
    N = 3
    c = random_case(N, 300, 40.0, kind, dt_max, seed=13, nhp=nhp, orc=orc)
    m = er.Model.of(c["proc"])
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive)
    g = er.gradient(m, er.statistics(m, pr), pr.cnt, pr.T)
    x = er.params_vector(m)
    fd = np.empty_like(x)
    h = 1e-5
    for i in range(len(x)):
        e = np.zeros_like(x)
        e[i] = h
        fd[i] = (_oracle_ll(orc, er.from_vector(x + e, N, kind, dt_max), c, recursive)
                 - _oracle_ll(orc, er.from_vector(x - e, N, kind, dt_max), c, recursive)) / (2 * h)
    err = np.max(np.abs(g - fd) / np.maximum(1.0, np.abs(fd)))
    _, wg = orc.loglik_grad(c["om"], c["times"], c["nodes"], c["T"], recursive=recursive)
    err_a = np.max(np.abs(g - wg) / np.maximum(1.0, np.abs(wg)))
    print(f"{kind} dt_max={dt_max} recursive={recursive}: against central differences {err:.2e}, against the analytic gradient {err_a:.2e}")
    assert err <= 1e-6
    assert err_a <= 1e-9


def test_mstep_rules_at_the_edges():
    """A node without events keeps its row of W and its impulse parameters (flat terms) and sends its λ0 to the lower bound;
    with priors the same coordinates go to the prior's mode; a clamped coordinate is exactly on the bound."""
    N = 3
    times = np.sort(np.random.default_rng(0).uniform(0, 30, 200))
    nodes = np.random.default_rng(1).integers(1, 3, 200)             # node 3 has no events
    m = er.Model(np.full(N, 0.5), np.full((N, N), 0.3), 1.0, theta=np.full((N, N), 2.0))
    pr = er.Pairs(times, nodes, 30.0, N, 1.0)
    st = er.statistics(m, pr)
    new = er.mstep(m, st, pr.cnt, pr.T)
    assert new.lam0[2] == er.LOWER
    assert np.array_equal(new.W[2], m.W[2]) and np.array_equal(new.theta[2], m.theta[2])      # cnt_p = 0: flat
    assert np.all(new.W[:2, 2] == er.LOWER) and np.array_equal(new.theta[:2, 2], m.theta[:2, 2])    # no children on node 3
    withp = er.mstep(m, st, pr.cnt, pr.T, PRIORS)
    assert withp.lam0[2] == pytest.approx((PRIORS["alpha0"] - 1) / (30.0 + PRIORS["beta0"]))
    assert np.allclose(withp.W[2], (PRIORS["kappa"] - 1) / PRIORS["nu"])
    assert np.allclose(withp.theta[2], (PRIORS["a"] - 1) / PRIORS["b"])
    empty = er.Pairs(np.zeros(0), np.zeros(0, np.int64), 30.0, N, 1.0)
    e = er.mstep(m, er.statistics(m, empty), empty.cnt, empty.T)
    assert np.all(e.lam0 == er.LOWER) and np.array_equal(e.W, m.W) and np.array_equal(e.theta, m.theta)


# restated iterations to |Δf| < 1e-9 observed on these inputs: exponential 5329, logit-normal 1363; max_steps is about twice that
@pytest.mark.parametrize("kind,max_steps", [("exponential", 11000), ("logitnormal", 2700)])
def test_restated_em_reaches_a_maximum_on_the_inputs_of_the_gpu_fit_test(nhp, kind, max_steps):
    """The case of tests/test_em_gpu.py::test_em_reaches_a_maximum (the generator and start of the device L-BFGS's test,
    windowed objective): the restated EM stopped at |Δf| < 1e-9 meets the project's "this is a maximum" bound on the
    projected gradient, max |pg| < 5e-2·sqrt(|ll|), within max_steps -- the method itself passes on these inputs before any
    device is involved.  (numpy sums, not fsum: thousands of iterations.  The recursive objective is left to the device
    test: its 4.5e6 pairs per iteration take minutes here.)"""
    N, dt_max = 5, 1.5
    c = random_case(N, 3000, 250.0, kind, dt_max, seed=31, nhp=nhp)
    guess = np.random.default_rng(5).uniform(0.2, 0.8, len(c["proc"].params()))
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max)
    m, trace, converged = er.em(er.from_vector(np.clip(guess, er.LOWER, er.UPPER), N, kind, dt_max), pr, max_steps, 1e-9, exact=False)
    st = er.statistics(m, pr, exact=False)
    x = er.params_vector(m)
    pg = er.projected(x, er.gradient(m, st, pr.cnt, pr.T))
    bound = 5e-2 * max(1.0, abs(trace[-1])) ** 0.5
    print(f"{kind}: {len(trace) - 1} iterations, ll {trace[0]:.3f} -> {trace[-1]:.6f}, max |pg| {np.max(np.abs(pg)):.3e} (bound {bound:.3f}), "
          f"smallest step {np.min(np.diff(trace)):.2e}")
    assert converged
    assert np.all(x >= er.LOWER) and np.all(x <= er.UPPER)
    assert np.max(np.abs(pg)) < bound
    assert np.min(np.diff(trace)) >= -1e-11 * max(1.0, abs(trace[-1]))


def test_argument_errors_are_raised_before_any_device_work(nhp):
    """Network process: TypeError; LGCP baseline and ShardedDataset: NotImplementedError; a guess of the wrong length: the
    reference's params! error -- none of them touches a device (this test runs without one)."""
    std = random_case(3, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    net = random_case(3, 50, 10.0, "exponential", 1.0, network=True, seed=1, nhp=nhp)
    lgcp = random_case(3, 50, 10.0, "exponential", 1.0, lgcp=True, seed=1, nhp=nhp)
    shard = object.__new__(nhp.ShardedDataset)
    for fn in (nhp.em_, nhp.expected_statistics):
        with pytest.raises(TypeError):
            fn(net["proc"], net["data"])
        with pytest.raises(NotImplementedError):
            fn(lgcp["proc"], lgcp["data"])
        with pytest.raises(NotImplementedError):
            fn(std["proc"], shard)
    with pytest.raises(ValueError, match="Parameter vector length"):
        nhp.em_(std["proc"], std["data"], guess=np.full(7, 0.5))
    with pytest.raises(TypeError):
        nhp.em_(nhp.DiscreteStandardHawkesProcess.__new__(nhp.DiscreteStandardHawkesProcess), std["data"])


def test_the_header_declares_the_em_entry_points():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nhp.h")).read()
    assert "nhp_status nhp_cont_em_stats(" in header and "nhp_status nhp_cont_em_run(" in header
