"""numpy/scipy restatement of the mean-field variational fit of the continuous standard process, written from its definition
(include/nhp.h, nhp_cont_vb_step / nhp_cont_vb_run), not from the kernels, on top of tests/em_ref.py's Pairs / statistics.

A state is a dict of plain arrays: alpha, beta [N] (λ0 ~ Gamma), kappa, nu [N, N] (W ~ Gamma), a, b [N, N] (θ ~ Gamma, or τ of the
normal-gamma factor) and, for logit-normal impulses, m, k [N, N]; matrices are indexed [parent, child].  Priors are em_ref's
dict (alpha0, beta0, kappa, nu, a, b, mu_mu, kappa_mu).  Test code only."""
import math

import numpy as np
from scipy.special import digamma, gammaln

import em_ref as er


def surrogate(state, dt_max):
    """The ordinary parameter vector whose E-step gives q(z) of `state`, as an em_ref Model."""
    lam0 = np.exp(digamma(state["alpha"]) - np.log(state["beta"]))
    elw = digamma(state["kappa"]) - np.log(state["nu"])
    ela = digamma(state["a"]) - np.log(state["a"])
    if "m" not in state:
        return er.Model(lam0, np.exp(elw + ela), dt_max, theta=state["a"] / state["b"])
    return er.Model(lam0, np.exp(elw + 0.5 * ela - 0.5 / state["k"]), dt_max, mu=state["m"].copy(), tau=state["a"] / state["b"])


def update(model, stats, cnt, T, q):
    """The conjugate update of every factor from the statistics taken at `model` (a surrogate, or any parameter vector)."""
    _, bg, EM, S1, S2 = stats
    N = model.N
    st = dict(alpha=q["alpha0"] + bg, beta=np.full(N, q["beta0"] + T), kappa=q["kappa"] + EM,
              nu=q["nu"] + np.repeat(cnt[:, None], N, axis=1))
    if model.theta is not None:
        st.update(a=q["a"] + EM, b=q["b"] + S1)
        return st
    c = model.mu
    D1, d0 = S1 - c * EM, q["mu_mu"] - c
    k = q["kappa_mu"] + EM
    dm = (D1 + q["kappa_mu"] * d0) / k
    st.update(m=c + dm, k=k, a=q["a"] + 0.5 * EM, b=q["b"] + 0.5 * (S2 + q["kappa_mu"] * d0 ** 2 - k * dm ** 2))
    return st


def kl_gamma(a1, b1, a0, b0):
    return (a1 - a0) * digamma(a1) - gammaln(a1) + gammaln(a0) + a0 * (np.log(b1) - np.log(b0)) + a1 * (b0 - b1) / b1


def kl_normal_gamma(m, k, a, b, mu_mu, kappa_mu, a0, b0):
    return kl_gamma(a, b, a0, b0) + 0.5 * (kappa_mu / k - 1.0 + np.log(k / kappa_mu) + kappa_mu * (a / b) * (m - mu_mu) ** 2)


def pieces(state, cnt, T, q):
    """(E_q[compensator], KL_λ0, KL_W, KL_imp) of a state, each one math.fsum over its entries."""
    comp = math.fsum(np.concatenate([T * state["alpha"] / state["beta"], (cnt[:, None] * state["kappa"] / state["nu"]).ravel()]))
    kl0 = math.fsum(kl_gamma(state["alpha"], state["beta"], q["alpha0"], q["beta0"]))
    klw = math.fsum(kl_gamma(state["kappa"], state["nu"], q["kappa"], q["nu"]).ravel())
    if "m" in state:
        kli = math.fsum(kl_normal_gamma(state["m"], state["k"], state["a"], state["b"], q["mu_mu"], q["kappa_mu"], q["a"], q["b"]).ravel())
    else:
        kli = math.fsum(kl_gamma(state["a"], state["b"], q["a"], q["b"]).ravel())
    return comp, kl0, klw, kli


def loglam(model, stats, pr):
    """Σ_i log λ̃_i: the log-likelihood of em_ref.statistics with its -T Σ λ̃0 - Σ cnt_p Σ_c W̃ undone."""
    return math.fsum(np.concatenate([[stats[0]], pr.T * model.lam0, (pr.cnt[:, None] * model.W).ravel()]))


def step(model, pr, q, exact=True):
    """One update from the surrogate (or guess) `model`: (new state, Σ log λ̃ at `model`, the E-step's statistics)."""
    stats = er.statistics(model, pr, exact)
    return update(model, stats, pr.cnt, pr.T, q), loglam(model, stats, pr), stats


def elbo(state, pr, q, dt_max, exact=True):
    """The ELBO of a state with q(z) optimal for it."""
    model = surrogate(state, dt_max)
    stats = er.statistics(model, pr, exact)
    return loglam(model, stats, pr) - math.fsum(pieces(state, pr.cnt, pr.T, q))


def run(model, pr, q, steps, exact=True):
    """`steps` updates from the guess `model`: (final state, [L_1 .. L_steps])."""
    dt_max = model.dt_max
    trace = []
    state = None
    for k in range(steps + 1):
        stats = er.statistics(model, pr, exact)
        if state is not None:
            trace.append(loglam(model, stats, pr) - math.fsum(pieces(state, pr.cnt, pr.T, q)))
        if k == steps:
            break
        state = update(model, stats, pr.cnt, pr.T, q)
        model = surrogate(state, dt_max)
    return state, np.array(trace)


def planes(state):
    """(S, R) in params(process) order: [α'; a' | m', a'; κ'] and [β'; b' | k', b'; ν'], matrices column-major."""
    f = lambda v: v.ravel(order="F")
    if "m" in state:
        return (np.concatenate([state["alpha"], f(state["m"]), f(state["a"]), f(state["kappa"])]),
                np.concatenate([state["beta"], f(state["k"]), f(state["b"]), f(state["nu"])]))
    return (np.concatenate([state["alpha"], f(state["a"]), f(state["kappa"])]),
            np.concatenate([state["beta"], f(state["b"]), f(state["nu"])]))


def from_planes(S, R, N, kind):
    S, R = np.asarray(S, float), np.asarray(R, float)
    t = lambda v, j: v[N + j * N * N:N + (j + 1) * N * N].reshape((N, N), order="F")
    st = dict(alpha=S[:N], beta=R[:N])
    if kind == "exponential":
        st.update(a=t(S, 0), b=t(R, 0), kappa=t(S, 1), nu=t(R, 1))
    else:
        st.update(m=t(S, 0), k=t(R, 0), a=t(S, 1), b=t(R, 1), kappa=t(S, 2), nu=t(R, 2))
    return st


def random_state(N, kind, seed):
    """A random positive state (m of either sign)."""
    rng = np.random.default_rng(seed)
    st = dict(alpha=rng.uniform(0.5, 30.0, N), beta=rng.uniform(5.0, 40.0, N), kappa=rng.uniform(0.05, 12.0, (N, N)),
              nu=rng.uniform(1.0, 40.0, (N, N)), a=rng.uniform(0.3, 15.0, (N, N)), b=rng.uniform(0.3, 10.0, (N, N)))
    if kind != "exponential":
        st.update(m=rng.normal(0.0, 1.0, (N, N)), k=rng.uniform(0.2, 20.0, (N, N)))
    return st
