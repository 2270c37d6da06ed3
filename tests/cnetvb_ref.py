"""numpy/scipy restatement of the mean-field variational fit of the continuous NETWORK process (spike-and-slab weights under
a dense or Bernoulli network), written from its definition (include/nhp.h, nhp_cont_netvb_step / nhp_cont_netvb_run), not
from the kernels, on top of tests/em_ref.py's Pairs / statistics and tests/vb_ref.py's factors.

A state is vb_ref's dict, where kappa, nu are the SLAB's q(W | A = 1), plus kappa0, nu0 [N, N] (the spike's), rho [N, N]
(q(A = 1)) and na, nb (q(ρ) = Beta(na, nb)); matrices are indexed [parent, child].  Priors are vb_ref's dict (kappa, nu: the
slab) plus kappa0, nu0 (the spike) and `net` = (α, β) of the Bernoulli network's Beta prior, or None for a dense network
(rho ≡ 1, na / nb pass through).

The logit is written the cancellation-free way of tests/disc_netvb_ref.py (κv1 = κv0 + dk, νv1 = νv0 + dn, so neither bracket
is a difference of large numbers); `measured_logit_error()` is this file's own rounding error against 50-digit mpmath on the
shapes of the GPU tests.  Test code only."""
import math

import numpy as np
from scipy.special import digamma, gammaln

import disc_netvb_ref as dn
import em_ref as er
import vb_ref as vr

SPIKE = (0.3, 30.0)            # Gamma(0.3, 30): mean 0.01
NET = (1.5, 2.5)               # Beta prior of ρ
NET_START = (2.0, 3.0)         # (αv, βv) a random state starts with


def wpri(q):
    return (q["kappa0"], q["nu0"], q["kappa"], q["nu"])


def elogw(state):
    return (1.0 - state["rho"]) * (digamma(state["kappa0"]) - np.log(state["nu0"])) + state["rho"] * (digamma(state["kappa"]) - np.log(state["nu"]))


def surrogate(state, dt_max):
    """The ordinary parameter vector whose E-step gives q(z) of `state`, as an em_ref Model (no adjacency matrix)."""
    lam0 = np.exp(digamma(state["alpha"]) - np.log(state["beta"]))
    elw = elogw(state)
    ela = digamma(state["a"]) - np.log(state["a"])
    if "m" not in state:
        return er.Model(lam0, np.exp(elw + ela), dt_max, theta=state["a"] / state["b"])
    return er.Model(lam0, np.exp(elw + 0.5 * ela - 0.5 / state["k"]), dt_max, mu=state["m"].copy(), tau=state["a"] / state["b"])


def logit(state_new, na, nb, q):
    """logit ρv at the NEW (κv, νv) and the OLD network parameters (na, nb)."""
    return dn.logit(float(digamma(na) - digamma(nb)), wpri(q), state_new["kappa0"], state_new["nu0"], state_new["nu"])


def logit_mp(state_new, na, nb, q):
    return dn.logit_mp(na, nb, wpri(q), state_new["kappa0"], state_new["nu0"])


def update(model, stats, cnt, T, q, na, nb):
    """The update of every factor from the statistics taken at `model`, with (na, nb) the network parameters of the state
    stepped from."""
    st = vr.update(model, stats, cnt, T, q)
    EM, N = stats[2], model.N
    st["kappa0"] = q["kappa0"] + EM
    st["nu0"] = q["nu0"] + np.repeat(cnt[:, None], N, axis=1)
    if q["net"] is None:
        st.update(rho=np.ones((N, N)), na=na, nb=nb)
    else:
        rho = dn.sigmoid(logit(st, na, nb, q))
        st.update(rho=rho, na=q["net"][0] + math.fsum(rho.ravel()), nb=q["net"][1] + math.fsum((1.0 - rho).ravel()))
    return st


def _xlogx(v):
    return np.where(v > 0.0, v * np.log(np.where(v > 0.0, v, 1.0)), 0.0)


def kl_beta(a1, b1, a0, b0):
    s = digamma(a1 + b1)
    return (gammaln(a1 + b1) - gammaln(a1) - gammaln(b1)) - (gammaln(a0 + b0) - gammaln(a0) - gammaln(b0)) \
        + (a1 - a0) * (digamma(a1) - s) + (b1 - b0) * (digamma(b1) - s)


def pieces(state, cnt, T, q):
    """(E_q[compensator], KL_λ0, KL_W, KL_imp, KL_net) of a state, each one math.fsum over its entries."""
    rho = state["rho"]
    comp = math.fsum(np.concatenate([T * state["alpha"] / state["beta"],
                                     (cnt[:, None] * ((1.0 - rho) * state["kappa0"] / state["nu0"] + rho * state["kappa"] / state["nu"])).ravel()]))
    kl0 = math.fsum(vr.kl_gamma(state["alpha"], state["beta"], q["alpha0"], q["beta0"]))
    klw = math.fsum(((1.0 - rho) * vr.kl_gamma(state["kappa0"], state["nu0"], q["kappa0"], q["nu0"])
                     + rho * vr.kl_gamma(state["kappa"], state["nu"], q["kappa"], q["nu"])).ravel())
    if "m" in state:
        kli = math.fsum(vr.kl_normal_gamma(state["m"], state["k"], state["a"], state["b"], q["mu_mu"], q["kappa_mu"], q["a"], q["b"]).ravel())
    else:
        kli = math.fsum(vr.kl_gamma(state["a"], state["b"], q["a"], q["b"]).ravel())
    if q["net"] is None:
        return comp, kl0, klw, kli, 0.0
    na, nb = state["na"], state["nb"]
    s = digamma(na + nb)
    terms = _xlogx(rho) + _xlogx(1.0 - rho) - rho * (digamma(na) - s) - (1.0 - rho) * (digamma(nb) - s)
    klnet = math.fsum(np.concatenate([terms.ravel(), [kl_beta(na, nb, *q["net"])]]))
    return comp, kl0, klw, kli, klnet


def net_terms(state, q):
    """Σ of the magnitudes of the terms KL_net is added up from (the rounded-terms allowance of the GPU tests)."""
    if q["net"] is None:
        return 0.0
    rho, na, nb = state["rho"], state["na"], state["nb"]
    s = digamma(na + nb)
    per = np.abs(_xlogx(rho)) + np.abs(_xlogx(1.0 - rho)) + np.abs(rho * (digamma(na) - s)) + np.abs((1.0 - rho) * (digamma(nb) - s))
    a0, b0 = q["net"]
    beta = abs(gammaln(na + nb)) + abs(gammaln(na)) + abs(gammaln(nb)) + abs(gammaln(a0 + b0) - gammaln(a0) - gammaln(b0)) \
        + abs((na - a0) * (digamma(na) - s)) + abs((nb - b0) * (digamma(nb) - s))
    return float(np.sum(per) + beta)


def step(model, pr, q, na, nb, exact=True):
    """One update from the surrogate (or guess) `model`: (new state, Σ log λ̃ at `model`, the E-step's statistics)."""
    stats = er.statistics(model, pr, exact)
    return update(model, stats, pr.cnt, pr.T, q, na, nb), vr.loglam(model, stats, pr), stats


def elbo(state, pr, q, dt_max, exact=True):
    model = surrogate(state, dt_max)
    stats = er.statistics(model, pr, exact)
    return vr.loglam(model, stats, pr) - math.fsum(pieces(state, pr.cnt, pr.T, q))


def run(model, pr, q, steps, na, nb, exact=True):
    """`steps` updates from the guess `model` and the network parameters (na, nb): (final state, [L_1 .. L_steps])."""
    dt_max = model.dt_max
    trace = []
    state = None
    for k in range(steps + 1):
        stats = er.statistics(model, pr, exact)
        if state is not None:
            trace.append(vr.loglam(model, stats, pr) - math.fsum(pieces(state, pr.cnt, pr.T, q)))
        if k == steps:
            break
        state = update(model, stats, pr.cnt, pr.T, q, na, nb)
        na, nb = state["na"], state["nb"]
        model = surrogate(state, dt_max)
    return state, np.array(trace)


def planes(state):
    """(S, R, Q): vb_ref's planes (the slab in the W block) and Q = [κv0; νv0; ρv; αv; βv], matrices column-major."""
    f = lambda v: v.ravel(order="F")
    S, R = vr.planes(state)
    return S, R, np.concatenate([f(state["kappa0"]), f(state["nu0"]), f(state["rho"]), [state["na"], state["nb"]]])


def from_planes(S, R, Q, N, kind):
    st = vr.from_planes(S, R, N, kind)
    Q = np.asarray(Q, float)
    t = lambda j: Q[j * N * N:(j + 1) * N * N].reshape((N, N), order="F")
    st.update(kappa0=t(0), nu0=t(1), rho=t(2), na=float(Q[-2]), nb=float(Q[-1]))
    return st


def random_state(N, kind, seed, dense=False):
    """vb_ref's random positive state, a spike table, ρv uniform in [0.05, 0.95] and (αv, βv) = NET_START."""
    st = vr.random_state(N, kind, seed)
    rng = np.random.default_rng(seed + 1000)
    st.update(kappa0=rng.uniform(0.05, 12.0, (N, N)), nu0=rng.uniform(1.0, 60.0, (N, N)),
              rho=np.ones((N, N)) if dense else rng.uniform(0.05, 0.95, (N, N)), na=NET_START[0], nb=NET_START[1])
    return st


PRIORS = dict(alpha0=2.0, beta0=1.5, kappa=1.5, nu=2.0, a=2.0, b=0.7, mu_mu=0.5, kappa_mu=2.0)       # tests/test_cont_vb_gpu.py's, as the slab
SHAPES = [(3, 300, 30.0), (70, 2000, 100.0)]                                                          # its (N, M, T)


def priors(net=NET, spike=SPIKE, base=None):
    return dict(PRIORS if base is None else base, kappa0=spike[0], nu0=spike[1], net=net)


def parity_problem(N, M, T, kind, dt_max, recursive=False, seed=1):
    """The one-step problem of the GPU tests: helpers.random_case(seed=3)'s events, a random state, its surrogate and the
    restated step from it.  Returns (state, pairs, new state, Σ log λ̃, statistics)."""
    from helpers import random_case
    c = random_case(N, M, T, kind, dt_max, seed=3)
    state = random_state(N, kind, seed)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive and kind == "exponential")
    new, loglam, stats = step(surrogate(state, dt_max), pr, priors(), state["na"], state["nb"])
    return state, pr, new, loglam, stats


_MEASURED = []


def measured_logit_error():
    """max |logit - logit_mp| over every link of SHAPES, at the tables the restated step writes from the parity start (both
    impulse families, Δtmax = 1.5).  Computed once per process (20 000 links at 50 digits)."""
    if not _MEASURED:
        worst, q = 0.0, priors()
        for N, M, T in SHAPES:
            for kind in ("exponential", "logitnormal"):
                state, _, new, _, _ = parity_problem(N, M, T, kind, 1.5)
                worst = max(worst, float(np.max(np.abs(logit(new, state["na"], state["nb"], q) - logit_mp(new, state["na"], state["nb"], q)))))
        _MEASURED.append(worst)
    return _MEASURED[0]
