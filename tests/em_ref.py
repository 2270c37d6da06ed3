"""numpy restatement of the EM fit's E-step and M-step, written from their definition (include/nhp.h, nhp_cont_em_stats /
nhp_cont_em_run), not from the kernels.  The objective is the reference's

    ll = -T Σ λ0 - Σ_p cnt_p Σ_c W[p,c] + Σ_i log λ_i,     λ_i = λ0[c_i] + Σ_j W[n_j,c_i]·ħ_{n_j,c_i}(t_i - t_j)

over the pairs the chosen formulation sums: windowed, the earlier events (j < i) with t_j > t_i - Δtmax (oracle/nhp_oracle.c,
total_intensity); recursive (exponential impulses), every earlier event whatever Δtmax is.  With r_ij = W·ħ/λ_i and
r_i0 = λ0/λ_i the statistics are bg[c] = Σ r_i0, EM[p,c] = Σ r_ij, S1 = Σ r·Δt (exponential) | Σ r·z, z = logit(Δt/Δtmax)
(logit-normal), S2 = Σ r·(z - μ[p,c])² (logit-normal, centred at the current μ).  exact=True: one math.fsum per value;
exact=False: numpy's sums (bincount), for runs of thousands of iterations.  Test code only."""
import math

import numpy as np
from scipy.special import gammaln

from compensator_ref import Model  # noqa: F401  (plain arrays: lam0, W, theta | mu, tau, dt_max; matrices [parent, child])

LOWER, UPPER = 1e-6, 10.0


class Pairs:
    """The (child event i, parent event j) pairs of a dataset under one formulation, listed once."""

    def __init__(self, times, nodes, T, N, dt_max, recursive=False):
        self.times, self.nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
        self.T, self.N, self.M = float(T), int(N), len(self.times)
        t = self.times
        idx = np.arange(self.M)
        if recursive:
            first = np.zeros(self.M, np.int64)
        else:       # first j with t_j > t_i - Δtmax (never past i)
            first = np.minimum(np.searchsorted(t, t - dt_max, side="right"), idx)
        n = idx - first
        self.i = np.repeat(idx, n)
        self.j = (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)) + np.repeat(first, n)
        self.dt = t[self.i] - t[self.j]
        self.p, self.c = self.nodes0[self.j], self.nodes0[self.i]
        self.key = self.p * self.N + self.c
        self.cnt = np.bincount(self.nodes0, minlength=self.N).astype(float)
        if np.isfinite(dt_max):
            x = self.dt / dt_max
            self.ok = (x > 0.0) & (x < 1.0)
            self.xs = np.where(self.ok, x, 0.5)
            self.z = np.log(self.xs / (1.0 - self.xs))


def _group_sum(keys, vals, n, exact):
    if not exact:
        return np.bincount(keys, weights=vals, minlength=n).astype(float)
    out = np.zeros(n)
    if len(keys) == 0:
        return out
    order = np.argsort(keys, kind="stable")
    k, v = keys[order], vals[order]
    cut = np.flatnonzero(np.diff(k)) + 1
    for kk, seg in zip(k[np.concatenate([[0], cut])], np.split(v, cut)):
        out[kk] = math.fsum(seg)
    return out


def statistics(model, pr, exact=True):
    """(ll, bg [N], EM, S1, S2 [N, N] indexed [parent, child]; S2 None for exponential impulses) of `model` on the pairs `pr`."""
    N, M = pr.N, pr.M
    p, c = pr.p, pr.c
    if model.theta is not None:
        th = model.theta[p, c]
        h, s1 = th * np.exp(-th * pr.dt), pr.dt
    else:
        mu, tau = model.mu[p, c], model.tau[p, c]
        h = np.where(pr.ok, np.sqrt(tau / (2.0 * np.pi)) * np.exp(-0.5 * tau * (pr.z - mu) ** 2) / (pr.xs * (1.0 - pr.xs)), 0.0)
        s1 = pr.z
    term = model.W[p, c] * h
    base = model.lam0[pr.nodes0]
    lam = _group_sum(np.concatenate([pr.i, np.arange(M)]), np.concatenate([term, base]), M, exact)
    r = term / lam[pr.i]
    logs = np.log(lam)
    fixed = np.concatenate([-pr.T * model.lam0, (-pr.cnt[:, None] * model.W).ravel()])
    ll = math.fsum(np.concatenate([fixed, logs])) if exact else float(np.sum(fixed) + np.sum(logs))
    bg = _group_sum(pr.nodes0, base / lam, N, exact)
    EM = _group_sum(pr.key, r, N * N, exact).reshape(N, N)
    S1 = _group_sum(pr.key, r * s1, N * N, exact).reshape(N, N)
    S2 = None if model.theta is not None else _group_sum(pr.key, r * (pr.z - model.mu[p, c]) ** 2, N * N, exact).reshape(N, N)
    return ll, bg, EM, S1, S2


def _ratio(num, den, old):
    """The maximiser of num·log(v) - den·v on the box: a flat term keeps the old value, a non-positive numerator goes to
    the lower bound, a zero denominator under a positive numerator to the upper bound."""
    if num == 0.0 and den == 0.0:
        return old
    if not num > 0.0:
        return LOWER
    if not den > 0.0:
        return UPPER
    return min(max(num / den, LOWER), UPPER)


def mstep(model, stats, cnt, T, priors=None):
    """The closed-form M-step on the box [1e-6, 10] from the statistics of `model`; `priors`: None, or a dict with alpha0,
    beta0 (λ0), kappa, nu (W), a, b (θ | τ), mu_mu, kappa_mu (μ) for the modes of bound + log prior.  Returns a new Model."""
    _, bg, EM, S1, S2 = stats
    N = model.N
    q = priors
    lam0, W = np.empty(N), np.empty((N, N))
    exp_imp = model.theta is not None
    p1, p2 = np.empty((N, N)), np.empty((N, N))
    for c in range(N):
        lam0[c] = _ratio(bg[c], T, model.lam0[c]) if q is None else _ratio(bg[c] + q["alpha0"] - 1.0, T + q["beta0"], model.lam0[c])
    for p in range(N):
        for c in range(N):
            em = EM[p, c]
            W[p, c] = _ratio(em, cnt[p], model.W[p, c]) if q is None else _ratio(em + q["kappa"] - 1.0, cnt[p] + q["nu"], model.W[p, c])
            if exp_imp:
                p1[p, c] = _ratio(em, S1[p, c], model.theta[p, c]) if q is None else \
                    _ratio(em + q["a"] - 1.0, S1[p, c] + q["b"], model.theta[p, c])
                continue
            mu0 = model.mu[p, c]
            num, den = (S1[p, c], em) if q is None else (S1[p, c] + q["kappa_mu"] * q["mu_mu"], em + q["kappa_mu"])
            mu = min(max(num / den, LOWER), UPPER) if den > 0.0 else mu0
            d = mu - mu0
            V = max(S2[p, c] - 2.0 * d * (S1[p, c] - mu0 * em) + d * d * em, 0.0)      # Σ r (z - μ_new)²
            if q is None:
                tau = _ratio(em, V, model.tau[p, c])
            else:
                tau = _ratio(0.5 * em + q["a"] - 0.5, 0.5 * V + q["b"] + 0.5 * q["kappa_mu"] * (mu - q["mu_mu"]) ** 2, model.tau[p, c])
            p1[p, c], p2[p, c] = mu, tau
    kw = dict(theta=p1) if exp_imp else dict(mu=p1, tau=p2)
    return Model(lam0, W, model.dt_max, **kw)


def _gamma_logpdf(x, shape, rate):
    return shape * np.log(rate) - gammaln(shape) + (shape - 1.0) * np.log(x) - rate * x


def logprior(model, q):
    """inference.py::logprior on plain arrays."""
    lp = np.sum(_gamma_logpdf(model.lam0, q["alpha0"], q["beta0"])) + np.sum(_gamma_logpdf(model.W, q["kappa"], q["nu"]))
    if model.theta is not None:
        return float(lp + np.sum(_gamma_logpdf(model.theta, q["a"], q["b"])))
    prec = q["kappa_mu"] * model.tau
    lp += np.sum(_gamma_logpdf(model.tau, q["a"], q["b"]))
    return float(lp + np.sum(0.5 * np.log(prec / (2 * np.pi)) - 0.5 * prec * (model.mu - q["mu_mu"]) ** 2))


def params_vector(model):
    """[λ0; θ | μ; τ; W], matrices column-major (params(process))."""
    imp = [model.theta] if model.theta is not None else [model.mu, model.tau]
    return np.concatenate([model.lam0] + [m.ravel(order="F") for m in imp] + [model.W.ravel(order="F")])


def from_vector(x, N, kind, dt_max):
    x = np.asarray(x, float)
    m = [x[N + k * N * N:N + (k + 1) * N * N].reshape((N, N), order="F") for k in range(2 if kind == "exponential" else 3)]
    if kind == "exponential":
        return Model(x[:N], m[1], dt_max, theta=m[0])
    return Model(x[:N], m[2], dt_max, mu=m[0], tau=m[1])


def priors_of(proc):
    """The prior dict of one of the package's standard processes (inference.py::_priors)."""
    b, w, imp = proc.baseline, proc.weights, proc.impulses
    if hasattr(imp, "θ"):
        return dict(alpha0=b.α0, beta0=b.β0, kappa=w.κ, nu=w.ν, a=imp.α, b=imp.β, mu_mu=0.0, kappa_mu=1.0)
    return dict(alpha0=b.α0, beta0=b.β0, kappa=w.κ, nu=w.ν, a=imp.α0, b=imp.β0, mu_mu=imp.μμ, kappa_mu=imp.κμ)


def gradient(model, stats, cnt, T):
    """∇ll in params order from the statistics: the identities csrc/cont_em.hip uses, read backwards."""
    _, bg, EM, S1, S2 = stats
    g = [bg / model.lam0 - T]
    if model.theta is not None:
        g.append((EM / model.theta - S1).ravel(order="F"))
    else:
        g.append((model.tau * (S1 - model.mu * EM)).ravel(order="F"))
        g.append((0.5 * (EM / model.tau - S2)).ravel(order="F"))
    g.append((EM / model.W - cnt[:, None]).ravel(order="F"))
    return np.concatenate(g)


def projected(x, g):
    """The gradient with the components that point out of the box at a bound set to zero."""
    return np.where(((x <= LOWER) & (g < 0)) | ((x >= UPPER) & (g > 0)), 0.0, g)


def em(model, pr, max_steps, f_abstol, priors=None, exact=True):
    """The iteration of nhp_cont_em_run: (model at the last iterate, trace of the objective, converged)."""
    trace = []
    for k in range(max_steps + 1):
        st = statistics(model, pr, exact)
        trace.append(st[0] + (logprior(model, priors) if priors is not None else 0.0))
        if k > 0 and abs(trace[-1] - trace[-2]) < f_abstol:
            return model, np.array(trace), True
        if k == max_steps:
            break
        model = mstep(model, st, pr.cnt, pr.T, priors)
    return model, np.array(trace), False
