"""numpy restatement of the compensator, written from its definition (include/nhp.h, nhp_cont_compensator), not from the
kernels: Λ_c(t) = base_c(t) + Σ_{i: t_i < t} W[n_i,c]·A[n_i,c]·H_{n_i,c}(t - t_i), the exact time integral of the intensity
that intensity(process, data, t) evaluates, with

    H(d) = 1 - exp(-θ·min(d, Δtmax))                                   exponential impulses (cut, not renormalised)
    H(d) = Δtmax·Φ(√τ (logit(d/Δtmax) - μ)) for d < Δtmax, else Δtmax  logit-normal (pdf not divided by Δtmax, D11)

a homogeneous baseline λ0_c·t or the exact integral of the piecewise-linear interpolant of (grid_x, λ_c).  One
math.fsum per evaluation.  Test code only."""
import math

import numpy as np
from scipy.special import ndtr


class Model:
    """Plain arrays: lam0 [N] (or [N, G] with grid_x), W, A (or None), theta | (mu, tau), dt_max; matrices [parent, child]."""

    def __init__(self, lam0, W, dt_max, theta=None, mu=None, tau=None, A=None, grid_x=None):
        self.lam0, self.W, self.dt_max = np.asarray(lam0, float), np.asarray(W, float), float(dt_max)
        self.theta = None if theta is None else np.asarray(theta, float)
        self.mu = None if mu is None else np.asarray(mu, float)
        self.tau = None if tau is None else np.asarray(tau, float)
        self.WA = self.W if A is None else self.W * np.asarray(A, float)
        self.grid_x = None if grid_x is None else np.asarray(grid_x, float)
        self.N = self.W.shape[0]

    @classmethod
    def of(cls, proc):
        """From one of the package's continuous process objects."""
        imp, b = proc.impulses, proc.baseline
        gx = getattr(b, "x", None)
        lam0 = np.asarray(b.λ, float) if gx is None else np.vstack([np.asarray(y, float) for y in b.λ])
        kw = dict(theta=imp.θ) if hasattr(imp, "θ") else dict(mu=imp.μ, tau=imp.τ)
        return cls(lam0, proc.weights.W, imp.Δtmax, A=getattr(proc, "adjacency_matrix", None), grid_x=gx, **kw)

    def H(self, p, c, d):
        """∫₀^min(d,Δtmax) of the impulse pdf of link (p, c); p and d arrays (d > 0), c a scalar."""
        d = np.asarray(d, float)
        if self.theta is not None:
            return -np.expm1(-self.theta[p, c] * np.minimum(d, self.dt_max))
        inside = d < self.dt_max
        x = np.where(inside, d, 0.5 * self.dt_max) / self.dt_max
        z = np.sqrt(self.tau[p, c]) * (np.log(x / (1.0 - x)) - self.mu[p, c])
        return np.where(inside, self.dt_max * ndtr(z), self.dt_max)

    def V(self):
        """Saturated mass of every link: W·A·H(Δtmax)."""
        if self.theta is not None:
            return self.WA * -np.expm1(-self.theta * self.dt_max) if np.isfinite(self.dt_max) else self.WA.copy()
        return self.WA * self.dt_max

    def base(self, c, t):
        if self.grid_x is None:
            return self.lam0[c] * t
        x, y = self.grid_x, self.lam0[c]
        g = min(int(np.searchsorted(x, t, side="right")) - 1, len(x) - 2)          # cell [x_g, x_g+1] holding t
        cells = 0.5 * (x[1:g + 1] - x[:g]) * (y[1:g + 1] + y[:g])
        h = t - x[g]
        yt = (y[g + 1] * h + y[g] * (x[g + 1] - t)) / (x[g + 1] - x[g])
        return math.fsum(cells) + 0.5 * h * (y[g] + yt)

    def Lambda(self, c, t, times, nodes0):
        """Λ_c(t): every event with t_i < t, one fsum."""
        i = np.flatnonzero(times < t)
        p = nodes0[i]
        return self.base(c, t) + math.fsum(self.WA[p, c] * self.H(p, c, t - times[i]))


def _residuals(at, nodes0, N):
    res = np.empty_like(at)
    for c in range(N):
        k = np.flatnonzero(nodes0 == c)
        res[k] = np.diff(at[k], prepend=0.0)
    return res


def compensator(model, times, nodes, T):
    """(at_events [M], residuals [M], total [N]) of the definition, O(M²)."""
    times, nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    at = np.array([model.Lambda(nodes0[k], times[k], times, nodes0) for k in range(len(times))])
    total = np.array([model.Lambda(c, T, times, nodes0) for c in range(model.N)])
    return at, _residuals(at, nodes0, model.N), total


def at_events_slice(model, times, nodes, k0, k1):
    """at_events[k0:k1] in O(window + N) per event (finite Δtmax): the events older than Δtmax enter through a running
    per-node count vector times the saturated masses V[:, c]."""
    times, nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    V = model.V()
    ws = np.searchsorted(times, times[k0:k1] - model.dt_max, side="right")     # first event with t_i > t_k - Δtmax
    cnt = np.bincount(nodes0[:ws[0]], minlength=model.N).astype(float)
    out, w = np.empty(k1 - k0), ws[0]
    for j, k in enumerate(range(k0, k1)):
        while w < ws[j]:
            cnt[nodes0[w]] += 1.0
            w += 1
        c, t = nodes0[k], times[k]
        i = np.arange(ws[j], k)
        i = i[times[i] < t]
        p = nodes0[i]
        out[j] = model.base(c, t) + math.fsum(np.concatenate([cnt * V[:, c], model.WA[p, c] * model.H(p, c, t - times[i])]))
    return out


def total_closed_form(model, times, nodes, T):
    """Λ_c(T) = base_c(T) + countsᵀ·V corrected for the events within Δtmax of T (finite Δtmax)."""
    times, nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    V = model.V()
    j = int(np.searchsorted(times, T - model.dt_max, side="right"))
    cnt = np.bincount(nodes0[:j], minlength=model.N).astype(float)
    i = np.arange(j, len(times))
    i = i[times[i] < T]
    p = nodes0[i]
    return np.array([model.base(c, T) + math.fsum(np.concatenate([cnt * V[:, c], model.WA[p, c] * model.H(p, c, T - times[i])]))
                     for c in range(model.N)])


def ks_exp1(res):
    """(D, p) of the Kolmogorov-Smirnov test of `res` against Exp(1); p from the asymptotic series with Stephens' correction."""
    u = np.sort(-np.expm1(-np.asarray(res, float)))
    n = len(u)
    i = np.arange(1, n + 1)
    d = max(np.max(i / n - u), np.max(u - (i - 1) / n))
    x = d * (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n))
    k = np.arange(1, 101)
    p = 1.0 if x < 0.2 else 2.0 * float(np.sum((-1.0) ** (k - 1) * np.exp(-2.0 * k * k * x * x)))
    return d, min(1.0, max(0.0, p))


def gauss_legendre_total(f, breaks, c_count, sub=1, order=40):
    """∫ f over [breaks[0], breaks[-1]] by Gauss-Legendre panels split at `breaks` (each cut into `sub` sub-panels);
    f(q) -> [len(q), c_count]."""
    xg, wg = np.polynomial.legendre.leggauss(order)
    b = np.unique(np.asarray(breaks, float))
    if sub > 1:
        b = np.unique(np.concatenate([np.linspace(b[i], b[i + 1], sub + 1) for i in range(len(b) - 1)]))
    a, h = b[:-1], np.diff(b)
    keep = h > 0
    a, h = a[keep], h[keep]
    q = (a[:, None] + 0.5 * h[:, None] * (xg[None, :] + 1.0)).ravel()
    w = (0.5 * h[:, None] * wg[None, :]).ravel()
    vals = f(q)
    return np.array([math.fsum(w * vals[:, c]) for c in range(c_count)])
