"""numpy restatements of forecast(process, data, horizon) (nhp_cont_forecast, include/nhp.h).

(a) `ensemble`: the law itself with numpy's own generator, vectorised over the replicas.  It takes the routes the device
    does not: per-(event, node) carry-over tables with inverse-CDF delays for logit-normal impulses (the device thins), and
    per-link Poisson counts for the exponential carry-over (the device merges a node's links and splits them again).
(b) `replay`: the documented Philox scheme, draw by draw: reproduces one call exactly (times to rounding).
`carry_expected` is the deterministic part both share."""
import math

import numpy as np

from test_simulate_gpu import U53, normal, poisson, u2

K_IMM_COUNT, K_CARRY_COUNT, K_ROOT = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB, 0x8EBC6AF09C88C6E3
K_CHILD_COUNT, K_CHILD = 0x589965CC75374CC3, 0x1D8E4E27C47D124F


class Model:
    """The arrays of a continuous process with a homogeneous baseline: λ0 [N], V = W∘A [N, N], θ | μ, τ, Δtmax."""

    def __init__(self, proc):
        self.lam0 = np.asarray(proc.baseline.λ, float)
        self.N = len(self.lam0)
        A = getattr(proc, "adjacency_matrix", None)
        W = np.asarray(proc.weights.W, float)
        self.V = W * np.asarray(A, float) if A is not None else W.copy()
        imp = proc.impulses
        self.expo = hasattr(imp, "θ")
        self.dt_max = float(imp.Δtmax)
        if self.expo:
            self.theta = np.asarray(imp.θ, float)
        else:
            self.mu, self.tau = np.asarray(imp.μ, float), np.asarray(imp.τ, float)
        self.G = np.cumsum(self.V, axis=1)                # sequential row prefix, the device's order of additions
        self.R = self.G[:, -1]


def _phi(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def cdf_ln(mu, tau, d, dt_max):
    """The logit-normal delay CDF: 0 for d <= 0, 1 from Δtmax on."""
    if not d > 0.0:
        return 0.0
    if not d < dt_max:
        return 1.0
    x = d / dt_max
    return _phi(math.sqrt(tau) * (math.log(x / (1.0 - x)) - mu))


def window_start(times, T0, dt_max):
    """The first event with T0 - t_j < Δtmax."""
    return int(np.searchsorted(-(T0 - np.asarray(times, float)), -dt_max, side="right"))


def exp_masses(m, times, nodes0, T0, h):
    """m[p, c] = V·G·(1 - e^{-θh}) with the state G[p, c] = Σ_{j on p} e^{-θ[p,c](T0 - t_j)}."""
    mass = np.zeros((m.N, m.N))
    for p in range(m.N):
        age = T0 - times[nodes0 == p]
        g = np.exp(-m.theta[p][None, :] * age[:, None]).sum(axis=0)
        mass[p] = m.V[p] * g * -np.expm1(-m.theta[p] * h)
    return np.where(m.V > 0.0, mass, 0.0)


def ln_masses(m, times, nodes0, T0, h):
    """(w0, mass [Wn, N]): mass[j - w0, c] = V[n_j, c]·(F(T0 + h - t_j) - F(T0 - t_j)) for the window events."""
    w0, Tend = window_start(times, T0, m.dt_max), T0 + h
    mass = np.zeros((len(times) - w0, m.N))
    for j in range(w0, len(times)):
        p = nodes0[j]
        for c in range(m.N):
            if m.V[p, c] > 0.0:
                mass[j - w0, c] = m.V[p, c] * (cdf_ln(m.mu[p, c], m.tau[p, c], Tend - times[j], m.dt_max)
                                               - cdf_ln(m.mu[p, c], m.tau[p, c], T0 - times[j], m.dt_max))
    return w0, mass


def carry_expected(proc, times, nodes, T0, h):
    """carry[c]: the expected number of carry-over events of node c in (T0, T0 + h]."""
    m = Model(proc)
    times, nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    if m.expo:
        return exp_masses(m, times, nodes0, T0, h).sum(axis=0)
    return ln_masses(m, times, nodes0, T0, h)[1].sum(axis=0)


# ---- (a) the law, numpy's generator ------------------------------------------------------------------------------------

def _delays(m, p, c, rng):
    if m.expo:
        return rng.exponential(1.0, len(p)) / m.theta[p, c]
    z = rng.standard_normal(len(p))
    return m.dt_max / (1.0 + np.exp(-(m.mu[p, c] + z / np.sqrt(m.tau[p, c]))))


def ensemble(proc, times, nodes, T0, h, S, seed=0, return_events=False):
    """counts [S, N] of S independent continuations on (T0, T0 + h]; with return_events also (t, node, replica, carried),
    carried = the event is a carry-over child."""
    from scipy.special import ndtri
    m = Model(proc)
    rng = np.random.default_rng(seed)
    times, nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    N, Tend = m.N, T0 + h
    ts, ns, rs = [], [], []
    reps = np.arange(S)
    for c in range(N):                                    # new immigrants
        k = rng.poisson(m.lam0[c] * h, S)
        ts.append(T0 + h * (1.0 - rng.uniform(size=k.sum()))); ns.append(np.full(k.sum(), c)); rs.append(np.repeat(reps, k))
    n_imm = sum(len(x) for x in ts)
    if m.expo:                                            # carry-over, link by link
        mass = exp_masses(m, times, nodes0, T0, h)
        for p, c in zip(*np.nonzero(mass)):
            k = rng.poisson(mass[p, c], S)
            q = -math.expm1(-m.theta[p, c] * h)
            d = -np.log1p(-rng.uniform(size=k.sum()) * q) / m.theta[p, c]
            ts.append(T0 + d); ns.append(np.full(k.sum(), c)); rs.append(np.repeat(reps, k))
    else:                                                 # carry-over, event by event, delays by the inverse CDF
        w0, mass = ln_masses(m, times, nodes0, T0, h)
        for jj, c in zip(*np.nonzero(mass)):
            j, p = w0 + jj, nodes0[w0 + jj]
            k = rng.poisson(mass[jj, c], S)
            f0 = cdf_ln(m.mu[p, c], m.tau[p, c], T0 - times[j], m.dt_max)
            f1 = cdf_ln(m.mu[p, c], m.tau[p, c], Tend - times[j], m.dt_max)
            u = f0 + (f1 - f0) * rng.uniform(size=k.sum())
            d = m.dt_max / (1.0 + np.exp(-(m.mu[p, c] + ndtri(u) / math.sqrt(m.tau[p, c]))))
            ts.append(np.clip(times[j] + d, np.nextafter(T0, np.inf), Tend)); ns.append(np.full(k.sum(), c)); rs.append(np.repeat(reps, k))
    t, node, rep = np.concatenate(ts), np.concatenate(ns).astype(np.int64), np.concatenate(rs)
    carried = np.arange(len(t)) >= n_imm
    all_t, all_n, all_r, all_c = [t], [node], [rep], [carried]
    while len(t):                                         # descendants, generation by generation
        k = rng.poisson(m.R[node])
        p, pt, pr = np.repeat(node, k), np.repeat(t, k), np.repeat(rep, k)
        x = rng.uniform(size=len(p)) * m.R[p]
        c = np.minimum((m.G[p] > x[:, None]).argmax(axis=1), N - 1) if len(p) else p
        ct = pt + _delays(m, p, c, rng)
        keep = ct <= Tend
        t, node, rep = ct[keep], c[keep], pr[keep]
        all_t.append(t); all_n.append(node); all_r.append(rep); all_c.append(np.zeros(len(t), bool))
    t, node, rep = np.concatenate(all_t), np.concatenate(all_n), np.concatenate(all_r)
    counts = np.zeros((S, N), np.int64)
    np.add.at(counts, (rep, node), 1)
    return (counts, (t, node, rep, np.concatenate(all_c))) if return_events else counts


# ---- (b) the documented Philox scheme ----------------------------------------------------------------------------------

def _after(T0, d):
    t = T0 + d
    return t if t > T0 else float(np.nextafter(T0, np.inf))


def replay(proc, times, nodes, T0, h, S, seed):
    """(counts [S, N], times, nodes (1-based), offsets [S + 1]) of forecast(proc, (times, nodes, T0), h, S, seed)."""
    m = Model(proc)
    times, nodes0 = np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    N, Tend = m.N, T0 + h
    at, an, ar = [], [], []
    if m.expo:
        CP = np.cumsum(exp_masses(m, times, nodes0, T0, h), axis=0)        # sequential over p
        carry = CP[-1]
    else:
        for r in range(S):                                # generation 0: the window events, once per replica
            for j in range(window_start(times, T0, m.dt_max), len(times)):
                at.append(times[j]); an.append(int(nodes0[j])); ar.append(r)
    n_pro = len(at)
    kids = [poisson(m.R[an[i]], seed ^ K_CHILD_COUNT, 0, i) for i in range(n_pro)]
    roots = []                                            # (replica, node, carried) in root order
    for e in range(S * N):
        r, c = divmod(e, N)
        roots += [(r, c, False)] * poisson(m.lam0[c] * h, seed ^ K_IMM_COUNT, 0, e)
        if m.expo:
            roots += [(r, c, True)] * poisson(carry[c], seed ^ K_CARRY_COUNT, 0, e)
    for k, (r, c, carried) in enumerate(roots):
        ua, ub = u2(seed ^ K_ROOT, 0, k, 0)
        if not carried:
            t = _after(T0, ua * h)
        else:
            x = (ua - U53) * carry[c]
            p = int(np.searchsorted(CP[:, c], x, side="right"))
            if p == N:
                p = int(np.searchsorted(CP[:, c], x, side="left"))
            th = m.theta[p, c]
            t = _after(T0, min(-math.log1p(-(ub * -math.expm1(-(th * h)))) / th, h))
        at.append(t); an.append(c); ar.append(r)
    root_kids = [poisson(m.R[an[i]], seed ^ K_CHILD_COUNT, 1, i) for i in range(n_pro, len(at))]
    g0, g1, gen = 0, n_pro, 0
    while True:
        s, first_new = 0, len(at)
        for i, k in zip(range(g0, g1), kids):
            p = an[i]
            for _ in range(k):
                ua, ub = u2(seed ^ K_CHILD, gen, s, 0)
                x = (ua - U53) * m.R[p]
                c = int(np.searchsorted(m.G[p], x, side="right"))
                if c == N:
                    c = int(np.searchsorted(m.G[p], x, side="left"))
                if m.expo:
                    dt = -math.log(ub) / m.theta[p, c]
                else:
                    dt = m.dt_max / (1.0 + math.exp(-(m.mu[p, c] + normal(seed ^ K_CHILD, gen, s) / math.sqrt(m.tau[p, c]))))
                t = at[i] + dt
                if T0 < t <= Tend:
                    at.append(t); an.append(c); ar.append(ar[i])
                s += 1
        new_kids = [poisson(m.R[an[i]], seed ^ K_CHILD_COUNT, gen + 1, i) for i in range(first_new, len(at))]
        kids = root_kids + new_kids if gen == 0 else new_kids
        g0, g1, gen = g1, len(at), gen + 1
        if sum(kids) == 0:
            break
    t, node, rep = np.array(at[n_pro:], float), np.array(an[n_pro:], np.int64), np.array(ar[n_pro:], np.int64)
    order = np.argsort(t, kind="stable")
    order = order[np.argsort(rep[order], kind="stable")]
    counts = np.zeros((S, N), np.int64)
    np.add.at(counts, (rep, node), 1)
    offsets = np.concatenate([[0], np.cumsum(counts.sum(axis=1))]).astype(np.int64)
    return counts, t[order], node[order] + 1, offsets
