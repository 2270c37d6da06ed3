"""Reference for mean-field VB and SVI on a discrete network Hawkes process with spike-and-slab weights.

Model: A[p,c] ~ Bernoulli(ρ), W[p,c] | A = a ~ Gamma(κ_a, ν_a) (a = 0 the spike, a = 1 the slab), ρ ~ Beta(α, β); family
q(A[p,c] = 1) = ρv[p,c], q(W | A = a) = Gamma(κv_a, νv_a), the rest as in the dense step.  One update! reads the OLD
parameters for the factors and then updates baseline, weights, impulses, adjacency, network:

    ElogW = (1 - ρv)(ψ(κv0) - log νv0) + ρv (ψ(κv1) - log νv1)
    E[p,c,b] = exp(ψ(γv[p,c,b]) - ψ(Σ_b γv) + ElogW),   e0[c] = exp(ψ(αv[c]) - log βv[c])
    Z[t,c] = e0[c] + Σ_{p,b} Ŝ[t,p,b] E[p,c,b],   R = data/Z,   Γ[p,c,b] = E[p,c,b] Σ_t Ŝ[t,p,b] R[t,c]
    αv = α0 + e0 Σ_t R,  βv = 1/β0 + T dt,  γv = γ + Γ,  κv_a = κ_a + Σ_b Γ,  νv_a[p,c] = ν_a + Σ_t data[p,t]
    logit ρv = ψ(αv_net) - ψ(βv_net) + [κ1 log ν1 - lgamma κ1 + lgamma κv1 - κv1 log νv1]
                                      - [κ0 log ν0 - lgamma κ0 + lgamma κv0 - κv0 log νv0]      (new κv, νv; old network)
    αv_net = α + Σρv,  βv_net = β + Σ(1 - ρv)                                                   (all N² links)

`params` = (αv, βv, κv0, νv0, κv1, νv1, γv, ρv, αv_net, βv_net); `priors` = (α0, β0, κ0, ν0, κ1, ν1, γ); `net` = (α, β) of a
Bernoulli network or None for a dense one (ρv ≡ 1, the network parameters pass through).

`logit` is written as the library writes it (κv1 = κv0 + dk, νv1 = νv0 + dn with dk = κ1 - κ0, dn = ν1 - ν0, so neither
bracket is a difference of large numbers); `logit_mp` is the same function of (net, priors, κv0, νv0) in 50-digit
arithmetic, and `measured_logit_error()` is this file's own rounding error against it on the parity shapes of the GPU
tests (8.9e-15 where it was written); four times it is what the device logit is held to.  The `_brute` functions use
explicit loops over t, c, p, b, the literal formulas (scipy's gammaln, no rearrangement) and no oracle: for tiny shapes.
"""
import math

import numpy as np
from scipy.special import digamma, gammaln

import disc_svi_ref as sr


def stirling_tail(z):
    f = 1.0 / (z * z)
    return (1.0 / 12.0 + f * (-1.0 / 360.0 + f * (1.0 / 1260.0 + f * (-1.0 / 1680.0 + f * (1.0 / 1188.0))))) / z


def lgamma_diff(x, d):
    """lgamma(x + d) - lgamma(x): inside Stirling's formula once both arguments are >= 16, the library values below."""
    x = np.asarray(x, dtype=np.float64)
    y = x + d
    small = (x < 16.0) | (y < 16.0)
    xs, ys = np.where(small, 20.0, x), np.where(small, 20.0, y)
    big = ((xs - 0.5) * np.log1p(d / xs) + d * np.log(ys) - d) + (stirling_tail(ys) - stirling_tail(xs))
    return np.where(small, gammaln(y) - gammaln(x), big)


def prior_logit(k0, n0, k1, n1):
    return (k1 * math.log(n1) - math.lgamma(k1)) - (k0 * math.log(n0) - math.lgamma(k0))


def logit(net_term, wpri, kv0, nv0, nv1):
    k0, n0, k1, n1 = wpri
    dk, dn = k1 - k0, n1 - n0
    return ((net_term + prior_logit(*wpri)) + lgamma_diff(kv0, dk)) - (kv0 * np.log1p(dn / nv0) + dk * np.log(nv1))


def logit_mp(net_a, net_b, wpri, kv0, nv0):
    """The logit in 50-digit arithmetic at κv1 = κv0 + (κ1 - κ0), νv1 = νv0 + (ν1 - ν0) taken exactly; float64 array out."""
    import mpmath as mp
    mp.mp.dps = 50
    k0, n0, k1, n1 = (mp.mpf(v) for v in wpri)
    net = mp.digamma(mp.mpf(net_a)) - mp.digamma(mp.mpf(net_b))
    pri = (k1 * mp.log(n1) - mp.loggamma(k1)) - (k0 * mp.log(n0) - mp.loggamma(k0))
    out = np.empty(np.shape(kv0))
    for idx in np.ndindex(*out.shape):
        x0, m0 = mp.mpf(float(kv0[idx])), mp.mpf(float(nv0[idx]))
        x1, m1 = x0 + (k1 - k0), m0 + (n1 - n0)
        out[idx] = float(net + pri + (mp.loggamma(x1) - x1 * mp.log(m1)) - (mp.loggamma(x0) - x0 * mp.log(m0)))
    return out


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def rho_update(net, wpri, na, nb, kv0, nv0, nv1):
    if net is None:
        return np.ones_like(kv0)
    return sigmoid(logit(digamma(na) - digamma(nb), wpri, kv0, nv0, nv1))


def factors(params):
    av, bv, k0, n0, k1, n1, gv, rho = params[:8]
    elw = (1.0 - rho) * (digamma(k0) - np.log(n0)) + rho * (digamma(k1) - np.log(n1))
    E = np.exp(digamma(gv) - digamma(gv.sum(axis=2))[:, :, None] + elw[:, :, None])
    return E, np.exp(digamma(av) - np.log(bv))


def block_stats(data, conv, params, t0, t1):
    """(e0 Σ_t R, Γ) with the sums over t restricted to [t0, t1)."""
    E, e0 = factors(params)
    cv = conv[t0:t1]
    Z = e0[None, :] + np.einsum("tpb,pcb->tc", cv, E)
    R = data[:, t0:t1].T / Z
    return e0 * R.sum(axis=0), E * np.einsum("tpb,tc->pcb", cv, R)


def _finish(data, dt, priors, net, params, ah, gh, r):
    a0, b0, k0, n0, k1, n1, g = priors
    N, T = data.shape
    S = (gh - g).sum(axis=2)
    M = data.sum(axis=1).astype(np.float64)[:, None]
    k0h, k1h = k0 + S, k1 + S
    n0h, n1h = np.repeat(n0 + M, N, axis=1), np.repeat(n1 + M, N, axis=1)
    na, nb = params[8], params[9]
    rh = rho_update(net, (k0, n0, k1, n1), na, nb, k0h, n0h, n1h)
    bh = np.full(N, 1.0 / b0 + T * dt)
    if net is None:
        nah, nbh = na, nb
    else:
        nah, nbh = net[0] + rh.sum(), net[1] + (1.0 - rh).sum()
    hats = (ah, bh, k0h, n0h, k1h, n1h, gh, rh, nah, nbh)
    if r is None:
        return hats
    out = tuple(sr.blend(x, xh, r) for x, xh in zip(params, hats))
    return out if net is not None else out[:7] + (np.ones_like(rh), na, nb)


def netvb_step(data, conv, dt, priors, net, params):
    a_stat, G = block_stats(data, conv, params, 0, data.shape[1])
    return _finish(data, dt, priors, net, params, priors[0] + a_stat, priors[6] + G, None)


def netvb_run(data, conv, dt, priors, net, params, n):
    for _ in range(n):
        params = netvb_step(data, conv, dt, priors, net, params)
    return params


def netsvi_step(data, conv, dt, priors, net, params, j, Tb, i, delay, forgetting):
    T = data.shape[1]
    nblk = sr.n_blocks(T, Tb)
    t0, t1 = sr.block_bounds(T, Tb, j)
    a_stat, G = block_stats(data, conv, params, t0, t1)
    a0, g = priors[0], priors[6]
    ah = a0 + nblk * ((a0 + a_stat) - a0)
    gh = g + nblk * ((g + G) - g)
    return _finish(data, dt, priors, net, params, ah, gh, sr.rho(i, delay, forgetting))


def netsvi_run(data, conv, dt, priors, net, params, blocks, Tb, delay, forgetting, step0=0):
    for k, j in enumerate(blocks):
        params = netsvi_step(data, conv, dt, priors, net, params, int(j), Tb, step0 + k + 1, delay, forgetting)
    return params


# ---- brute force, no oracle, literal formulas ---------------------------------------------------------------------------

def netsvi_step_brute(data, L, dt, priors, net, params, j, Tb, i, delay, forgetting, vb=False):
    """One SVI step with explicit loops; vb=True gives one update! (one block, no scaling, no blend)."""
    a0, b0, k0, n0, k1, n1, g = priors
    av, bv, kv0, nv0, kv1, nv1, gv, rho, na, nb = params
    N, T = data.shape
    B = gv.shape[2]
    conv = sr.convolve_brute(data, sr.basis_brute(L, B, dt))
    nblk = 1 if vb else sr.n_blocks(T, Tb)
    t0, t1 = (0, T) if vb else sr.block_bounds(T, Tb, j)
    e0 = np.array([np.exp(digamma(av[c]) - np.log(bv[c])) for c in range(N)])
    E = np.empty((N, N, B))
    for p in range(N):
        for c in range(N):
            elw = (1.0 - rho[p, c]) * (digamma(kv0[p, c]) - np.log(nv0[p, c])) + rho[p, c] * (digamma(kv1[p, c]) - np.log(nv1[p, c]))
            for b in range(B):
                E[p, c, b] = np.exp(digamma(gv[p, c, b]) - digamma(gv[p, c, :].sum()) + elw)
    a_stat, g_stat = np.zeros(N), np.zeros((N, N, B))
    for t in range(t0, t1):
        for c in range(N):
            Z = e0[c]
            for p in range(N):
                for b in range(B):
                    Z += conv[t, p, b] * E[p, c, b]
            a_stat[c] += data[c, t] * e0[c] / Z
            for p in range(N):
                for b in range(B):
                    g_stat[p, c, b] += data[c, t] * conv[t, p, b] * E[p, c, b] / Z
    ah = a0 + nblk * a_stat
    gh = g + nblk * g_stat
    bh = np.full(N, 1.0 / b0 + T * dt)
    k0h, k1h, n0h, n1h, rh = (np.empty((N, N)) for _ in range(5))
    for p in range(N):
        Mp = sum(float(data[p, t]) for t in range(T))
        for c in range(N):
            S = sum(gh[p, c, b] - g for b in range(B))
            k0h[p, c], k1h[p, c], n0h[p, c], n1h[p, c] = k0 + S, k1 + S, n0 + Mp, n1 + Mp
            if net is None:
                rh[p, c] = 1.0
            else:
                lo = digamma(na) - digamma(nb)
                lo += k1 * np.log(n1) - gammaln(k1) + gammaln(k1h[p, c]) - k1h[p, c] * np.log(n1h[p, c])
                lo -= k0 * np.log(n0) - gammaln(k0) + gammaln(k0h[p, c]) - k0h[p, c] * np.log(n0h[p, c])
                rh[p, c] = 1.0 / (1.0 + np.exp(-lo))
    nah, nbh = (na, nb) if net is None else (net[0] + rh.sum(), net[1] + (1.0 - rh).sum())
    hats = (ah, bh, k0h, n0h, k1h, n1h, gh, rh, nah, nbh)
    if vb:
        return hats
    r = sr.rho(i, delay, forgetting)
    out = tuple(sr.blend(x, xh, r) for x, xh in zip(params, hats))
    return out if net is not None else out[:7] + (np.ones_like(rh), na, nb)


def netvb_step_brute(data, L, dt, priors, net, params):
    return netsvi_step_brute(data, L, dt, priors, net, params, 0, data.shape[1], 1, 0.0, 1.0, vb=True)


# ---- starts and data ----------------------------------------------------------------------------------------------------

def random_start(N, B, seed=5):
    """The start of tests/test_disc_svi_gpu.py widened: ρv random in (0.05, 0.95), network parameters in (0.5, 3)."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(0.5, 3.0, s)                                      # noqa: E731
    return (u(N), u(N), u(N, N), u(N, N), u(N, N), u(N, N), u(N, N, B), rng.uniform(0.05, 0.95, (N, N)),
            float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.5, 3.0)))


def ones_start(N, B, rho=0.5):
    o = np.ones((N, N))
    return np.ones(N), np.ones(N), o.copy(), o.copy(), o.copy(), o.copy(), np.ones((N, N, B)), np.full((N, N), rho), 1.0, 1.0


def counts(N, T, seed, rate=0.3):
    return np.random.default_rng(seed).poisson(rate, (N, T)).astype(np.int64)


# the parity shapes of tests/test_disc_netvb_gpu.py: (N, T, B, L)
PARITY = [(3, 50, 2, 4), (5, 700, 3, 7), (130, 300, 2, 3)]
PARITY_PRIORS = (1.0, 1.0, 0.5, 20.0, 2.0, 1.5, 1.0)        # spike Gamma(0.5, 20): mean 0.025; slab Gamma(2, 1.5)
PARITY_NET = (1.5, 2.5)

def convolve(data, phi):
    """convolve(process, data) in numpy: Ŝ[t, n, b] = Σ_{l=1..L} data[n, t-l] ϕ[l, b], lags added in increasing order."""
    N, T = data.shape
    L, B = phi.shape
    conv = np.zeros((T, N, B))
    for l in range(1, min(L, T - 1) + 1):
        conv[l:] += data[:, :T - l].T[:, :, None] * phi[l - 1][None, None, :]
    return np.maximum(conv, 0.0)


def parity_problem(N, T, B, L):
    data = counts(N, T, 7 * N)
    return data, convolve(data, sr.basis_brute(L, B, 1.0)), random_start(N, B)


_MEASURED = []


def measured_logit_error():
    """max |logit - logit_mp| over every link of the PARITY shapes, at the tables the first and the sixth step write from
    the parity start.  Computed once per process (2.5 s: 34 000 links at 50 digits)."""
    if not _MEASURED:
        worst = 0.0
        wp = PARITY_PRIORS[2:6]
        for shape in PARITY:
            data, conv, p = parity_problem(*shape)
            for step in range(6):
                q = netvb_step(data, conv, 1.0, PARITY_PRIORS, PARITY_NET, p)
                if step in (0, 5):
                    lo = logit(float(digamma(p[8]) - digamma(p[9])), wp, q[2], q[3], q[5])
                    worst = max(worst, float(np.max(np.abs(lo - logit_mp(p[8], p[9], wp, q[2], q[3])))))
                p = q
        _MEASURED.append(worst)
    return _MEASURED[0]


# ---- recovery: the dataset of disc_svi_ref.simulate with a sparse truth that is kept ----------------------------------------
RECOVERY = dict(N=4, T=20000, B=3, L=8, seed=2, steps=30, priors=(1.0, 1.0, 1.0, 50.0, 2.0, 4.0, 1.0), net=(1.0, 1.0))


def simulate_sparse(N=4, T=20000, B=3, L=8, seed=2024, dt=1.0):
    """disc_svi_ref.simulate, with absent links exactly 0 and present ones in [0.1, 0.3]; returns (data, A, W)."""
    rng = np.random.default_rng(seed)
    lam0 = rng.uniform(0.05, 0.15, N)
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
    W = rng.uniform(0.1, 0.3, (N, N)) * A
    theta = rng.dirichlet(np.ones(B), (N, N))
    phi = sr.basis_brute(L, B, dt)
    h = np.einsum("pc,pcb,lb->lpc", W, theta, phi) * dt
    data = np.zeros((N, T), dtype=np.int64)
    for t in range(T):
        lam = lam0 * dt
        for l in range(1, min(L, t) + 1):
            lam = lam + data[:, t - l] @ h[l - 1]
        data[:, t] = rng.poisson(lam)
    return data, A, W


# ---- the package's objects for a problem of this file (shared by the host and the GPU tests) ------------------------------------

def make_process(nhp, N, B, L, priors, net, seed=0, dt=1.0, standard=False):
    """A DiscreteNetworkHawkesProcess with SparseWeightModel and a Bernoulli (net = (α, β)) or dense (net = None) network;
    standard=True gives the DiscreteStandardHawkesProcess + DenseWeightModel(κ1, ν1) of the dense limit."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.05, 0.3, (N, N)) / max(1, N // 4)
    th = rng.dirichlet(np.ones(B), (N, N))
    base = nhp.DiscreteHomogeneousProcess(rng.uniform(0.2, 1.0, N), priors[0], priors[1], np.ones(N), np.ones(N), dt)
    imp = nhp.DiscreteGaussianImpulseResponse.__new__(nhp.DiscreteGaussianImpulseResponse)
    imp.θ, imp.γ, imp.γv, imp.nlags, imp.dt, imp.ϕ = th, priors[6], np.ones_like(th), L, dt, None
    if standard:
        return nhp.DiscreteStandardHawkesProcess(base, imp, nhp.DenseWeightModel(W, priors[4], priors[5]), dt)
    wts = nhp.SparseWeightModel(W, *priors[2:6])
    network = nhp.DenseNetworkModel(N) if net is None else nhp.BernoulliNetworkModel(0.5, N, net[0], net[1])
    return nhp.DiscreteNetworkHawkesProcess(base, imp, wts, np.ones((N, N)), network, dt)


def put(proc, params):
    av, bv, k0, n0, k1, n1, gv, rho = (np.array(p, dtype=np.float64) for p in params[:8])
    proc.baseline.αv, proc.baseline.βv, proc.impulses.γv = av, bv, gv
    w = proc.weights
    w.κv0, w.νv0, w.κv1, w.νv1, w.ρv = k0, n0, k1, n1, rho
    if hasattr(proc.network, "αv"):
        proc.network.αv, proc.network.βv = float(params[8]), float(params[9])
    return proc


def get(proc):
    w, net = proc.weights, proc.network
    return (proc.baseline.αv, proc.baseline.βv, w.κv0, w.νv0, w.κv1, w.νv1, proc.impulses.γv, w.ρv,
            getattr(net, "αv", 1.0), getattr(net, "βv", 1.0))
