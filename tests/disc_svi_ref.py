"""Reference for stochastic variational inference on discrete Hawkes processes, in numpy.

The step.  The T bins are cut into nb = ceil(T / Tb) consecutive blocks, block j = [j·Tb, min(T, (j+1)·Tb)).  Step i (global,
1-based) on block j: with (α', κ', γ') the mean-field update! computed from the current parameters with every sum over t
restricted to the block (Ŝ is the convolution of the WHOLE data, so lags reach back before the block's first bin),

    α̂ = α0 + nb (α' - α0)      γ̂ = γ + nb (γ' - γ)      κ̂ = κ + Σ_b (γ̂ - γ)
    β̂ = 1/β0 + T·dt            ν̂[p, c] = ν + Σ_{t<T} data[p, t]          (whole data: no local variable in either)

and every parameter x <- (1 - ρ_i) x + ρ_i x̂ with ρ_i = (i + τ)^(-κ_f).

`svi_step` takes the block update from the oracle's VB step on data[:, t0:t1] and conv[t0:t1]; it writes κ̂ as
κ + nb (κ' - κ) from the oracle's own κ' -- the same number as κ + Σ_b (γ̂ - γ), since κ' - κ = Σ_b (γ' - γ), and with
nb = 1, τ = 0 the step then IS the oracle's VB step bit for bit.  `svi_step_brute` is written straight from the formulas
with explicit loops over t, c, p, b and calls no oracle (basis and convolution included): for tiny shapes.
"""
import numpy as np
from scipy.special import digamma


def block_bounds(T, Tb, j):
    Tb = min(Tb, T)
    t0 = j * Tb
    return t0, min(T, t0 + Tb)


def n_blocks(T, Tb):
    Tb = min(Tb, T)
    return -(-T // Tb)


def rho(i, delay, forgetting):
    return (i + delay) ** (-forgetting)


def blend(x, xhat, r):
    return (1.0 - r) * x + r * xhat


def svi_step(orc, data, conv, dt, priors, params, j, Tb, i, delay, forgetting):
    """One step on block j as global step i; params = (αv, βv, κv, νv, γv); returns the five new arrays."""
    alpha0, beta0, kappa, nu, gamma = priors
    N, T = data.shape
    nb = n_blocks(T, Tb)
    t0, t1 = block_bounds(T, Tb, j)
    a1, _b1, k1, _n1, g1 = orc.disc_vb_step(data[:, t0:t1], conv[t0:t1], dt, alpha0, beta0, kappa, nu, gamma, *params)
    ah = alpha0 + nb * (a1 - alpha0)
    gh = gamma + nb * (g1 - gamma)
    kh = kappa + nb * (k1 - kappa)
    bh = np.full(N, 1.0 / beta0 + T * dt)
    nh = np.repeat((nu + data.sum(axis=1).astype(np.float64))[:, None], N, axis=1)
    r = rho(i, delay, forgetting)
    av, bv, kv, nv, gv = params
    return blend(av, ah, r), blend(bv, bh, r), blend(kv, kh, r), blend(nv, nh, r), blend(gv, gh, r)


def svi_run(orc, data, conv, dt, priors, params, blocks, Tb, delay, forgetting, step0=0):
    params = tuple(np.array(p, dtype=np.float64) for p in params)
    for k, j in enumerate(blocks):
        params = svi_step(orc, data, conv, dt, priors, params, int(j), Tb, step0 + k + 1, delay, forgetting)
    return params


def vb_run(orc, data, conv, dt, priors, params, passes):
    params = tuple(np.array(p, dtype=np.float64) for p in params)
    for _ in range(passes):
        params = orc.disc_vb_step(data, conv, dt, *priors, *params)
    return params


def loglik_at_means(orc, data, conv, params, dt):
    """Poisson log-likelihood at the variational means: λ0 = αv/βv, W = κv/νv, θ = γv/Σ_b γv."""
    av, bv, kv, nv, gv = params
    theta = gv / gv.sum(axis=2, keepdims=True)
    return orc.disc_loglik(data, orc.disc_intensity(conv, av / bv, kv / nv, theta, dt))


# ---- brute force, no oracle ----------------------------------------------------------------------------------------

def basis_brute(L, B, dt):
    """basis(impulse) (src/impulses.jl:321-335): L x B, column b normalised to 1/dt."""
    sigma = L / (B - 1)
    coef = ((-1.0 / 2.0) * (1.0 / sigma)) / 2.0
    phi = np.empty((L, B))
    for b in range(B):
        ln, i = (B + 2, b + 1) if B < L else (B, b)
        tt = i / (ln - 1 if ln > 1 else 1)
        mu = (1.0 - tt) * 1.0 + tt * L
        for l in range(L):
            phi[l, b] = np.exp(coef * ((l + 1) - mu) ** 2)
        phi[:, b] /= phi[:, b].sum() * dt
    return phi


def convolve_brute(data, phi):
    N, T = data.shape
    L, B = phi.shape
    conv = np.zeros((T, N, B))
    for t in range(T):
        for n in range(N):
            for b in range(B):
                s = 0.0
                for l in range(1, min(L, t) + 1):
                    s += data[n, t - l] * phi[l - 1, b]
                conv[t, n, b] = max(s, 0.0)
    return conv


def svi_step_brute(data, L, dt, priors, params, j, Tb, i, delay, forgetting):
    alpha0, beta0, kappa, nu, gamma = priors
    av, bv, kv, nv, gv = params
    N, T = data.shape
    B = gv.shape[2]
    conv = convolve_brute(data, basis_brute(L, B, dt))
    nb = n_blocks(T, Tb)
    t0, t1 = block_bounds(T, Tb, j)
    e0 = np.array([np.exp(digamma(av[c]) - np.log(bv[c])) for c in range(N)])
    E = np.empty((N, N, B))
    for p in range(N):
        for c in range(N):
            for b in range(B):
                E[p, c, b] = np.exp(digamma(gv[p, c, b]) - digamma(gv[p, c, :].sum()) + digamma(kv[p, c]) - np.log(nv[p, c]))
    a_stat = np.zeros(N)
    g_stat = np.zeros((N, N, B))
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
    ah = alpha0 + nb * ((alpha0 + a_stat) - alpha0)
    gh = gamma + nb * ((gamma + g_stat) - gamma)
    kh = kappa + (gh - gamma).sum(axis=2)
    bh = np.full(N, 1.0 / beta0 + T * dt)
    nh = np.empty((N, N))
    for p in range(N):
        nh[p, :] = nu + sum(float(data[p, t]) for t in range(T))
    r = rho(i, delay, forgetting)
    return blend(av, ah, r), blend(bv, bh, r), blend(kv, kh, r), blend(nv, nh, r), blend(gv, gh, r)


# ---- the data of the "SVI earns its name" property -------------------------------------------------------------------

EARNS = dict(N=4, T=20000, B=3, L=8, Tb=256, delay=10.0, forgetting=0.6, passes=5)


def simulate(N=4, T=20000, B=3, L=8, seed=2024, dt=1.0):
    """Counts of a discrete Hawkes process: bin (c, t) ~ Poisson(λ0[c]·dt + Σ_{p,l} data[p, t-l]·W[p,c]·dt·Σ_b θ[p,c,b]·ϕ_b[l])."""
    rng = np.random.default_rng(seed)
    lam0 = rng.uniform(0.05, 0.15, N)
    W = rng.uniform(0.0, 0.25, (N, N)) * (rng.uniform(size=(N, N)) < 0.6)
    theta = rng.dirichlet(np.ones(B), (N, N))
    phi = basis_brute(L, B, dt)
    h = np.einsum("pc,pcb,lb->lpc", W, theta, phi) * dt           # h[l-1, p, c]
    data = np.zeros((N, T), dtype=np.int64)
    for t in range(T):
        lam = lam0 * dt
        for l in range(1, min(L, t) + 1):
            lam = lam + data[:, t - l] @ h[l - 1]
        data[:, t] = rng.poisson(lam)
    return data


def ones_start(N, B):
    return np.ones(N), np.ones(N), np.ones((N, N)), np.ones((N, N)), np.ones((N, N, B))


def earns_blocks(seed):
    nb = n_blocks(EARNS["T"], EARNS["Tb"])
    return np.random.default_rng(seed).integers(nb, size=EARNS["passes"] * nb).astype(np.int32)
