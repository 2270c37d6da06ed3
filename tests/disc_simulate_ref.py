"""numpy restatement of nhp_disc_simulate, written from the scheme in include/nhp.h (not from the kernels), the models both
test files use, and the statistics they assert.

`simulate` replays the documented counters exactly -- Philox4x32-10 blocks, the inversion / PTRS Poisson sampler, the
sequential prefix tables, the arena order -- vectorised over the elements of a step, so a GPU sample must equal it bit for
bit.  `martingale_z` and `immigrant_checks` are the statistical checks of tests/test_disc_simulate_gpu.py; the host test
file runs them on `simulate`'s samples, which shows that the fixed seeds pass for a correct sampler."""
import math

import numpy as np

K_IMM, K_CHILD_COUNT, K_CHILD = 0xA3B195354A39B70D, 0x1B03738712FAD5C9, 0xC2B2AE3D27D4EB4F
M32 = np.uint64(0xFFFFFFFF)
U53 = 2.0 ** -53
S32, S11 = np.uint64(32), np.uint64(11)


# ---- the counter scheme ---------------------------------------------------------------------------------------------------

def philox(key, step, e, attempt):
    """Philox4x32-10 on counters (e mod 2^32, (e >> 32) ^ (attempt << 8), step mod 2^32, step >> 32), key = (lo, hi)."""
    e = np.asarray(e, dtype=np.uint64)
    c0, c1 = e & M32, ((e >> S32) ^ np.uint64((attempt << 8) & 0xFFFFFFFF)) & M32
    c2 = np.full(e.shape, step & 0xFFFFFFFF, dtype=np.uint64)
    c3 = np.full(e.shape, (step >> 32) & 0xFFFFFFFF, dtype=np.uint64)
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> S32) ^ c1 ^ np.uint64(k0)) & M32, p1 & M32, ((p0 >> S32) ^ c3 ^ np.uint64(k1)) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def u2(key, step, e, attempt):
    """ua, ub in (0, 1] of one block."""
    w0, w1, w2, w3 = philox(key, step, e, attempt)
    return ((((w0 << S32) | w1) >> S11).astype(np.float64) + 1.0) * U53, ((((w2 << S32) | w3) >> S11).astype(np.float64) + 1.0) * U53


def loggam(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.where(x < 7.0, np.floor(7.0 - x), 0.0)
    x0 = x + n
    x2 = (1.0 / x0) * (1.0 / x0)
    c = (8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04,
         -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e+00)
    g = np.full(x.shape, c[9])
    for k in range(8, -1, -1):
        g = g * x2 + c[k]
    gl = g / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * np.log(x0) - x0
    for k in range(1, 7):
        on = n >= k
        gl = np.where(on, gl - np.log(np.where(on, x0 - 1.0, 1.0)), gl)
        x0 = np.where(on, x0 - 1.0, x0)
    return np.where((x == 1.0) | (x == 2.0), 0.0, gl)


def poisson(mean, key, step, e, branches=None):
    """Poisson(mean[i]) of element e[i]: inversion below 10 (one uniform, attempt 0), PTRS from there on (a block per attempt)."""
    e = np.asarray(e, dtype=np.uint64)
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), e.shape)
    out = np.zeros(e.shape, dtype=np.int64)
    small = (mean > 0.0) & (mean < 10.0)
    if small.any():
        if branches is not None:
            branches.add("inversion")
        m = mean[small]
        ua, _ = u2(key, step, e[small], 0)
        u = ua - U53
        p = np.exp(-m)
        F, k = p.copy(), np.zeros(m.shape)
        on = (u >= F) & (k < 100.0)
        while on.any():
            k[on] += 1.0
            p[on] = p[on] * m[on] / k[on]
            F[on] = F[on] + p[on]
            on = (u >= F) & (k < 100.0)
        out[small] = k.astype(np.int64)
    big = mean >= 10.0
    if big.any():
        if branches is not None:
            branches.add("ptrs")
        m, ee = mean[big], e[big]
        slam, loglam = np.sqrt(m), np.log(m)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha, vr = 1.1239 + 1.1328 / (b - 3.4), 0.9277 - 3.6224 / (b - 2.0)
        lia = np.log(invalpha)
        res = np.zeros(m.shape, dtype=np.int64)
        todo = np.arange(len(m))
        for att in range(4096):
            if not len(todo):
                break
            mm, aa, bb = m[todo], a[todo], b[todo]
            ua, V = u2(key, step, ee[todo], att)
            U = (ua - U53) - 0.5
            us = 0.5 - np.abs(U)
            with np.errstate(divide="ignore", invalid="ignore"):
                k = np.floor((2.0 * aa / us + bb) * U + mm + 0.43)
                quick = (us >= 0.07) & (V <= vr[todo])
                skip = ~quick & ((k < 0.0) | ((us < 0.013) & (V > us)))
                slow = ~quick & ~skip
                ks = np.where(slow, k, 0.0)
                ok = slow & (np.log(V) + lia[todo] - np.log(aa / (us * us) + bb) <= -mm + ks * loglam[todo] - loggam(ks + 1.0))
            done = quick | ok
            res[todo[done]] = k[done].astype(np.int64)
            todo = todo[~done]
        assert not len(todo), "PTRS did not accept"
        out[big] = res
    return out


def first_above(table, x):
    """Per row: the first column with table > x; if none, the first with table >= x."""
    gt = table > x[:, None]
    ge = table >= x[:, None]
    return np.where(gt.any(axis=1), gt.argmax(axis=1), ge.argmax(axis=1))


# ---- the sampler ------------------------------------------------------------------------------------------------------------

def lower(process, T):
    """What disc_rand hands the library: base [T, N] (per-bin means, already times dt), W, θ, A | None, φ [L, B], dt."""
    dt = process.dt
    if hasattr(process.baseline, "x"):
        base = process.baseline.intensity(np.arange(1, T + 1, dtype=np.float64))
    else:
        base = np.tile(np.asarray(process.baseline.λ, float) * dt, (T, 1))
    return (base, np.asarray(process.weights.W, float), np.asarray(process.impulses.θ, float),
            getattr(process, "adjacency_matrix", None), np.asarray(process.impulses.basis(), float), dt)


def tables(W, theta, A, phi, dt):
    cdf = np.cumsum(phi, axis=0)                      # [L, B], sequential
    mb = cdf[-1] * dt
    S = np.zeros(W.shape)
    for b in range(theta.shape[2]):
        S = S + theta[:, :, b] * mb[b]
    V = (W * A if A is not None else W) * S
    G = np.cumsum(V, axis=1)                          # sequential row prefix
    return cdf, mb, G, G[:, -1].copy()


def simulate(process, T, seed, info=None, tabs=None):
    """(counts, background), both N x T int64.  info (a dict) receives the generated child slots, the kept children, the
    generations, the slots of each generation and the Poisson branches taken."""
    base, W, theta, A, phi, dt = tabs if tabs is not None else lower(process, T)
    N, B, L = W.shape[0], theta.shape[2], phi.shape[0]
    cdf, mb, G, R = tables(W, theta, A, phi, dt)
    branches = set()
    e = np.arange(N * T, dtype=np.uint64)
    cell_c, cell_t = (e % np.uint64(N)).astype(np.int64), (e // np.uint64(N)).astype(np.int64)
    k0 = poisson(base[cell_t, cell_c], seed ^ K_IMM, 0, e, branches)
    background = k0.reshape(T, N).T.copy()
    occ = k0 > 0
    node, bins, mult = [cell_c[occ]], [cell_t[occ]], [k0[occ]]
    g0, g1, gen = 0, int(occ.sum()), 0
    kids = poisson(mult[0] * R[node[0]], seed ^ K_CHILD_COUNT, 0, np.arange(g0, g1, dtype=np.uint64), branches)
    slots, kept, per_gen = 0, 0, []
    while kids.sum():
        C = int(kids.sum())
        per_gen.append(C)
        par = np.repeat(np.arange(len(kids)), kids)
        p, tp = node[-1][par], bins[-1][par]
        s = np.arange(C, dtype=np.uint64)
        ua, ub = u2(seed ^ K_CHILD, gen, s, 0)
        uc, _ = u2(seed ^ K_CHILD, gen, s, 1)
        c = first_above(G[p], (ua - U53) * R[p])
        Sb = np.cumsum(theta[p, c, :] * mb[None, :], axis=1)
        b = first_above(Sb, (ub - U53) * Sb[:, -1])
        col = cdf[:, b].T
        lag = first_above(col, (uc - U53) * col[:, -1]) + 1
        keep = tp + lag < T
        slots, kept = slots + C, kept + int(keep.sum())
        node.append(c[keep]); bins.append((tp + lag)[keep]); mult.append(np.ones(int(keep.sum()), dtype=np.int64))
        g0, g1, gen = g1, g1 + int(keep.sum()), gen + 1
        kids = poisson(R[node[-1]], seed ^ K_CHILD_COUNT, gen, np.arange(g0, g1, dtype=np.uint64), branches)
    counts = np.zeros((N, T), dtype=np.int64)
    np.add.at(counts, (np.concatenate(node), np.concatenate(bins)), np.concatenate(mult))
    if info is not None:
        info.update(slots=slots, kept=kept, generations=gen, per_generation=per_gen, branches=branches)
    return counts, background


# ---- the models of the tests --------------------------------------------------------------------------------------------------

def make(nhp, N, L=4, B=3, seed=0, dt=1.0, network=False, rate=0.3, scale=0.5, lgcp_T=None, theta_zero=False, self_weight=0.0):
    """Standard or network process with row sums of W near `scale` (+ self_weight on the diagonal); network: A ~ Bernoulli(0.7)
    with column 1 all zero; lgcp_T: a DiscreteLogGaussianCoxProcess baseline on a grid over [0, lgcp_T]."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.2, 1.0, (N, N)) * scale / (0.6 * N) + self_weight * np.eye(N)
    th = rng.dirichlet(np.ones(B), (N, N))
    if theta_zero:
        th[0, :, 0] = 0.0                             # node 0 never acts through basis 0
        th[0] /= th[0].sum(axis=1, keepdims=True)
    if self_weight:
        th[np.arange(N), np.arange(N)] = np.r_[0.9, np.full(B - 1, 0.1 / (B - 1))]       # self-excitation sits at the short lags
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    lam0 = rng.uniform(0.5, 1.5, N) * rate
    if lgcp_T is None:
        base = nhp.DiscreteHomogeneousProcess(lam0, dt)
    else:
        x = np.linspace(0.0, float(lgcp_T), 11)
        lam = lam0[None, :] * np.exp(0.8 * np.sin(2.0 * np.pi * x / lgcp_T)[:, None] * rng.uniform(0.5, 1.0, N)[None, :])
        base = nhp.DiscreteLogGaussianCoxProcess(x, lam, None, 0.0, dt)
    imp = nhp.DiscreteGaussianImpulseResponse.__new__(nhp.DiscreteGaussianImpulseResponse)
    imp.θ, imp.γ, imp.γv, imp.nlags, imp.dt, imp.ϕ = th, 1.0, np.ones_like(th), L, dt, None
    wts = nhp.DenseWeightModel(W)
    if not network:
        return nhp.DiscreteStandardHawkesProcess(base, imp, wts, dt)
    A = (rng.uniform(size=(N, N)) < 0.7).astype(float)
    A[:, 1] = 0.0
    return nhp.DiscreteNetworkHawkesProcess(base, imp, wts, A, nhp.BernoulliNetworkModel(0.7, N), dt)


def link_mass(process):
    """G[p, c] = W·A·Σ_b θ·m_b: the expected children on node c of one event on node p."""
    _, W, theta, A, phi, dt = lower(process, 1)
    cdf, mb, G, R = tables(W, theta, A, phi, dt)
    return np.diff(G, axis=1, prepend=0.0)


# ---- the statistics -----------------------------------------------------------------------------------------------------------

def intensity(process, counts, phi=None):
    """λ [T, N] from its definition (src/discrete.jl:115-129): base[t,c] + Σ_p Σ_l s[p,t-l]·W·A·dt·Σ_b θ[p,c,b]·φ[l,b]."""
    N, T = counts.shape
    base, W, theta, A, ph, dt = lower(process, T)
    phi = ph if phi is None else phi
    V = W * A if A is not None else W
    h = np.einsum("pc,pcb,lb->pcl", V, theta, phi) * dt
    lam = base.copy()
    s = counts.astype(np.float64)
    for l in range(1, phi.shape[0] + 1):
        lam[l:] += s[:, :T - l].T @ h[:, :, l - 1]
    return lam


def shifted_basis(process):
    """The lag table moved one bin later: lag l takes what lag l - 1 had, lag 1 nothing."""
    phi = np.asarray(process.impulses.basis(), float)
    return np.vstack([np.zeros((1, phi.shape[1])), phi[:-1]])


def martingale_z(counts, lam, L):
    """z_c = Σ_t (s[c,t] - λ[t,c]) / √Σ_t λ[t,c] and, for every (p, c, lag l), z = Σ_t (s[c,t] - λ[t,c])·s[p,t-l] /
    √Σ_t λ[t,c]·s[p,t-l]²: normalised martingale sums, N(0, 1) under the model that produced `lam`.  -> (z_c [N], z [L, N, N])"""
    s = counts.astype(np.float64).T                   # [T, N]
    r = s - lam
    zc = r.sum(axis=0) / np.sqrt(lam.sum(axis=0))
    T = s.shape[0]
    z = np.empty((L,) + (s.shape[1],) * 2)
    for l in range(1, L + 1):
        z[l - 1] = (s[:T - l].T @ r[l:]) / np.sqrt((s[:T - l] ** 2).T @ lam[l:])
    return zc, z


def chi2_ok(obs, exp):
    """χ² goodness of fit, Wilson-Hilferty normal approximation, p > 1e-4."""
    k = len(obs) - 1
    if k < 1:
        return True
    x = float(np.sum((obs - exp) ** 2 / exp))
    z = ((x / k) ** (1 / 3) - (1 - 2 / (9 * k))) / math.sqrt(2 / (9 * k))
    return z < 3.72


def immigrant_checks(counts, mean):
    """counts [N, T] of i.i.d. Poisson(mean) cells: per-node totals within 5σ of T·mean, and the histogram of the cell counts
    against the Poisson pmf (cells pooled so that every expected count is at least 20)."""
    N, T = counts.shape
    z = (counts.sum(axis=1) - T * mean) / math.sqrt(T * mean)
    kmax = int(counts.max())
    ks = np.arange(kmax + 1)
    logp = -mean + ks * math.log(mean) - np.array([math.lgamma(k + 1.0) for k in ks])
    exp = N * T * np.exp(logp)
    obs = np.bincount(counts.ravel(), minlength=kmax + 1).astype(float)
    keep = exp >= 20.0
    lo, hi = np.argmax(keep), len(keep) - np.argmax(keep[::-1]) - 1
    pmf_tail = N * T - exp[lo:hi + 1].sum()            # the pooled tails: everything outside [lo, hi]
    o = np.r_[obs[lo:hi + 1], obs[:lo].sum() + obs[hi + 1:].sum()]
    x = np.r_[exp[lo:hi + 1], pmf_tail]
    if x[-1] < 20.0:                                  # a thin pooled tail joins its neighbour
        o[-2] += o[-1]; x[-2] += x[-1]
        o, x = o[:-1], x[:-1]
    return z, chi2_ok(o, x)


def two_sample_z(a, b):
    """Welch z of the means of two samples along axis 0."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return (a.mean(axis=0) - b.mean(axis=0)) / np.sqrt(a.var(axis=0, ddof=1) / len(a) + b.var(axis=0, ddof=1) / len(b))


# ---- the cases both test files run (the host file on `simulate`, the GPU file on disc_rand) --------------------------------------

T_SMALL = 300
# name -> (make() arguments, bins, seed): the cases of the exact comparison
RESTATE_CASES = {
    "standard": (dict(N=3, seed=1), T_SMALL, 3),
    "network, A with a zero column": (dict(N=5, seed=2, network=True, dt=0.5), T_SMALL, 4),
    "a zero in theta": (dict(N=3, seed=3, theta_zero=True), T_SMALL, 5),
    "LGCP baseline": (dict(N=5, seed=4, lgcp_T=T_SMALL), T_SMALL, 6),
    "cell means from 10 on (PTRS)": (dict(N=3, seed=5, rate=14.0, scale=0.3), T_SMALL, 7),
    "N = 70: two row tiles": (dict(N=70, seed=6, rate=0.05), T_SMALL, 8),
}
# the processes of the martingale check: N = 5, T = 20000, more than 2·10^4 events per node
MARTINGALE_T, MARTINGALE_SEED = 20000, 11
MARTINGALE_CASES = {
    "standard": dict(N=5, seed=1, self_weight=0.35, scale=0.3, rate=0.4),
    "network": dict(N=5, seed=2, network=True, self_weight=0.35, scale=0.3, rate=0.4, dt=0.5),
}
IMMIGRANT_MEANS, IMMIGRANT_T, IMMIGRANT_SEED, IMMIGRANT_DT = (0.05, 3.0, 40.0), 20000, 5, 0.5
AGREEMENT = (dict(N=3, seed=4, rate=0.3, scale=0.5), 2000, 40)      # make() arguments, bins, seeds per route


def immigrant_process(nhp, mean):
    p = make(nhp, 3, scale=0.0, dt=IMMIGRANT_DT)
    p.baseline = nhp.DiscreteHomogeneousProcess(np.full(3, mean / IMMIGRANT_DT), IMMIGRANT_DT)
    return p


def assert_martingale(process, counts, lam, lam_shifted):
    """|z| <= 5 for every statistic under the process' own intensity `lam`; more than 5 somewhere under `lam_shifted`, the
    intensity of the same process with its lag table one bin late (the check has the power to see a lag off by one)."""
    L = process.nlags()
    zc, z = martingale_z(counts, lam, L)
    fin = np.isfinite(z)                              # a pair with no expected mass (a zero column of A and no events) has 0/0
    print(f"martingale: max |z_c| = {np.abs(zc).max():.2f}, max |z_pcl| = {np.abs(z[fin]).max():.2f} over {fin.sum()} statistics")
    assert fin.sum() >= 0.75 * z.size
    assert np.all(np.abs(zc) <= 5.0) and np.all(np.abs(z[fin]) <= 5.0)
    zc2, z2 = martingale_z(counts, lam_shifted, L)
    print(f"lag table shifted by one bin: max |z_c| = {np.abs(zc2).max():.2f}, max |z_pcl| = {np.nanmax(np.abs(z2)):.2f}")
    assert max(np.abs(zc2).max(), np.nanmax(np.abs(z2))) > 5.0


def agreement_stats(counts):
    """Per-node totals and the lag-1 cross-products Σ_t s[p,t]·s[c,t+1], as one vector."""
    s = counts.astype(np.float64)
    return np.r_[s.sum(axis=1), (s[:, :-1] @ s[:, 1:].T).ravel()]


def assert_agreement(a, b):
    """Two routes, the same law: two-sample z of every statistic of agreement_stats, |z| <= 5."""
    z = two_sample_z(np.array([agreement_stats(x) for x in a]), np.array([agreement_stats(x) for x in b]))
    print(f"two routes: max |z| = {np.abs(z).max():.2f} over {z.size} statistics")
    assert np.all(np.abs(z) <= 5.0)
