"""numpy restatement of nhp_disc_residuals, written from the text in include/nhp.h (not from the kernels), an independent
`exact()` on mpmath at 60 digits, the grid of cells the host test holds the restatement to, and the model and seeds of the
statistical checks that tests/test_disc_residuals_host.py runs on the restatement and tests/test_disc_residuals_gpu.py on
the device."""
import math

import numpy as np

import disc_simulate_ref as dr

K_RES = 0x2545F4914F6CDD1D
U53 = 2.0 ** -53
TINY = 2.0 ** -60
TWO_PI = 6.283185307179586
CELL_MAX = 2.0 ** 20
SFERR = np.array([0.0] + [math.lgamma(s + 1.0) - (s + 0.5) * math.log(s) + s - 0.5 * math.log(2.0 * math.pi) for s in range(1, 16)])


# ---- the arithmetic of a cell -------------------------------------------------------------------------------------------------

def stirlerr(s):
    """δ(s) for s >= 1: lgamma-based below 16, the asymptotic series from 16 on."""
    s = np.asarray(s, dtype=np.float64)
    z = s * s
    big = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) / z) / z) / z) / z) / s
    return np.where(s < 16.0, SFERR[np.minimum(s, 15.0).astype(np.int64)], big)


def bd0(s, mu):
    """D(s, μ) = s·log(s/μ) + μ - s for s > 0, μ > 0."""
    d, sm = s - mu, s + mu
    x = d / sm
    w = x * x
    q = np.full(np.shape(w), 1.0 / 21.0)
    for c in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        q = q * w + 1.0 / c
    q = q * w
    near = d * x + ((2.0 * s) * x) * q
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        far = s * np.log(s / mu) + mu - s
    return np.where(np.abs(d) < 0.1 * sm, near, far)


def pmf(s, mu):
    """(p(s), D) for μ > 0: the saddle-point form; p(0) = exp(-μ), D(0, μ) = μ."""
    s, mu = np.asarray(s, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    pos = s > 0.0
    ss = np.where(pos, s, 1.0)
    D = np.where(pos, bd0(ss, mu), mu)
    with np.errstate(under="ignore"):
        p = np.where(pos, np.exp(-stirlerr(ss) - D) / np.sqrt(TWO_PI * ss), np.exp(-mu))
    return p, D


def naive_pmf(s, mu):
    """The form the header rules out: exp(s·log μ - μ - lgamma(s + 1))."""
    return math.exp(s * math.log(mu) - mu - math.lgamma(s + 1.0))


def pit_cells(s, mu, v, steps=None, pmf_fn=pmf):
    """pit of cells with μ > 0 (flat arrays): the tails term by term, every cell for as long as it needs."""
    s, mu, v = (np.asarray(a, dtype=np.float64) for a in (s, mu, v))
    ps, _ = pmf_fn(s, mu)
    out = np.empty(s.shape)
    n_steps = np.zeros(s.shape, dtype=np.int64)
    with np.errstate(under="ignore"):
        lo = np.flatnonzero(s <= mu)
        t, a, k = ps[lo].copy(), np.zeros(len(lo)), s[lo].copy()
        on = np.flatnonzero(k > 0.0)
        while len(on):
            t[on] = (t[on] * k[on]) / mu[lo][on]
            a[on] = a[on] + t[on]
            k[on] = k[on] - 1.0
            n_steps[lo[on]] += 1
            on = on[(k[on] > 0.0) & (t[on] > TINY * a[on])]
        out[lo] = a + v[lo] * ps[lo]
        hi = np.flatnonzero(s > mu)
        t, a, k, m = ps[hi].copy(), np.zeros(len(hi)), s[hi].copy(), mu[hi]
        on = np.arange(len(hi))
        while len(on):
            k[on] = k[on] + 1.0
            t[on] = (t[on] * m[on]) / k[on]
            a[on] = a[on] + t[on]
            n_steps[hi[on]] += 1
            on = on[t[on] > (TINY * a[on]) * (1.0 - m[on] / (k[on] + 1.0))]
        out[hi] = (1.0 - a) - (1.0 - v[hi]) * ps[hi]
    if steps is not None:
        steps.append(n_steps)
    return np.minimum(np.maximum(out, 0.0), 1.0)


def uniforms(N, T, seed):
    """v [T, N] of the cells (c, t): family K_RES, step 0, element c + N·t, attempt 0, v = ua - 2^-53."""
    ua, _ = dr.u2((seed ^ K_RES) & (2 ** 64 - 1), 0, np.arange(N * T, dtype=np.uint64), 0)
    return (ua - U53).reshape(T, N)


def residuals(counts, lam, seed, nbins=20, v=None):
    """Everything nhp_disc_residuals returns, from counts [N, T] and the cell means lam [T, N] -> a dict; the planes are
    [N, T]."""
    N, T = counts.shape
    s = counts.T.astype(np.float64)
    mu = np.asarray(lam, dtype=np.float64)
    assert mu.shape == (T, N) and np.all(np.isfinite(mu)) and np.all(mu >= 0.0) and mu.max() <= CELL_MAX and s.max() <= CELL_MAX
    v = uniforms(N, T, seed) if v is None else v
    zero = mu == 0.0
    imp = zero & (s > 0.0)
    m1 = np.where(zero, 1.0, mu)
    d = s - m1
    pe = np.where(zero, np.where(imp, np.inf, 0.0), d / np.sqrt(m1))
    chi = np.where(zero, np.where(imp, np.inf, 0.0), (d * d) / m1)
    _, D = pmf(s, m1)
    D = np.where(zero, 0.0, D)
    p = np.where(zero, np.where(imp, 1.0, v), 0.0)
    live = ~zero
    p[live] = pit_cells(s[live], mu[live], v[live])
    b = np.minimum((p * float(nbins)).astype(np.int64), nbins - 1)
    hist = np.zeros((N, nbins), dtype=np.int64)
    np.add.at(hist, (np.broadcast_to(np.arange(N), (T, N)).ravel(), b.ravel()), 1)
    return dict(pit=p.T, pearson=pe.T, cumulative=np.cumsum(mu, axis=0).T, expected=mu.sum(axis=0),
                observed=counts.sum(axis=1).astype(np.int64), chi2=chi.sum(axis=0), deviance=2.0 * D.sum(axis=0), histogram=hist,
                impossible=int(imp.sum()))


# ---- the independent reference: mpmath at 60 digits ------------------------------------------------------------------------------

def exact(s, mu, v):
    """pit = F(s-1) + v·p(s) of one cell from the regularised incomplete gamma function, at 60 digits -> an mpf."""
    import mpmath as mp
    with mp.workdps(60):
        s, m, v = int(s), mp.mpf(mu), mp.mpf(v)
        p = mp.exp(s * mp.log(m) - m - mp.loggamma(s + 1))
        below = mp.gammainc(s, m, mp.inf, regularized=True) if s > 0 else mp.mpf(0)     # F(s-1) = Q(s, μ)
        return below + v * p


def grid():
    """The 109 cells (s, μ): μ from 1e-300 to 2^20, s at 0, 1, 2, 5 and at μ + {0, ±1, ±4, ±8}·√μ (counts inside [0, 2^20])."""
    cells = set()
    for mu in (1e-300, 1e-10, 1e-3, 0.05, 0.2, 0.5, 1.0, 3.0, 10.0, 15.5, 64.0, 1000.0, 2500.0, 65536.0, 1048576.0):
        for s in (0, 1, 2, 5):
            cells.add((s, mu))
        for z in (0, 1, -1, 4, -4, 8, -8):
            s = int(math.floor(mu + z * math.sqrt(mu)))
            if 0 <= s <= CELL_MAX:
                cells.add((s, mu))
    return sorted(cells)


GRID_V = (0.0, 0.37, 1.0 - U53)


# ---- the statistics (the product's own are in discrete.py; these are written again so that the host file needs no GPU) ---------

def ks_uniform(u):
    """(D_n, p) of the one-sample Kolmogorov-Smirnov test against U(0, 1), Stephens' asymptotic series."""
    u = np.sort(np.asarray(u, dtype=np.float64).ravel())
    n = len(u)
    i = np.arange(1, n + 1)
    d = float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))
    x = d * (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n))
    k = np.arange(1, 101)
    return d, (1.0 if x < 0.2 else float(min(1.0, max(0.0, 2.0 * np.sum((-1.0) ** (k - 1) * np.exp(-2.0 * k * k * x * x))))))


def histogram_pvalue(hist):
    from scipy.special import gammaincc
    h = np.asarray(hist, dtype=np.float64).sum(axis=0)
    e = h.sum() / len(h)
    return float(gammaincc(0.5 * (len(h) - 1), 0.5 * np.sum((h - e) ** 2 / e)))


# ---- the model and the seeds of the statistical checks ----------------------------------------------------------------------------

STAT_T, STAT_DATA_SEED, STAT_SEED = 4096, 21, 5
KS_TRUE_MIN, KS_WRONG_MAX, DISPERSION_TOL = 0.01, 1e-6, 0.1


def stat_process(nhp):
    return dr.make(nhp, N=4, L=4, B=3)


def wrong(process):
    """The same process with every weight times 1.5."""
    import copy
    q = copy.deepcopy(process)
    q.weights.W = q.weights.W * 1.5
    return q
