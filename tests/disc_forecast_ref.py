"""numpy restatements of disc_forecast(process, data, horizon) (nhp_disc_forecast, include/nhp.h), the cases both test files
use, and the statistics they assert.

(a) `literal_sample`: the three parts of the law drawn one after the other with numpy's own generator -- carry-over children
    of the observed events, new immigrants, descendants generation by generation -- and `mean_recursion`, the exact predictive
    mean μ_k = base_k + carry_k + Σ_l H_lᵀ μ_{k-l}.  Nothing of the library's scheme enters.
(b) `restate`: the documented Philox scheme draw by draw, written from include/nhp.h alone (the Philox block, the Poisson
    sampler and the child draw are the helpers of disc_simulate_ref.py), so a GPU ensemble must equal it bit for bit: the
    sequential fp64 sums of x and carry, the cell means base + carry, cells e = c + N·(k + H·r), the shared arena.

The host test file runs every statistical check of the GPU file on (b)'s ensembles with the same models and seeds."""
import numpy as np

import disc_simulate_ref as dr

K_CELL, K_CHILD_COUNT, K_CHILD = 0xDA942042E4DD58B5, 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7
U53 = dr.U53


# ---- the law from its definition --------------------------------------------------------------------------------------------

def lower(process, T0, H):
    """base [H, N] (means of the forecast bins, already times dt), W, θ, A | None, φ [L, B], dt."""
    dt = process.dt
    if hasattr(process.baseline, "x"):
        base = process.baseline.intensity(np.arange(T0 + 1, T0 + H + 1, dtype=np.float64))
    else:
        base = np.tile(np.asarray(process.baseline.λ, float) * dt, (H, 1))
    return (base, np.asarray(process.weights.W, float), np.asarray(process.impulses.θ, float),
            getattr(process, "adjacency_matrix", None), np.asarray(process.impulses.basis(), float), dt)


def link_lag_mass(W, theta, A, phi, dt):
    """h[p, c, l-1] = W[p,c]·A[p,c]·dt·Σ_b θ[p,c,b]·φ[l,b]."""
    return np.einsum("pc,pcb,lb->pcl", W * A if A is not None else W, theta, phi) * dt


def carry_exact(data, h, H):
    """carry [H, N]: carry[k-1, c] = Σ_p Σ_{l=k..L, T0+k-l >= 1} s[p, T0+k-l]·h[p,c,l]."""
    N, T0 = data.shape
    L = h.shape[2]
    out = np.zeros((H, N))
    for k in range(1, H + 1):
        for l in range(k, L + 1):
            t = T0 + k - l                            # 1-based observed bin
            if t >= 1:
                out[k - 1] += data[:, t - 1].astype(float) @ h[:, :, l - 1]
    return out


def mean_recursion(base, carry, h):
    """μ [H, N]: μ_k = base_k + carry_k + Σ_{l=1..min(L, k-1)} H_lᵀ μ_{k-l}."""
    H, L = base.shape[0], h.shape[2]
    mu = np.zeros_like(base)
    for k in range(H):
        mu[k] = base[k] + carry[k]
        for l in range(1, min(L, k) + 1):
            mu[k] += mu[k - l] @ h[:, :, l - 1]
    return mu


def literal_sample(data, base, h, S, rng):
    """S continuations [S, N, H] by the three parts of the law, numpy's generator: (1) every observed cell (p, t) with s events
    has Poisson(s·h[p,c,l]) children in cell (c, t+l) for T0 < t+l <= T0+H; (2) Poisson(base) immigrants per cell; (3) every
    entry of a generation has Poisson(h[p,c,l]) children in bin k+l <= H of its own replica, generation after generation."""
    N, T0 = data.shape
    H, L = base.shape[0], h.shape[2]
    gen = np.zeros((S, N, H), dtype=np.int64)
    for t in range(1, T0 + 1):
        for l in range(1, L + 1):
            k = t + l - T0                            # 1-based forecast bin
            if 1 <= k <= H:
                gen[:, :, k - 1] += rng.poisson(data[:, t - 1].astype(float) @ h[:, :, l - 1], (S, N))
    gen += rng.poisson(base.T[None], (S, N, H))
    out = gen.copy()
    while gen.any():
        nxt = np.zeros_like(gen)
        for l in range(1, min(L, H - 1) + 1):
            nxt[:, :, l:] += rng.poisson(np.einsum("spk,pc->sck", gen[:, :, :H - l].astype(float), h[:, :, l - 1]))
        out += nxt
        gen = nxt
    return out


def cell_z(paths, mu):
    """z [H, N] of the ensemble mean per cell against mu [H, N], with the sample variance of the paths [S, N, H]."""
    S = paths.shape[0]
    m, v = paths.mean(axis=0).T, paths.var(axis=0, ddof=1).T
    return (m - mu) / np.sqrt(v / S)


# ---- (b) the documented scheme ------------------------------------------------------------------------------------------------

def boundary(process, data, H):
    """(cm [H, N], carry [H, N], tables) with the documented operation order: the bits of the library."""
    N, T0 = data.shape
    base, W, theta, A, phi, dt = lower(process, T0, H)
    L, B = phi.shape
    K, Tu = min(L, H), min(L, T0)
    tail = data[:, T0 - Tu:].astype(np.float64)       # tail[:, j] = bin T0 - Tu + 1 + j
    wa = W * A if A is not None else W
    carry = np.zeros((H, N))
    for k in range(K):
        x = np.zeros((N, B))
        for l in range(k + 1, min(L, Tu + k) + 1):
            x = x + tail[:, Tu + k - l][:, None] * phi[l - 1][None, :]
        acc = np.zeros(N)
        for p in range(N):
            for b in range(B):
                acc = acc + (wa[p] * theta[p, :, b]) * x[p, b]
        carry[k] = dt * acc
    return base + carry, carry, (W, theta, A, phi, dt)


def restate(process, data, H, S, seed, info=None):
    """(paths [S, N, H], carry [H, N]) of nhp_disc_forecast, draw by draw."""
    data = np.asarray(data)
    N = data.shape[0]
    cm, carry, (W, theta, A, phi, dt) = boundary(process, data, H)
    cdf, mb, G, R = dr.tables(W, theta, A, phi, dt)
    branches = set()
    T = S * H
    e = np.arange(N * T, dtype=np.uint64)
    cell_c, cell_g = (e % np.uint64(N)).astype(np.int64), (e // np.uint64(N)).astype(np.int64)
    k0 = dr.poisson(cm[cell_g % H, cell_c], seed ^ K_CELL, 0, e, branches)
    occ = k0 > 0
    node, bins, mult = [cell_c[occ]], [cell_g[occ]], [k0[occ]]
    g0, g1, gen = 0, int(occ.sum()), 0
    kids = dr.poisson(mult[0] * R[node[0]], seed ^ K_CHILD_COUNT, 0, np.arange(g0, g1, dtype=np.uint64), branches)
    per_gen = []
    while kids.sum():
        C = int(kids.sum())
        per_gen.append(C)
        par = np.repeat(np.arange(len(kids)), kids)
        p, gp = node[-1][par], bins[-1][par]
        s = np.arange(C, dtype=np.uint64)
        ua, ub = dr.u2(seed ^ K_CHILD, gen, s, 0)
        uc, _ = dr.u2(seed ^ K_CHILD, gen, s, 1)
        c = dr.first_above(G[p], (ua - U53) * R[p])
        Sb = np.cumsum(theta[p, c, :] * mb[None, :], axis=1)
        b = dr.first_above(Sb, (ub - U53) * Sb[:, -1])
        col = cdf[:, b].T
        lag = dr.first_above(col, (uc - U53) * col[:, -1]) + 1
        keep = gp % H + lag <= H - 1
        node.append(c[keep]); bins.append((gp + lag)[keep]); mult.append(np.ones(int(keep.sum()), dtype=np.int64))
        g0, g1, gen = g1, g1 + int(keep.sum()), gen + 1
        kids = dr.poisson(R[node[-1]], seed ^ K_CHILD_COUNT, gen, np.arange(g0, g1, dtype=np.uint64), branches)
    counts = np.zeros((N, T), dtype=np.int64)
    np.add.at(counts, (np.concatenate(node), np.concatenate(bins)), np.concatenate(mult))
    if info is not None:
        info.update(per_generation=per_gen, branches=branches, cells=N * T, cell_means=cm)
    return counts.reshape(N, S, H).transpose(1, 0, 2).copy(), carry


# ---- the cases both test files run ----------------------------------------------------------------------------------------------

def history(N, T0, seed, rate=1.5):
    """An observed count matrix: any non-negative integer matrix is data."""
    return np.random.default_rng(seed).poisson(rate, (N, T0)).astype(np.int64)


# name -> (make() arguments, T0, history rate, H, seed): the cases of the exact comparison, S = 3
RESTATE_S = 3
RESTATE_CASES = {
    "standard, H = 6 > L = 4": (dict(N=3, seed=1), 12, 1.5, 6, 3),
    "network, H = 3 < L = 4": (dict(N=5, seed=2, network=True, dt=0.5), 12, 1.5, 3, 4),
    "LGCP table": (dict(N=5, seed=4, lgcp_T=40), 12, 1.5, 6, 6),
    "T0 = 2 < L = 4": (dict(N=3, seed=1), 2, 1.5, 6, 5),
    "cell means from 10 on (PTRS)": (dict(N=3, seed=5, rate=14.0, scale=0.6), 12, 60.0, 6, 7),
}
# the ensemble-mean case of the issue: N = 4, L = 6, B = 2, H = 10, T0 = 9, S = 4000, dt = 0.5
MEAN_CASE = dict(make=dict(N=4, L=6, B=2, seed=21, dt=0.5, scale=0.68, rate=0.4), T0=9, hist_seed=5, H=10, S=4000, seed=17,
                 numpy_seed=123)
# W = 0: iid Poisson(λ0·dt) cells
IID = dict(mean=0.8, dt=0.5, N=3, H=8, S=2500, seed=9)
# λ0 = 0 and the single link 0 -> 2 (node 2 has no out-links): cell (2, T0+k) is Poisson(carry[k, 2])
LINK = dict(N=3, L=4, T0=6, H=6, S=4000, seed=10, weight=0.9, rate=6.0)
# martingale sums: the MEAN_CASE model and history (T0 = 9 >= L = 6, so the replicas can follow each other in one matrix)
MARTINGALE = dict(S=4000, seed=23)


def mean_case(nhp):
    m = MEAN_CASE
    p = dr.make(nhp, **m["make"])
    return p, history(m["make"]["N"], m["T0"], m["hist_seed"])


def iid_process(nhp):
    p = dr.make(nhp, IID["N"], scale=0.0, dt=IID["dt"])
    p.baseline = nhp.DiscreteHomogeneousProcess(np.full(IID["N"], IID["mean"] / IID["dt"]), IID["dt"])
    return p


def link_process(nhp):
    k = LINK
    p = dr.make(nhp, k["N"], L=k["L"], seed=3, rate=0.0)
    W = np.zeros((k["N"], k["N"]))
    W[0, 2] = k["weight"]
    p.weights = nhp.DenseWeightModel(W)
    return p, history(k["N"], k["T0"], 8, rate=k["rate"])


def chunk_case(nhp):
    """(process, data, H, S, seed, max_events): 4800 cells and more than 4096 child slots in generation 0 with fewer than 4096
    events in all, so that max_events = 4096 makes the chunk SIM_CHUNK_MIN and both loops take several chunks: the
    immigrants sit in the last bin but one of every replica (an LGCP table), two children per event, most of them past H."""
    N, T0, H, S = 8, 12, 6, 100
    p = dr.make(nhp, N, seed=13, scale=2.6, lgcp_T=T0 + H)
    lam = np.zeros((4, N))
    lam[2] = 2.2
    p.baseline = nhp.DiscreteLogGaussianCoxProcess(np.array([0.0, T0 + H - 2.0, T0 + H - 1.0, float(T0 + H)]), lam, None, 0.0, 1.0)
    data = np.zeros((N, T0), dtype=np.int64)
    data[0, T0 - p.nlags()] = 1                       # one observed event, which only its last lag carries across T0
    return p, data, H, S, 31, 4096


def iid_checks(paths, mean):
    """paths [S, N, H] of iid Poisson(mean) cells -> (z of the node totals, χ² verdict, z of the pooled variance against the mean)."""
    S, N, H = paths.shape
    flat = paths.transpose(1, 0, 2).reshape(N, S * H)
    z, chi2 = dr.immigrant_checks(flat, mean)
    n = flat.size
    # Var of the sample variance of a Poisson(m): (m + 2 m² · n/(n-1)) / n, to first order
    zv = (flat.var(ddof=1) - mean) / np.sqrt((mean + 2.0 * mean * mean) / n)
    return z, chi2, zv


def link_checks(paths, carry, c=2):
    """Cells (c, k) ~ Poisson(carry[k, c]) over S replicas -> (z of the means, z of the variances) for the bins with carry > 0."""
    S = paths.shape[0]
    m = carry[:, c]
    on = m > 0
    x = paths[:, c, :][:, on].astype(float)
    zm = (x.mean(axis=0) - m[on]) / np.sqrt(m[on] / S)
    zv = (x.var(axis=0, ddof=1) - m[on]) / np.sqrt((m[on] + 2.0 * m[on] ** 2) / S)
    return zm, zv, on


def chain(data, paths):
    """[data | path_0 | data | path_1 | ...] as one N x S·(T0+H) matrix and the mask of its forecast bins; T0 >= L keeps a
    replica's events out of reach of the next replica's forecast bins."""
    S, N, H = paths.shape
    T0 = data.shape[1]
    full = np.concatenate([np.broadcast_to(data[None], (S, N, T0)), paths], axis=2)          # [S, N, T0+H]
    mask = np.r_[np.zeros(T0, bool), np.ones(H, bool)]
    return full.transpose(1, 0, 2).reshape(N, S * (T0 + H)).copy(), np.tile(mask, S)


def martingale_z(counts, lam, L, mask):
    """dr.martingale_z with the sums over the masked (forecast) bins only; the lagged counts come from the whole matrix."""
    s = counts.astype(np.float64).T                   # [T, N]
    r = np.where(mask[:, None], s - lam, 0.0)
    lm = np.where(mask[:, None], lam, 0.0)
    zc = r.sum(axis=0) / np.sqrt(lm.sum(axis=0))
    T = s.shape[0]
    z = np.empty((L,) + (s.shape[1],) * 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        for l in range(1, L + 1):
            z[l - 1] = (s[:T - l].T @ r[l:]) / np.sqrt((s[:T - l] ** 2).T @ lm[l:])
    return zc, z


def assert_martingale(L, counts, mask, lam, lam_shifted):
    """|z| <= 5 for every statistic under the process' own intensity; more than 5 somewhere with the lag table one bin late."""
    zc, z = martingale_z(counts, lam, L, mask)
    fin = np.isfinite(z)
    print(f"martingale over the forecast bins: max |z_c| = {np.abs(zc).max():.2f}, max |z_pcl| = {np.abs(z[fin]).max():.2f} "
          f"over {zc.size + fin.sum()} statistics")
    assert fin.sum() >= 0.75 * z.size
    assert np.all(np.abs(zc) <= 5.0) and np.all(np.abs(z[fin]) <= 5.0)
    zc2, z2 = martingale_z(counts, lam_shifted, L, mask)
    print(f"lag table shifted by one bin: max |z_c| = {np.abs(zc2).max():.2f}, max |z_pcl| = {np.nanmax(np.abs(z2)):.2f}")
    assert max(np.abs(zc2).max(), np.nanmax(np.abs(z2))) > 5.0
