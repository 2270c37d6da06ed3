"""Restatements of the chain scorer (csrc/disc_score.hip, include/nhp.h: nhp_disc_score_*).

`score_numpy` is the device's algorithm in plain numpy fp64: the direct convolution, λ = base + Ŝ·E, ℓ = xlogy(s, λ) − λ, a
running np.logaddexp and Welford's recursion per cell and for the draw's total, loggamma restored at the end (math.lgamma).
`score_mp` is the definitions themselves in mpmath at 50 digits, with λ computed from the draws: the products and sums that
make λ are exact (integers scaled by powers of two; every double is one), rounded once to 50 digits, and everything after
that -- log, exp, the mean and the variance over the draws -- is mpmath.  The error of the first against the second is the
yardstick the device is held to (tests/test_disc_score_gpu.py); `tolerances` turns it into bounds.

A case is a dict: data [N, T] int, phi [L, B] (lags 1..L), dt, bins (t0, t1), draws = [(λ0 [N], W [N, N], θ [N, N, B],
A [N, N] or None), …]."""
import math

import numpy as np
from mpmath import mp, mpf
from mpmath.libmp import from_man_exp

FIELDS = ("n", "cells", "lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "joint_lpd", "joint_mean", "joint_sd")
K2 = 300                                        # every input is an integer over 2**K2 (checked)


# ---- the inputs --------------------------------------------------------------------------------------------------------
def gaussian_basis(L, B, dt=1.0):
    """B Gaussian bumps over lags 1..L, each summing to 1/dt: a stand-in basis for the host tests, which need no library.  The
    GPU tests pass the package's own basis(impulse) as `phi`."""
    lags = np.arange(1, L + 1, dtype=np.float64)
    means = np.linspace(1.0, L, B) if B > 1 else np.array([(1.0 + L) / 2.0])
    sd = L / (B + 1.0) if B > 1 else L / 2.0
    phi = np.exp(-0.5 * ((lags[:, None] - means[None, :]) / sd) ** 2)
    return phi / (phi.sum(axis=0, keepdims=True) * dt)


def make_case(N, T, B, L, bins, S, network, seed, rate=0.3, dt=1.0, phi=None):
    """Hand-made states: S draws that differ by tens of percent, a network's A with zeros, counts with empty cells, ones
    and larger values."""
    rng = np.random.default_rng(seed)
    data = rng.poisson(rate, (N, T)).astype(np.int64)
    data[rng.uniform(size=(N, T)) < 0.02] += 3
    draws = []
    for _ in range(S):
        th = rng.dirichlet(np.ones(B), (N, N))
        A = (rng.uniform(size=(N, N)) < 0.6).astype(np.float64) if network else None
        draws.append((rng.uniform(0.05, 0.4, N), rng.uniform(0.0, 0.8, (N, N)) / N, th, A))
    return dict(data=data, phi=gaussian_basis(L, B, dt) if phi is None else np.asarray(phi, dtype=np.float64), dt=dt,
                bins=bins if bins is not None else (0, T), draws=draws)


def convolve_numpy(data, phi):
    """Ŝ[t, p, b] = Σ_{l=1..min(L,t)} data[p, t−l]·φ[l, b] (0-based t), summed in lag order."""
    N, T = data.shape
    L, B = phi.shape
    S = np.zeros((T, N, B))
    d = data.T.astype(np.float64)
    for l in range(1, L + 1):
        S[l:] += d[:T - l, :, None] * phi[l - 1][None, None, :]
    return S


# ---- plain numpy fp64 --------------------------------------------------------------------------------------------------
def loglik_cells_numpy(case, draw):
    """ℓ without loggamma over the scored cells, [R, N], as the device forms it."""
    data, phi, dt = case["data"], case["phi"], case["dt"]
    t0, t1 = case["bins"]
    N, T = data.shape
    B = phi.shape[1]
    l0, W, th, A = draw
    G = convolve_numpy(data, phi)[t0:t1].reshape(t1 - t0, N * B)                  # column p·B + b
    w = W if A is None else A * W
    E = ((w[:, :, None] * th) * dt).transpose(0, 2, 1).reshape(N * B, N)            # row p·B + b
    lam = (l0 * dt)[None, :] + G @ E
    s = data[:, t0:t1].T.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s == 0.0, 0.0, s * np.log(lam)) - lam


def score_numpy(case):
    t0, t1 = case["bins"]
    s = case["data"][:, t0:t1].T
    lg = np.vectorize(lambda v: math.lgamma(v + 1.0))(s.astype(np.float64))
    lg_total = float(lg.sum())
    lse = mean = m2 = None
    jl = jm = j2 = 0.0
    for k, draw in enumerate(case["draws"]):
        ell = loglik_cells_numpy(case, draw)
        tot = float(ell.sum()) - lg_total
        n = float(k + 1)
        if k == 0:
            lse, mean, m2 = ell.copy(), ell.copy(), np.zeros_like(ell)
            jl, jm, j2 = tot, tot, 0.0
        else:
            lse = np.logaddexp(lse, ell)
            d = ell - mean
            mean = mean + d / n
            m2 = m2 + d * (ell - mean)
            jl = float(np.logaddexp(jl, tot))
            d = tot - jm
            jm = jm + d / n
            j2 = j2 + d * (tot - jm)
    S = len(case["draws"])
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd = lse - math.log(S) - lg
        p = m2 / np.float64(S - 1)
        e = lppd - p
        cells = e.size
        se = np.sqrt(cells * np.var(e, ddof=1)) if cells > 1 else np.nan
        summary = dict(n=S, cells=cells, lppd=lppd.sum(), p_waic=p.sum(), elpd_waic=e.sum(), waic=-2.0 * e.sum(), se_elpd=se,
                       joint_lpd=jl - math.log(S), joint_mean=jm, joint_sd=np.sqrt(np.float64(j2) / np.float64(S - 1)))
    return dict(summary={k: float(v) for k, v in summary.items()}, per_node=np.stack([lppd.sum(axis=0), p.sum(axis=0), e.sum(axis=0)]),
                pointwise=e, mean=mean - lg, lppd_i=lppd, p_i=p)


# ---- mpmath, 50 digits ---------------------------------------------------------------------------------------------------
def _scaled(x):
    """The doubles of x as exact integers over 2**K2 (object array)."""
    out = np.empty(np.shape(x), dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(np.asarray(x, dtype=np.float64).reshape(-1)):
        num, den = float(v).as_integer_ratio()
        assert (1 << K2) % den == 0, "input below 2**-K2"
        flat[i] = num * ((1 << K2) // den)
    return out


def lambda_exact(case, draw):
    """λ over the scored cells as exact integers over 2**(4·K2), [R, N] (object array): Σ_l Σ_p data[p, t−l]·H[p, c, l] with
    H[p, c, l] = Σ_b φ[l, b]·(A·W)[p, c]·θ[p, c, b]·dt, walked over the occupied bins only."""
    data, phi, dt = case["data"], case["phi"], case["dt"]
    t0, t1 = case["bins"]
    N, T = data.shape
    L, B = phi.shape
    l0, W, th, A = draw
    one = 1 << K2
    w = _scaled(W if A is None else A * W)                       # (A is 0 or 1: the product is exact)
    E = (w[:, :, None] * _scaled(th)) * _scaled(dt)[()]          # 3·K2
    ph = _scaled(phi)
    H = np.zeros((N, N, L), dtype=object)
    for l in range(L):
        for b in range(B):
            H[:, :, l] = H[:, :, l] + E[:, :, b] * ph[l, b]      # 4·K2
    lam = np.empty((t1 - t0, N), dtype=object)
    lam[:] = (_scaled(l0) * _scaled(dt)[()] * (one * one))[None, :]
    for p, tau in zip(*np.nonzero(data)):
        cnt = int(data[p, tau])
        for l in range(1, L + 1):
            t = tau + l
            if t0 <= t < t1:
                lam[t - t0] = lam[t - t0] + cnt * H[p, :, l - 1]
    return lam


def cells_mp(case):
    """ℓ_i(θ_s) with its loggamma, at 50 digits: one [R][N] table of mpf per draw."""
    t0, t1 = case["bins"]
    s = case["data"][:, t0:t1].T
    R, N = s.shape
    with mp.workdps(50):
        lgf = {int(v): mp.loggamma(int(v) + 1) for v in np.unique(s)}
        ells, log, make, prec = [], mp.log, mp.make_mpf, mp.prec
        for draw in case["draws"]:
            lam = lambda_exact(case, draw)
            rows = []
            for r in range(R):
                row = []
                for c in range(N):
                    x = make(from_man_exp(int(lam[r, c]), -4 * K2, prec, "n"))
                    sv = int(s[r, c])
                    row.append(sv * log(x) - x - lgf[sv] if sv else -x)
                rows.append(row)
            ells.append(rows)
    return ells


def score_mp_prefix(ells, S):
    """The definitions over the first S draws of cells_mp's tables."""
    R, N = len(ells[0]), len(ells[0][0])
    cells = R * N
    exp, log, fsum, nan = mp.exp, mp.log, mp.fsum, mp.nan
    with mp.workdps(50):
        logS = log(S)
        lppd = np.empty((R, N), dtype=object)
        p = np.empty((R, N), dtype=object)
        mean = np.empty((R, N), dtype=object)
        for r in range(R):
            for c in range(N):
                if S == 1:
                    lppd[r, c] = mean[r, c] = ells[0][r][c]
                    p[r, c] = nan
                    continue
                v = [ells[k][r][c] for k in range(S)]
                top = max(v)
                lppd[r, c] = top + log(fsum([exp(x - top) for x in v])) - logS
                m = fsum(v) / S
                mean[r, c] = m
                p[r, c] = fsum([(x - m) ** 2 for x in v]) / (S - 1)
        e = lppd - p
        tot = [fsum([x for row in ells[k] for x in row]) for k in range(S)]
        top = max(tot)
        jm = fsum(tot) / S
        flat = list(e.reshape(-1))
        esum = fsum(flat) if S > 1 else nan
        em = esum / cells
        summary = dict(n=S, cells=cells, lppd=fsum(list(lppd.reshape(-1))), p_waic=fsum(list(p.reshape(-1))) if S > 1 else nan,
                       elpd_waic=esum, waic=-2 * esum,
                       se_elpd=mp.sqrt(cells * fsum([(x - em) ** 2 for x in flat]) / (cells - 1)) if S > 1 and cells > 1 else nan,
                       joint_lpd=top + log(fsum([exp(x - top) for x in tot])) - logS, joint_mean=jm,
                       joint_sd=mp.sqrt(fsum([(x - jm) ** 2 for x in tot]) / (S - 1)) if S > 1 else nan)
        absl = fsum([abs(x) for x in mean.reshape(-1)])
        return dict(summary=summary, per_node=[[fsum(list(a[:, c])) if (S > 1 or a is lppd) else nan for c in range(N)] for a in (lppd, p, e)],
                    pointwise=e, mean=mean, lppd_i=lppd, sum_abs_ell=float(absl))


def score_mp(case, prefixes=None):
    """{S: the definitions at 50 digits over the first S draws} for every S in `prefixes` (default: all the draws); λ and ℓ of
    a draw are computed once."""
    ells = cells_mp(case)
    return {S: score_mp_prefix(ells, S) for S in (tuple(prefixes) if prefixes is not None else (len(ells),))}


# ---- errors and bounds -----------------------------------------------------------------------------------------------------
def _err(got, want):
    """|got − want| with want in mpmath, as a float; NaN where both are NaN, inf where only one is."""
    got = float(got)
    if mp.isnan(want) or math.isnan(got):
        return math.nan if (mp.isnan(want) and math.isnan(got)) else math.inf
    with mp.workdps(50):
        return float(abs(mpf(got) - want))


def pointwise_errors(result, ref):
    """|elpd_i − reference| per cell, [R, N]; NaN where both are NaN, inf where only one is."""
    pw = np.asarray(result["pointwise"], dtype=np.float64)
    return np.array([[_err(pw[r, c], ref["pointwise"][r, c]) for c in range(pw.shape[1])] for r in range(pw.shape[0])])


def errors(result, ref):
    """Per quantity the largest |result − ref|: the ten summary fields, "per_node" and "pointwise" (whose cells
    pointwise_errors gives one by one).  `result` holds floats (score_numpy's or the device's), `ref` is one entry of
    score_mp's."""
    out = {k: _err(result["summary"][k], ref["summary"][k]) for k in FIELDS}
    pn = np.asarray(result["per_node"], dtype=np.float64)
    out["per_node"] = _worst([_err(pn[a, c], ref["per_node"][a][c]) for a in range(3) for c in range(pn.shape[1])])
    out["pointwise"] = _worst(list(pointwise_errors(result, ref).reshape(-1)))
    return out


def _worst(errs):
    if any(math.isinf(x) for x in errs):
        return math.inf
    finite = [x for x in errs if not math.isnan(x)]
    return max(finite) if finite else math.nan


def tolerances(yardstick, ref):
    """What the device may differ from mpmath by: 16 times the error plain numpy fp64 makes on the same case and quantity,
    and not less than the project's standing parity bound for the discrete intensity and log-likelihood, 1e-12 -- of Σ|ℓ| over
    the scored cells for the sums, and for a pointwise value of that cell's own |ℓ_i| (the mean over the draws).  "pointwise"
    is therefore an [R, N] array of bounds, one per cell: 16 times the largest numpy error over the cells, or the cell's own
    floor where that is larger."""
    floor_sum = 1e-12 * ref["sum_abs_ell"]
    out = {}
    for k, y in yardstick.items():
        if math.isnan(y):
            out[k] = math.nan
        elif k == "pointwise":
            with mp.workdps(50):
                floor = np.array([[1e-12 * float(abs(x)) for x in row] for row in ref["mean"]])
            out[k] = np.maximum(16.0 * y, floor)
        else:
            out[k] = max(16.0 * y, floor_sum)
    return out
