"""Restatements of the continuous chain scorer (csrc/cont_score.hip, include/nhp.h: nhp_cont_score_*), written from the
definitions and not from the kernels.

A cell is (block k, node c); under a draw

    ℓ_{k,c} = Σ_{events m of c, b_k <= t_m < b_{k+1}} log λ_c(t_m)  −  ΔΛ_{k,c}
    λ_c(t_m) = λ0_c + Σ_{i < m: t_i > thr} W·A·pdf(t_m − t_i),  thr = fl(t_m − Δtmax)                (exact delays; as the reference's
                 parent loop and nhp_cont_event_intensity, an event EARLIER IN THE LIST at the same time is a parent at d = 0:
                 θ for the exponential pdf, 0 for the logit-normal)
    ΔΛ_{k,c} = λ0_c·(b_{k+1} − b_k) + Σ_{i: t_i < b_{k+1}} W·A·(H(min(b_{k+1} − t_i, Δtmax)) − H(min(max(b_k − t_i, 0), Δtmax)))
    exponential   pdf = θ e^{−θd},  H(d) = 1 − e^{−θd}                       (cut at Δtmax, not renormalised)
    logit-normal  pdf = √(τ/2π)·exp(−τ/2·(logit x − μ)²)/(x(1 − x)), x = d/Δtmax;  H(d) = Δtmax·Φ(√τ(logit x − μ))

`cells(case, draw, real)` evaluates ℓ for every cell term by term in `real`: np.longdouble with Φ from mpmath (the reference;
H differences are formed as e^{−θ d1}·(−expm1(−θ(d2 − d1))) and as a difference of two mpmath Φ, so nothing cancels), or
np.float64 with Φ = 0.5·erfc(−z/√2) from scipy (what `score_numpy` streams).  Next to ℓ it returns the cell's scale
Σ|log λ_m| + ΔΛ, which the floors of `tolerances` are made of.  `score_mp` is the definitions of lppd, p, elpd and the joint
scores in mpmath at 50 digits over the long-double ℓ (the tables of tests/disc_score_ref.py); `score_numpy` is the device's
streaming algorithm in plain numpy fp64: running np.logaddexp and Welford's recursion per cell and for the draw's total.

mutate= plants exactly one mistake into `cells`:
    edge_earlier    an event exactly on an edge is scored in the earlier block (b_k < t <= b_{k+1})
    sat_straddle    an event inside the block contributes its saturated mass although its window straddles b_{k+1}
    no_clip         H is not clipped at b_k: an event before the block contributes H(d2), not H(d2) − H(d1)
    one_minus_exp   1 − exp(−x) for −expm1(−x)

A case is a dict: times [M] ascending, nodes [M] 1-based, T, dt_max, kind ("exponential" | "logitnormal"), edges [K + 1],
draws = [dict(lam0 [N], W [N, N], A [N, N] or None, theta | mu, tau [N, N])], matrices [parent, child].  Test code only."""
import math

import numpy as np
from mpmath import mp, mpf

import disc_score_ref as dref

MUTANTS = ("edge_earlier", "sat_straddle", "no_clip", "one_minus_exp")
FIELDS = dref.FIELDS


# ---- the inputs --------------------------------------------------------------------------------------------------------
def make_case(N, M, edges, S, kind, network, seed, T=None, dt_max=None, silent_node=None, zero_column=None, extra_times=()):
    """Scripted states: S draws that differ by tens of percent, a network's A with zeros.  `extra_times`: (time, node) pairs
    put among the random events (events exactly on an edge, exactly Δtmax before one)."""
    rng = np.random.default_rng(seed)
    T = float(T if T is not None else max(M, 1) / (2.0 * N))
    dt_max = float(dt_max if dt_max is not None else 4.0 * T / max(M, 1))
    times = np.sort(rng.uniform(0.0, T, M))
    nodes = rng.integers(1, N + 1, M)
    if silent_node is not None:
        nodes[nodes == silent_node] = silent_node % N + 1
    for t, n in extra_times:
        times, nodes = np.append(times, t), np.append(nodes, n)
    order = np.argsort(times, kind="stable")
    times, nodes = times[order], nodes[order].astype(np.int64)
    draws = []
    for _ in range(S):
        d = dict(lam0=rng.uniform(0.5, 2.0, N), W=rng.uniform(0.0, 0.9, (N, N)) / math.sqrt(N),
                 A=(rng.uniform(size=(N, N)) < 0.6).astype(np.float64) if network else None)
        if zero_column is not None and network:
            d["A"][:, zero_column - 1] = 0.0
        if kind == "exponential":
            d["theta"] = rng.uniform(0.5, 3.0, (N, N)) / (dt_max if np.isfinite(dt_max) else 4.0 * T / max(M, 1))
        else:
            d["mu"], d["tau"] = rng.normal(0.0, 1.0, (N, N)), rng.uniform(0.5, 3.0, (N, N))
        draws.append(d)
    return dict(times=times, nodes=nodes, T=T, dt_max=dt_max, kind=kind, edges=np.asarray(edges, dtype=np.float64), draws=draws)


def small_case(kind, network, seed=3, S=7):
    """N = 3, M ≈ 40: events exactly on an edge, one exactly Δtmax before an edge, an empty block, blocks narrower and wider
    than Δtmax, b_0 > 0 with history before it, b_K < T.  The host yardstick and the GPU test share this one case."""
    T, dt = 8.0, 0.5
    edges = [1.0, 1.25, 2.0, 2.5, 2.625, 4.0, 4.0625, 4.125, 7.0]            # (4.0625, 4.125) holds no event
    extra = [(2.0, 1), (2.0, 2), (2.5 - dt, 3), (4.0, 3), (7.0, 1)]
    case = make_case(3, 36, edges, S, kind, network, seed, T=T, dt_max=dt, extra_times=extra)
    inside = (case["times"] >= 4.0625) & (case["times"] < 4.125)
    case["times"], case["nodes"] = case["times"][~inside], case["nodes"][~inside]
    return case


# ---- ℓ per cell --------------------------------------------------------------------------------------------------------------
def _ncdf_diff(z1, z2, real):
    """Φ(z2) − Φ(z1) elementwise (z1 = −inf and z2 = +inf allowed)."""
    if real is np.float64:
        from scipy.special import erfc
        return 0.5 * erfc(-0.7071067811865476 * z2) - 0.5 * erfc(-0.7071067811865476 * z1)
    out = np.ones(len(z1), dtype=real)                          # Φ(+inf) − Φ(−inf): the whole mass, no mpmath needed
    lo_inf, hi_inf = np.isneginf(z1), np.isposinf(z2)
    with mp.workdps(30):
        for i in np.flatnonzero(~(lo_inf & hi_inf)):
            fa = mpf(0) if lo_inf[i] else mp.ncdf(_to_mp(z1[i]))
            fb = mpf(1) if hi_inf[i] else mp.ncdf(_to_mp(z2[i]))
            out[i] = _from_mp(fb - fa, real)
    return out


def _to_mp(v):
    hi = float(v)
    return mpf(hi) + mpf(float(v - type(v)(hi)))


def _from_mp(r, real):
    hi = float(r)
    return real(hi) + real(float(r - mpf(hi)))


def cells(case, draw, real=np.longdouble, mutate=None):
    """(ℓ [K, N], scale [K, N]) in `real`; scale = Σ|log λ_m| + ΔΛ of the cell."""
    sumlog, abslog, dlam = cell_parts(case, draw, real, mutate)
    return sumlog - dlam, abslog + dlam


def cell_parts(case, draw, real=np.longdouble, mutate=None):
    """(Σ log λ_m, Σ|log λ_m|, ΔΛ), each [K, N] in `real`."""
    assert mutate is None or mutate in MUTANTS
    t64, n0 = case["times"], case["nodes"] - 1
    edges, dt_max, expo = case["edges"], case["dt_max"], case["kind"] == "exponential"
    N, K, M = len(draw["lam0"]), len(case["edges"]) - 1, len(t64)
    t = t64.astype(real)
    WA = (draw["W"] if draw["A"] is None else draw["A"] * draw["W"]).astype(real)
    l0 = draw["lam0"].astype(real)
    if expo:
        th = draw["theta"].astype(real)
    else:
        mu, sq = draw["mu"].astype(real), np.sqrt(draw["tau"].astype(real))
        tau = draw["tau"].astype(real)
        with mp.workdps(30):
            two_pi = real(2.0 * math.pi) if real is np.float64 else _from_mp(2 * mp.pi, real)
    dtm = real(dt_max)
    # λ at every event
    loglam = np.empty(M, dtype=real)
    for m in range(M):
        c, thr = n0[m], t64[m] - dt_max                                          # fl(t_m − Δtmax): the data layout's threshold
        i = np.flatnonzero(t64[:m] > thr)                                          # earlier in the list: a tied event is a parent at d = 0
        p, d = n0[i], t[m] - t[i]
        w = WA[p, c]
        if expo:
            terms = w * th[p, c] * np.exp(-th[p, c] * d)
        else:
            x = d / dtm
            ok = (x > 0) & (x < 1)
            xs = np.where(ok, x, real(0.5))
            lg = np.log(xs / (1 - xs))
            terms = np.where(ok, w * np.sqrt(tau[p, c] / two_pi) * np.exp(-tau[p, c] / 2 * (lg - mu[p, c]) ** 2) / (xs * (1 - xs)), real(0))
        loglam[m] = np.log(l0[c] + (math.fsum(terms) if real is np.float64 else terms.sum()))
    sumlog, abslog, dlam = (np.zeros((K, N), dtype=real) for _ in range(3))
    for k in range(K):
        b0, b1 = real(edges[k]), real(edges[k + 1])
        inside = (t64 > edges[k]) & (t64 <= edges[k + 1]) if mutate == "edge_earlier" else (t64 >= edges[k]) & (t64 < edges[k + 1])
        for m in np.flatnonzero(inside):
            sumlog[k, n0[m]] += loglam[m]
            abslog[k, n0[m]] += abs(loglam[m])
        i = np.flatnonzero(t64 < edges[k + 1])
        d2r, d1r = b1 - t[i], b0 - t[i]
        keep = d1r < dtm                                                         # an event at least Δtmax before b_k has given everything
        i, d2r, d1r = i[keep], d2r[keep], d1r[keep]
        d2, d1 = np.minimum(d2r, dtm), np.maximum(d1r, real(0))
        if mutate == "no_clip":
            d1 = np.zeros_like(d1)
        if mutate == "sat_straddle":
            d2 = np.where(d1r <= 0, dtm, d2)
        dl = l0 * (b1 - b0)
        for c in range(N):
            w = WA[n0[i], c]
            nz = np.flatnonzero(w != 0)
            if not len(nz):
                continue
            p, a, b, wv = n0[i][nz], d1[nz], d2[nz], w[nz]
            if expo:
                r = th[p, c]
                tail = (1 - np.exp(-(r * (b - a)))) if mutate == "one_minus_exp" else -np.expm1(-(r * (b - a)))
                h = np.exp(-(r * a)) * tail
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    xa, xb = a / dtm, b / dtm
                    z1 = np.where(a > 0, sq[p, c] * (np.log(xa / (1 - xa)) - mu[p, c]), -np.inf)
                    z2 = np.where(b < dtm, sq[p, c] * (np.log(xb / (1 - xb)) - mu[p, c]), np.inf)
                h = dtm * _ncdf_diff(z1, z2, real)
            dl[c] += math.fsum(wv * h) if real is np.float64 else (wv * h).sum()
        dlam[k] = dl
    return sumlog, abslog, dlam


# ---- plain numpy fp64: the device's streaming algorithm ------------------------------------------------------------------------
def score_numpy(case, mutate=None):
    lse = mean = m2 = None
    jl = jm = j2 = 0.0
    for k, draw in enumerate(case["draws"]):
        ell = cells(case, draw, np.float64, mutate)[0]
        tot = float(ell.sum())
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
        lppd = lse - math.log(S)
        p = m2 / np.float64(S - 1)
        e = lppd - p
        ncell = e.size
        se = np.sqrt(ncell * np.var(e, ddof=1)) if ncell > 1 else np.nan
        summary = dict(n=S, cells=ncell, lppd=lppd.sum(), p_waic=p.sum(), elpd_waic=e.sum(), waic=-2.0 * e.sum(), se_elpd=se,
                       joint_lpd=jl - math.log(S), joint_mean=jm, joint_sd=np.sqrt(np.float64(j2) / np.float64(S - 1)))
    return dict(summary={k: float(v) for k, v in summary.items()}, per_node=np.stack([lppd.sum(axis=0), p.sum(axis=0), e.sum(axis=0)]),
                pointwise=e, mean=mean, lse=lse, m2=m2)


# ---- mpmath, 50 digits, over the long-double ℓ ---------------------------------------------------------------------------------
def score_mp(case):
    """The definitions at 50 digits (tests/disc_score_ref.score_mp_prefix) + "scale" [K, N]: the largest Σ|log λ| + ΔΛ of the
    cell over the draws, and "sum_abs" = Σ_i of the draws' mean |ℓ_i|."""
    tables, scale = [], None
    with mp.workdps(50):
        for draw in case["draws"]:
            ell, sc = cells(case, draw, np.longdouble)
            tables.append([[_to_mp(v) for v in row] for row in ell])
            scale = np.asarray(sc, dtype=np.float64) if scale is None else np.maximum(scale, np.asarray(sc, dtype=np.float64))
        S = len(tables)
        ref = dref.score_mp_prefix(tables, S)
        ref["sum_abs"] = float(mp.fsum([abs(x) for tab in tables for row in tab for x in row]) / S)
    ref["scale"] = scale
    return ref


errors = dref.errors
pointwise_errors = dref.pointwise_errors


def tolerances(yardstick, ref):
    """What the device may differ from the reference by: 16 times the error plain numpy fp64 makes on the same case and quantity,
    and not less than the continuous routes' parity bound 1e-11·max(1, ·) -- of Σ_i|ℓ_i| for the sums, and for a pointwise value
    of that cell's own Σ|log λ_m| + ΔΛ.  "pointwise" is a [K, N] array of bounds, one per cell."""
    floor_sum = 1e-11 * max(1.0, ref["sum_abs"])
    out = {}
    for k, y in yardstick.items():
        if math.isnan(y):
            out[k] = math.nan
        elif k == "pointwise":
            out[k] = np.maximum(16.0 * y, 1e-11 * np.maximum(1.0, ref["scale"]))
        else:
            out[k] = max(16.0 * y, floor_sum)
    return out


def exact_loglik_columns(case, draw, real=np.longdouble):
    """Σ_k ℓ_{k,c} of `cells` per node [N]: over edges covering [0, T] the exact log-likelihood Σ log λ_c − Λ_c(T)."""
    return cells(case, draw, real)[0].sum(axis=0)
