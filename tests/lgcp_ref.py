"""Extended-precision restatements for the Gibbs update of a log Gaussian Cox baseline, written from the formulas and
not from the kernels or the oracle's C:

    f_c(t)      piecewise linear through (x[g], lam[c, g]):  x[a] <= t < x[a+1] gives
                (lam[a+1]·(t - x[a]) + lam[a]·(x[a+1] - t)) / (x[a+1] - x[a]);  t >= x[G-1] gives lam[G-1]
    continuous  ll[c] = -Σ_g (lam[c,g] + lam[c,g+1])/2·(x[g+1] - x[g]) + Σ_i log f_c(t_i)
                over the events i on node c whose parent node is 0 (the baseline)
    discrete    ll[n] = Σ_t s·log λ_t - λ_t - lnΓ(s + 1),   s = base_counts[t, n],   λ_t the interpolant of cand[:, n]·dt at
                time_t = fl(x[0] + fl(t·dt)), t = 0..T-1, in float64 as the bins are laid out (exact for the dyadic dt and
                x[0] = 0 of the suites); s = 0 contributes -λ_t
    slice       Murray, Adams, MacKay (2010), per node: v ~ N(0, Σ), u ~ U(0,1), level = ll(y) + log u, θ = 2π·U(0,1),
                bracket [θ - 2π, θ]; propose y·cos θ + v·sin θ, accept on ll_new >= level; on reject the bracket shrinks to θ
                (θmin when θ < 0, θmax otherwise) and θ is redrawn uniformly inside it

Rounding bounds (float64, u = 2⁻⁵³; first order and worst case; derived, not measured).  lam and cand are float64 inputs of
both sides, so they carry no error.

  continuous.  One interpolated value takes: the two differences t - x[a], x[a+1] - t (1 rounding each), their products
    with lam (1 each), the sum of the two products (1), the width x[a+1] - x[a] (1) and the division (1).  lam > 0 and the
    weights are non-negative, so the numerator is a sum of non-negative numbers and nothing cancels: the two product
    terms carry 2 roundings each, their sum at most 2 + 1, and the quotient 3 + 1 + 1 = RHO_F = 5 relative roundings.  They
    move log f by 5u absolutely.  nhp_log (csrc/nhp_math.h) is fdlibm's algorithm, the argument reduction with Lg1..Lg7; the
    header states no error for it, and the figure used here is fdlibm's own statement about that algorithm, an error below
    one ulp: one ulp <= 2u·|log f|.  A sum of n terms in any order adds (n - 1)·u·Σ|log f|.  One trapezoid
    (lam[g] + lam[g+1] (1), ·0.5 (exact), x[g+1] - x[g] (1), the product (1)) carries RHO_TRAP = 3, the sum of the G - 1
    positive trapezoids G - 2 more, and the final (0 - I) + s one rounding on |I| + |s|.  With c = 2 (that last addition and
    one for the second-order terms):

        bound[c] = u·[ Σ_i (5 + 2|log f_i|) + (n + 2)·Σ_i |log f_i| + (3 + (G - 1) + 2)·I ]

    A node without baseline events has n = 0 and Σ = 0: its value is -I, and a float64 sum of the trapezoids in grid order
    (`sequential_trapezoid`) is what an implementation that adds them in that order returns, bit for bit.

  discrete.  time_t is the convention above (no error).  λ_t takes cand·dt (1), the difference (1), the product (1), the sum
    of two non-negative products (1), the width (1) and the division (1): RHO_LAM = 6, and 2 at or beyond the last grid
    point.  The term s·log λ_t - λ_t - lnΓ(s+1): the argument moves log λ by 6u (times s), the logarithm adds 2u·|log λ|
    and the product with s one more: s·(6 + 3|log λ|)u; λ_t itself 6u·λ_t; lnΓ(s + 1) comes from the device library,
    whose error nothing in the repository states: LGAMMA_ULP = 4 ulp = 8u·lnΓ is an ASSUMPTION, not derived (and that it is
    0 exactly at s = 0 and s = 1); it decides nothing at T >= 8, where the (T + 2) term below is larger; the two
    subtractions 2u·(|s log λ| + λ + lnΓ).  The sum
    of T terms in any order adds (T - 1)·u·Σ|term parts|.  With c = 2:

        bound[n] = u·[ Σ_t s(6 + 3|log λ_t|) + 6 λ_t + 8 lnΓ(s+1) + (T + 2)·(s|log λ_t| + λ_t + lnΓ(s+1)) ]

Everything is evaluated in numpy's long double where that is the x87 80-bit format or wider, otherwise in mpmath numbers
(tests/adjacency_ref.backend); real=np.float64 gives the plain double evaluation of the same sums, `order` the order in which
the terms enter them.  Test code only."""
import collections
import functools
import math

import numpy as np

from adjacency_ref import backend

EPS = 2.0 ** -53
RHO_F, RHO_TRAP, RHO_LAM, LGAMMA_ULP, C_SUM = 5.0, 3.0, 6.0, 4.0, 2.0

CandLL = collections.namedtuple("CandLL", "ll bound n S I")
"""ll in the evaluation's number type [N]; bound, n (terms), S = Σ|log f| (or Σ|term parts|), I (integral term) float64 [N]."""


def _f64(v):
    return np.asarray(v, dtype=np.float64)


def _lgamma1(b, s):
    """lnΓ(s + 1) = log s! of non-negative integers, in the backend's numbers, from the definition: a running sum of logs."""
    s = np.asarray(s, dtype=np.int64)
    top = int(s.max()) if s.size else 0
    table = b.zeros(top + 2)
    for k in range(2, top + 1):
        table[k] = table[k - 1] + b.log(b.arr(np.array([float(k)])))[0]
    return table[s]


def interpolate(b, gx, y, t):
    """f(t) of the module docstring for float64 times t, y in the backend's numbers; t inside [gx[0], inf)."""
    gx = _f64(gx)
    G = len(gx)
    t = _f64(t)
    assert np.all(t >= gx[0])
    last = ~(t < gx[G - 1])
    a = np.clip(np.searchsorted(gx, t, side="right") - 1, 0, G - 2)
    x0, x1, tt = b.arr(gx[a]), b.arr(gx[a + 1]), b.arr(t)
    f = (y[a + 1] * (tt - x0) + y[a] * (x1 - tt)) / (x1 - x0)
    if last.any():
        f[last] = y[G - 1]
    return f, last


def _ordered(v, order):
    return v[::-1] if order == "reversed" else v


def _sum(b, v, order):
    """The sum of v term by term in the given order (numpy's pairwise sum would not be `the same sums in that order`)."""
    acc = b.num(0.0)
    for q in _ordered(v, order):
        acc = acc + q
    return acc


def sequential_trapezoid(grid_x, y):
    """Σ_g 0.5·(y[g] + y[g+1])·(x[g+1] - x[g]) in float64, added in grid order."""
    I = 0.0
    for g in range(len(grid_x) - 1):
        I += 0.5 * (float(y[g]) + float(y[g + 1])) * (float(grid_x[g + 1]) - float(grid_x[g]))
    return I


def cont_candidate_ll(times, nodes, parentnodes, N, grid_x, lam, real=None, order="forward"):
    """ll[c] and its bound (CandLL); nodes and parentnodes 1-based, parent node 0 = the baseline; lam [N, G]."""
    b = backend(real)
    t, n0, pn = _f64(times), np.asarray(nodes, dtype=np.int64) - 1, np.asarray(parentnodes, dtype=np.int64)
    gx, lam = _f64(grid_x), _f64(lam).reshape(N, -1)
    G = len(gx)
    assert lam.shape[1] == G and G >= 2 and np.all(np.diff(gx) > 0)
    ll = b.zeros(N)
    out = {k: np.zeros(N) for k in ("bound", "n", "S", "I")}
    half = b.num(0.5)
    for c in range(N):
        y = b.arr(lam[c])
        traps = (y[:-1] + y[1:]) * half * (b.arr(gx[1:]) - b.arr(gx[:-1]))
        I = _sum(b, traps, order)
        tc = t[(n0 == c) & (pn == 0)]
        f, _ = interpolate(b, gx, y, tc)
        lf = b.log(f) if len(tc) else b.zeros(0)
        ll[c] = (b.num(0.0) - I) + _sum(b, lf, order)
        alf = np.abs(_f64(lf))
        n, S, I64 = float(len(tc)), float(alf.sum()), float(I)
        out["n"][c], out["S"][c], out["I"][c] = n, S, I64
        out["bound"][c] = EPS * ((RHO_F * n + 2.0 * S) + (n + C_SUM) * S + (RHO_TRAP + (G - 1) + C_SUM) * I64)
    return CandLL(ll=ll, **out)


def bin_times(grid_x, T, dt):
    """time_t = fl(x[0] + fl(t·dt)), t = 0..T-1, float64."""
    return float(grid_x[0]) + np.arange(int(T), dtype=np.float64) * float(dt)


def disc_candidate_ll(base_counts, grid_x, cand, dt, real=None, order="forward"):
    """ll[n] and its bound (CandLL; I = Σ λ_t); base_counts [T, N] non-negative integers, cand [G, N]."""
    b = backend(real)
    s_all = np.asarray(base_counts, dtype=np.int64)
    T, N = s_all.shape
    gx, cand = _f64(grid_x), _f64(cand)
    G = len(gx)
    assert cand.shape == (G, N) and np.all(s_all >= 0) and np.all(np.diff(gx) > 0)
    time = bin_times(gx, T, dt)
    assert time[-1] <= gx[G - 1]
    ll = b.zeros(N)
    out = {k: np.zeros(N) for k in ("bound", "n", "S", "I")}
    bdt = b.num(float(dt))
    for n in range(N):
        lam, last = interpolate(b, gx, b.arr(cand[:, n]) * bdt, time)
        s = s_all[:, n]
        llam = b.log(lam)
        sl = b.arr(s.astype(np.float64)) * llam
        sl[s == 0] = b.zeros(int((s == 0).sum()))
        lg = _lgamma1(b, s)
        ll[n] = _sum(b, sl - lam - lg, order)
        s64, al, l64, g64 = s.astype(np.float64), np.abs(_f64(llam)), _f64(lam), _f64(lg)
        parts = s64 * al + l64 + g64
        rho = np.where(last, 2.0, RHO_LAM)
        out["n"][n], out["S"][n], out["I"][n] = T, parts.sum(), l64.sum()
        out["bound"][n] = EPS * float((s64 * (rho + 3.0 * al) + rho * l64 + 2.0 * LGAMMA_ULP * g64 + (T + C_SUM) * parts).sum())
    return CandLL(ll=ll, **out)


def ratio(got, res):
    """Largest |got - ref| / bound over the values (bound > 0 everywhere: I > 0), and the indices outside."""
    err = np.abs(np.asarray(np.asarray(got, dtype=np.float64) - res.ll, dtype=np.float64))
    assert np.all(res.bound > 0)
    r = err / res.bound
    return float(r.max()), np.nonzero(~(err <= res.bound))[0]


# ------------------------------------------------------------------------------------------------------- elliptical slice
class ScriptedRng:
    """np.random.default_rng(seed) that records every standard_normal and uniform array it hands out, in order."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.record = []

    def standard_normal(self, size=None):
        z = self.rng.standard_normal(size)
        self.record.append(("normal", np.array(z, copy=True)))
        return z

    def uniform(self, low=0.0, high=1.0, size=None):
        u = self.rng.uniform(low, high, size)
        self.record.append(("uniform", np.array(u, copy=True)))
        return u


def draw_script(seed, N, G, rounds, layout="rows"):
    """A record of the shape one update makes: one normal array ([N, G] rows / [G, N] columns), then `rounds + 1` uniform
    arrays of N (log u, the first θ, one per later round)."""
    rng = ScriptedRng(seed)
    rng.standard_normal((N, G) if layout == "rows" else (G, N))
    for _ in range(rounds + 1):
        rng.uniform(size=N)
    return rng.record


SliceNode = collections.namedtuple("SliceNode", "theta rounds y margin shrunk_min shrunk_max")


def elliptical_slice_serial(Y, L, record, loglik, layout="rows", max_attempts=100, use_log_u=True):
    """The per-node loop, one node after another.  Y: latent curves ([N, G] rows or [G, N] columns), L = chol(Σ), record: a
    ScriptedRng record (one normal array in Y's layout, then uniform arrays of N), loglik(c, y) the candidate likelihood of
    node c (any real type).  Node c reads entry c of uniform array r + 1 in round r >= 1 (array 0 is u) -- only while it
    is undecided, so an array it does not reach is never read.  Returns one SliceNode per node: accepted θ, rounds, new
    curve, the smallest |ll_new - level| met, and how often each bracket end moved.  A node that uses up max_attempts
    raises RuntimeError.  use_log_u=False is the mutant whose level leaves log u out."""
    Y = _f64(Y)
    rows = layout == "rows"
    N = Y.shape[0] if rows else Y.shape[1]
    kind, Z = record[0]
    assert kind == "normal" and Z.shape == Y.shape
    unis = [a for k, a in record[1:] if k == "uniform"]
    out = []
    for c in range(N):
        y = Y[c] if rows else Y[:, c]
        v = np.dot(L, Z[c] if rows else Z[:, c])
        level = loglik(c, y) + (np.log(unis[0][c]) if use_log_u else 0.0)
        theta = 2 * np.pi * unis[1][c]
        tmin, tmax = theta - 2 * np.pi, theta
        rounds, margin, nmin, nmax = 1, np.inf, 0, 0
        while True:
            ynew = y * np.cos(theta) + v * np.sin(theta)
            d = loglik(c, ynew) - level
            margin = min(margin, abs(float(d)))
            if d >= 0:
                break
            if rounds >= max_attempts:
                raise RuntimeError("Elliptical slice sampling reached maximum attempts.")
            if theta < 0.0:
                tmin, nmin = theta, nmin + 1
            else:
                tmax, nmax = theta, nmax + 1
            rounds += 1
            theta = tmin + (tmax - tmin) * unis[rounds][c]
        out.append(SliceNode(theta, rounds, ynew, margin, nmin, nmax))
    return out


# ---------------------------------------------------------------------------------------- two-point posterior, invariance
def two_point_cont_loglik(X, m, events, weights_swapped=False):
    """ll(y0, y1) of a node on the grid [0, X] with baseline events `events` under λ = exp(m + y); works on floats and on
    arrays.  weights_swapped is the mutant that gives each event the other end's weight."""
    w1 = [e / X for e in events]
    if weights_swapped:
        w1 = [1.0 - w for w in w1]

    def ll(y0, y1):
        xp = np if isinstance(y0, np.ndarray) else math
        l0, l1 = xp.exp(m + y0), xp.exp(m + y1)
        out = -0.5 * (l0 + l1) * X
        for w in w1:
            out = out + xp.log(l1 * w + l0 * (1.0 - w))
        return out
    return ll


def two_point_disc_loglik(X, m, counts, dt):
    """ll(y0, y1), up to the constant Σ lnΓ(s+1), of Poisson counts in the bins at t·dt on the grid [0, X]."""
    w1 = [t * dt / X for t in range(len(counts))]

    def ll(y0, y1):
        xp = np if isinstance(y0, np.ndarray) else math
        l0, l1 = xp.exp(m + y0) * dt, xp.exp(m + y1) * dt
        out = 0.0
        for w, s in zip(w1, counts):
            lam = l1 * w + l0 * (1.0 - w)
            out = out - lam + (s * xp.log(lam) if s else 0.0)
        return out
    return ll


def posterior_cdfs(ll, Sigma, n=1600, width=6.0):
    """Marginal posterior cdfs of y0 and y1 under the prior N(0, Σ) (2 x 2) and the likelihood ll(y0, y1): 2-D quadrature
    (midpoints) on n² points over ±width prior standard deviations.  Returns two functions of arrays."""
    Sigma = _f64(Sigma)
    P = np.linalg.inv(Sigma)
    s0, s1 = np.sqrt(Sigma[0, 0]), np.sqrt(Sigma[1, 1])
    g0 = (np.arange(n) + 0.5) / n * 2 * width * s0 - width * s0
    g1 = (np.arange(n) + 0.5) / n * 2 * width * s1 - width * s1
    A, B = np.meshgrid(g0, g1, indexing="ij")
    logp = ll(A, B) - 0.5 * (P[0, 0] * A * A + 2 * P[0, 1] * A * B + P[1, 1] * B * B)
    p = np.exp(logp - logp.max())
    cdfs = []
    for grid, marg, h in ((g0, p.sum(axis=1), g0[1] - g0[0]), (g1, p.sum(axis=0), g1[1] - g1[0])):
        c = np.cumsum(marg) / marg.sum()                                   # the cdf at the cells' right edges
        edges = np.concatenate([[grid[0] - h / 2], grid + h / 2])
        vals = np.concatenate([[0.0], c])
        cdfs.append(lambda v, e=edges, q=vals: np.interp(v, e, q))
    return cdfs


BURN, KEPT_SWEEPS, THIN = 30, 50, 5
P_MIN = 1e-4            # tests/test_device_draws_gpu.py


def invariance_pvalues(sweep, Y0, cdfs):
    """Runs `sweep(Y) -> Y` (Y [R, 2], one replica per row) BURN times, then KEPT_SWEEPS times keeping every THIN-th state,
    and returns the Kolmogorov-Smirnov p-values of the kept y0 and y1 against cdfs."""
    from scipy import stats
    Y = np.array(Y0, dtype=np.float64)
    kept = []
    for s in range(BURN + KEPT_SWEEPS):
        Y = sweep(Y)
        if s >= BURN and (s - BURN) % THIN == THIN - 1:
            kept.append(Y.copy())
    K = np.concatenate(kept)
    return tuple(float(stats.kstest(cdfs[k](K[:, k]), "uniform").pvalue) for k in (0, 1))


def serial_sweeper(ll, L, seed, replicas, use_log_u=True):
    """A `sweep` for invariance_pvalues that runs elliptical_slice_serial with the two-point likelihood ll(y0, y1)."""
    state = {"k": 0}

    def sweep(Y):
        state["k"] += 1
        # 40 rounds of draws: a correct bracket has shrunk below double resolution long before
        rec = draw_script(seed * 100003 + state["k"], replicas, 2, 40)
        res = elliptical_slice_serial(Y, L, rec, lambda c, y: ll(float(y[0]), float(y[1])), max_attempts=40, use_log_u=use_log_u)
        return np.vstack([r.y for r in res])
    return sweep


# ---------------------------------------------------------------------------------------------------------------- cases
def _finish(case, rng, all_base, none_base):
    """Sorts the events, draws the attribution (half to the baseline, parents among the nodes otherwise) and forces node
    `all_base` wholly to the baseline and node `none_base` wholly away from it (1-based)."""
    t, nodes, N = case["times"], case["nodes"], case["N"]
    o = np.argsort(t, kind="stable")
    t, nodes = t[o], nodes[o]
    pn = (rng.integers(1, N + 1, len(t)) * (rng.uniform(size=len(t)) < 0.5)).astype(np.int64)
    if all_base is not None:
        pn[nodes == all_base] = 0
    if none_base is not None:
        pn[nodes == none_base] = rng.integers(1, N + 1, int((nodes == none_base).sum()))
    G = len(case["grid_x"])
    Y = rng.normal(0.0, 0.6, (N, G))                  # lam is what a baseline with m = 0 makes of the latent curves Y
    case.update(times=t, nodes=nodes, parentnodes=pn, Y=Y, lam=np.exp(0.0 + Y), all_base=all_base, none_base=none_base)
    gx = case["grid_x"]
    cnt = np.bincount(nodes - 1, minlength=N)
    on = np.isin(t, gx[1:-1])
    case["counts"] = dict(
        M=len(t), silent=int((cnt == 0).sum()), at_zero=int((t == 0.0).sum()), on_interior=int(on.sum()),
        interior_points_hit=int(len(np.unique(t[on]))),
        doubled=int(sum(1 for v in np.unique(t[on]) if len(set(nodes[t == v])) >= 2)),
        last_cell=int((t >= gx[-2]).sum()), at_end=int((t == gx[-1]).sum()),
        base_events=int((pn == 0).sum()),
        none_attributed=int(sum(1 for c in range(N) if cnt[c] > 0 and not np.any((nodes == c + 1) & (pn == 0)))),
        all_attributed=int(sum(1 for c in range(N) if cnt[c] > 0 and np.all(pn[nodes == c + 1] == 0))))
    return case


KNOTS_X = np.array([0.0, 0.5, 8.0, 8.25, 40.0, 63.5, 64.0])


def knots(seed=11, M=1500):
    """N = 5 (node 5 silent), T = 64, Δtmax = 1.5, G = 7 with cells of width 0.5, 7.5, 0.25, 31.75, 23.5, 0.5 (all dyadic).
    A first event at 0, events exactly on x[1] (node 1), x[2] (nodes 2 and 3: twice), x[3] (node 4) and x[4] (node 1),
    twelve more events in the last cell and the last event at x[6] = T."""
    rng = np.random.default_rng(seed)
    N, T = 5, 64.0
    t = np.sort(rng.uniform(0.0, T, M))
    nodes = rng.integers(1, 5, M).astype(np.int64)
    t[0] = 0.0
    for i, (v, c) in zip((200, 500, 501, 700, 1000), ((KNOTS_X[1], 1), (KNOTS_X[2], 2), (KNOTS_X[2], 3), (KNOTS_X[3], 4), (KNOTS_X[4], 1))):
        t[i], nodes[i] = v, c
    t[-13:-1] = np.sort(rng.uniform(63.5, 64.0, 12))
    t[-1] = T
    case = dict(name="knots", N=N, T=T, dt_max=1.5, grid_x=KNOTS_X.copy(), times=t, nodes=nodes)
    return _finish(case, rng, all_base=1, none_base=2)


def one_cell():
    rng = np.random.default_rng(12)
    N, T, M = 3, 32.0, 600
    t = rng.uniform(0.0, T, M)
    t[0], t[1] = 0.0, T
    case = dict(name="one_cell", N=N, T=T, dt_max=1.0, grid_x=np.array([0.0, T]), times=t, nodes=rng.integers(1, N + 1, M).astype(np.int64))
    return _finish(case, rng, all_base=1, none_base=2)


def narrow():
    """Two cells of width 2⁻²⁰·T between cells of about T/2; 40 events inside the narrow cells, on a dyadic lattice of 2⁻²⁶·T
    (so they are exact and some lie on the narrow cells' grid points)."""
    rng = np.random.default_rng(13)
    N, T, M = 3, 64.0, 800
    w = T * 2.0 ** -20
    gx = np.array([0.0, T / 2, T / 2 + w, T / 2 + 2 * w, T])
    t = rng.uniform(0.0, T, M)
    t[:40] = T / 2 + rng.integers(0, 129, 40) * (w / 64)
    case = dict(name="narrow", N=N, T=T, dt_max=1.0, grid_x=gx, times=t, nodes=rng.integers(1, N + 1, M).astype(np.int64))
    case = _finish(case, rng, all_base=1, none_base=2)
    case["counts"]["in_narrow"] = int(((case["times"] >= gx[1]) & (case["times"] < gx[3])).sum())
    return case


def wide_grid(G):
    """N = 3, M = 2000 on a non-uniform grid of G points (G = 4095 is the first that needs more than 64 KiB of LDS for the
    grid, the curve and the block sum's slots)."""
    rng = np.random.default_rng(14 + G)
    N, T, M = 3, 512.0, 2000
    gx = np.concatenate([[0.0], np.sort(rng.choice(np.arange(1, 1 << 16), G - 2, replace=False)) * (T / (1 << 16)), [T]])
    t = rng.uniform(0.0, T, M)
    t[:20] = gx[rng.integers(0, G, 20)]                                  # events on grid points, the last one included
    t[20] = T
    case = dict(name="wide_grid(%d)" % G, N=N, T=T, dt_max=1.0, grid_x=gx, times=t, nodes=rng.integers(1, N + 1, M).astype(np.int64))
    return _finish(case, rng, all_base=1, none_base=2)


def crowded():
    """N = 1 with 50 000 baseline events: 196 passes of the block-stride loop.  With one node the two attributions of the
    other cases cannot both hold: `parentnodes` is all zero and `parentnodes_none` sends every event to node 1."""
    rng = np.random.default_rng(15)
    T, M = 4096.0, 50000
    gx = np.array([0.0, 1.0, 300.0, 1024.5, 4000.0, T])
    case = dict(name="crowded", N=1, T=T, dt_max=2.0 ** -6, grid_x=gx, times=rng.uniform(0.0, T, M), nodes=np.ones(M, dtype=np.int64))
    case = _finish(case, rng, all_base=1, none_base=None)
    case["parentnodes_none"] = np.ones(M, dtype=np.int64)
    return case


def far_origin():
    rng = np.random.default_rng(16)
    N, T, M = 3, 1e6, 1500
    gx = np.array([0.0, 1.0, 1000.0, 1000.5, 250000.0, 5e5, 999000.0, 999999.0, T])
    t = rng.uniform(0.0, T, M)
    t[:4] = (0.0, 1000.5, 999999.0, T)
    case = dict(name="far_origin", N=N, T=T, dt_max=1.0, grid_x=gx, times=t, nodes=rng.integers(1, N + 1, M).astype(np.int64))
    return _finish(case, rng, all_base=1, none_base=2)


CASES = {"knots": knots, "one_cell": one_cell, "narrow": narrow, "crowded": crowded, "far_origin": far_origin}
CASES.update({"wide_grid(%d)" % g: (lambda g=g: wide_grid(g)) for g in (4094, 4095, 4096)})


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, CandLL) of a named continuous case, computed once per session and shared by the host and the GPU tests."""
    case = CASES[name]()
    return case, cont_candidate_ll(case["times"], case["nodes"], case["parentnodes"], case["N"], case["grid_x"], case["lam"])


DISC_CASES = {   # name: (T, N, dt, grid)
    "dt1": (257, 3, 1.0, [0.0, 1.0, 1.5, 32.0, 100.0, 257.0]),
    "dt.5": (257, 3, 0.5, [0.0, 0.5, 1.0, 32.0, 100.25, 128.0, 257.0]),
    "dt.25": (700, 3, 0.25, [0.0, 0.25, 1.0, 33.75, 174.75, 700.0]),
    "G2": (257, 3, 1.0, [0.0, 257.0]),
    "T1": (1, 3, 1.0, [0.0, 1.0]),
    "T700": (700, 3, 1.0, [0.0, 1.0, 256.0, 257.0, 699.0, 700.0]),
    "N1": (257, 1, 0.5, [0.0, 3.0, 64.0, 128.0, 257.0]),
    "N70": (257, 70, 1.0, [0.0, 7.0, 8.0, 256.0, 257.0]),
    # a grid that starts at 1 (the latest the process intensity at the bins 1..T allows): the last bin time, x[0] + (T-1)·dt,
    # is x[G-1] itself and takes the last value
    "x0=1": (257, 3, 1.0, [1.0, 2.0, 33.0, 100.5, 257.0]),
}


@functools.lru_cache(maxsize=None)
def disc_case(name):
    """Counts [N, T] (Poisson with a rate that sweeps 0.05..28: counts from 0 to about 40), grid, current curve λ [G, N] and a
    candidate Y [G, N] (m = -1).  The grid reaches T, as the process intensity at the bins 1..T needs, whatever dt is; every
    grid holds points that are bin times t·dt."""
    T, N, dt, gx = DISC_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    rate = np.exp(np.linspace(np.log(0.05), np.log(28.0), T))[None, :] * rng.uniform(0.5, 1.0, (N, 1))
    data = rng.poisson(rate).astype(np.int64)
    if T == 1:                                           # the sweep's first rate would leave the single bin empty
        data[:, 0] = (0, 3, 17)[:N]
    gx = np.array(gx)
    G = len(gx)
    on = int(np.isin(bin_times(gx, T, dt), gx).sum())
    return dict(name=name, T=T, N=N, dt=dt, grid_x=gx, data=data, m=-1.0, lam=np.exp(rng.normal(-1.0, 0.5, (G, N))),
                Y=rng.normal(0.0, 0.4, (G, N)), bins_on_grid=on,
                bins_at_end=int((bin_times(gx, T, dt) >= gx[-1]).sum()))


# ------------------------------------------------------------------------------------------------- lock step against serial
def squared_exponential(x, sigma, eta):
    x = _f64(x)
    return sigma ** 2 * np.exp(-((x[:, None] - x[None, :]) / eta) ** 2 / 2)


LOCK_X = np.array([0.0, 0.5, 8.0, 8.25, 24.0, 40.0, 56.0, 63.5, 64.0])
LOCK_SEED_CONT, LOCK_SEED_DISC = 3, 1
"""Chosen on the CPU with this module alone; the docstrings of the two lock-step tests in tests/test_lgcp_edges_gpu.py give
their rounds and smallest decision margins."""


@functools.lru_cache(maxsize=None)
def lockstep_cont_case():
    """N = 6 (node 6 without events), G = 9 on a knots-like grid, T = 64, a squared-exponential Σ; per node about 300
    events, all baseline events, at rate 8 before T/2 and 1.5 after; events at 0, on the grid points 8 and 24, and at T."""
    rng = np.random.default_rng(21)
    N, T = 6, 64.0
    ev, nd = [], []
    for c in range(1, N):
        a = rng.uniform(0.0, T / 2, rng.poisson(8.0 * T / 2))
        b_ = rng.uniform(T / 2, T, rng.poisson(1.5 * T / 2))
        t = np.concatenate([a, b_])
        t[:4] = (0.0, 8.0, 24.0, T)
        ev.append(t)
        nd.append(np.full(len(t), c))
    t, nodes = np.concatenate(ev), np.concatenate(nd).astype(np.int64)
    o = np.argsort(t, kind="stable")
    Sigma = squared_exponential(LOCK_X, 1.0, 6.0)
    m = math.log(4.0)
    lam = np.exp(m + 0.5 * rng.standard_normal((N, len(LOCK_X))) @ np.linalg.cholesky(Sigma).T)
    return dict(N=N, T=T, dt_max=1.0, grid_x=LOCK_X.copy(), times=t[o], nodes=nodes[o], parentnodes=np.zeros(len(t), dtype=np.int64),
                Sigma=Sigma, m=m, lam=lam)


@functools.lru_cache(maxsize=None)
def lockstep_disc_case():
    """N = 6, T = 300, dt = 1, G = 7 with grid points on bin times and cells of width 1; rate 3 before T/2 and 0.5 after."""
    rng = np.random.default_rng(22)
    N, T = 6, 300
    gx = np.array([0.0, 1.0, 32.0, 33.0, 150.0, 299.0, 300.0])
    rate = np.where(np.arange(T) < T // 2, 3.0, 0.5)[None, :] * rng.uniform(0.6, 1.4, (N, 1))
    data = rng.poisson(rate).astype(np.int64)
    Sigma = squared_exponential(gx, 1.0, 60.0)
    m = 0.0
    lam = np.exp(m + 0.5 * np.linalg.cholesky(Sigma) @ rng.standard_normal((len(gx), N)))
    return dict(N=N, T=T, dt=1.0, grid_x=gx, data=data, Sigma=Sigma, m=m, lam=lam)


def serial_update(case, record, layout, max_attempts=100):
    """elliptical_slice_serial on a lock-step case with this module's candidate likelihood, node by node.  Returns the
    SliceNodes and the largest likelihood bound of any evaluation."""
    bounds = []
    if layout == "rows":
        t, nodes, pn = case["times"], case["nodes"], case["parentnodes"]
        per = [t[(nodes == c + 1) & (pn == 0)] for c in range(case["N"])]

        def loglik(c, y):
            r = cont_candidate_ll(per[c], np.ones(len(per[c]), dtype=np.int64), np.zeros(len(per[c]), dtype=np.int64), 1,
                                  case["grid_x"], np.exp(case["m"] + y)[None, :])
            bounds.append(r.bound[0])
            return r.ll[0]
        Y = np.log(case["lam"]) - case["m"]
    else:
        def loglik(c, y):
            r = disc_candidate_ll(case["data"][c][:, None], case["grid_x"], np.exp(case["m"] + y)[:, None], case["dt"])
            bounds.append(r.bound[0])
            return r.ll[0]
        Y = np.log(case["lam"]) - case["m"]
    res = elliptical_slice_serial(Y, np.linalg.cholesky(case["Sigma"]), record, loglik, layout=layout, max_attempts=max_attempts)
    return res, max(bounds)


def lockstep_conditions(res, bound):
    """What the chosen seeds must show: (smallest margin, margin > 1e3·bound, a node done in round 1, a node with >= 4
    rounds, both bracket ends moved)."""
    margin = min(r.margin for r in res)
    rounds = [r.rounds for r in res]
    return dict(margin=margin, bound=bound, clear=margin > 1e3 * bound, first=min(rounds) == 1, long=max(rounds) >= 4,
                both=sum(r.shrunk_min for r in res) > 0 and sum(r.shrunk_max for r in res) > 0, rounds=rounds)
