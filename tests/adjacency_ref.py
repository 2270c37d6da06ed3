"""Extended-precision restatement of one Gibbs sweep of the adjacency matrix of a continuous network process, written from
the formulas of oracle/mp_eval.py (_pdf, _weight, _baseline) and the reference's conventions the oracle documents:

    pairs      event j is a parent of event k when j < k and t_k - Δtmax < t_j, the threshold t_k - Δtmax and the delay
               Δt = t_k - t_j both taken in float64, as the reference takes them; a tie t_j = t_k with j < k is a pair
    x_kp       Σ over the parents j of k on node p of W[p,c]·ħ(Δt),  ħ = θ·exp(-θ·Δt)  or the logit-normal density at
               Δt/Δtmax (not divided by Δtmax), zero outside (0, 1)
    l0_k       λ0_c(t_k) + Σ_{q != p} A[q,c]·x_kq         the intensity at child k without the entry being decided
    d[p,c]     -W[p,c]·cnt[p] + Σ_k [log(l0_k + x_kp) - log l0_k] + log ρ[p,c] - log(1 - ρ[p,c])
               (the first event's dropped term and the baseline integral cancel between ll1 and ll0; the integral term that
               is left is W[p,c]·cnt[p], cnt[p] the number of events on node p)
    decision   A[p,c] = 1 exactly when logit(u[p,c]) <= d[p,c]      (u <= exp(ll1 - logsumexp(ll0, ll1)))

The walk goes column by column and p ascending inside a column; l0_k is recomputed FROM SCRATCH for every entry from the
state the walk has reached, never updated incrementally.  Next to every d stands a rounding bound for a float64
implementation that does update λ incrementally,

    B[p,c] = 2⁻⁵³ · Σ_k [ (n_k + 2)·Λ_k / l0_k + |log l0_k| + |log(l0_k + x_kp)| + 4 ]

over the children k the list of p names.  n_k counts the list entries of the column that have gone into λ_k so far: those
of the parents whose link was present at the start (the terms of the starting sum), those of every parent decided before p,
and p's own; every one is at most one rounded addition into a number no larger than Λ_k, the largest value λ_k has held in
this sweep.  The 2 stand for removing the entry's own x from λ_k and adding it back, the two logarithms carry one rounding
each relative to their own size, and the 4 stand for the roundings of x_kp itself, which enters the term with a weight
x/(l0 + x) <= 1.  First order and worst case; derived, not measured.

Everything is evaluated in numpy's long double where that is the x87 80-bit format or wider (eps < 1e-18), otherwise in
mpmath numbers of 40 digits held in object arrays; real=np.float64 gives the plain double evaluation of the same
restatement.  Test code only."""
import collections
import functools

import numpy as np

LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)
MP_DIGITS = 40
EPS = 2.0 ** -53


class _Numpy:
    def __init__(self, real):
        self.real = real

    def arr(self, a):
        return np.asarray(a, dtype=self.real)

    def num(self, v):
        return self.real(v)

    def zeros(self, shape):
        return np.zeros(shape, dtype=self.real)

    def log(self, a):
        with np.errstate(divide="ignore"):
            return np.log(a)

    def exp(self, a):
        return np.exp(a)

    def sqrt(self, a):
        return np.sqrt(a)

    def pi(self):
        return self.real(4) * np.arctan(self.real(1))


class _Mpmath:
    def __init__(self):
        import mpmath
        mpmath.mp.dps = max(mpmath.mp.dps, MP_DIGITS)
        self.mp = mpmath
        self._mpf = np.frompyfunc(lambda v: mpmath.mpf(v), 1, 1)
        self._log = np.frompyfunc(lambda v: mpmath.log(v) if v != 0 else mpmath.mpf("-inf"), 1, 1)
        self._exp = np.frompyfunc(lambda v: mpmath.exp(v), 1, 1)
        self._sqrt = np.frompyfunc(lambda v: mpmath.sqrt(v), 1, 1)

    def arr(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        return self._mpf(a.astype(np.float64).astype(object))

    def num(self, v):
        return self.mp.mpf(float(v)) if not isinstance(v, self.mp.mpf) else v

    def zeros(self, shape):
        return self._mpf(np.zeros(shape).astype(object))

    def log(self, a):
        return self._log(a)

    def exp(self, a):
        return self._exp(a)

    def sqrt(self, a):
        return self._sqrt(a)

    def pi(self):
        return +self.mp.pi


def backend(real=None):
    """real = None: long double, or mpmath where long double is no wider than double; a numpy type: that type; "mpmath"."""
    if real is None:
        real = np.longdouble if LONGDOUBLE_OK else "mpmath"
    if isinstance(real, str):
        assert real == "mpmath"
        return _Mpmath()
    return _Numpy(real)


class Model:
    """The parameters of a continuous process, matrices indexed [parent, child]; the oracle's ContModel has the same fields."""

    def __init__(self, lambda0, W, theta=None, mu=None, tau=None, dt_max=1.0, grid_x=None):
        self.lambda0, self.W, self.theta, self.mu, self.tau = lambda0, W, theta, mu, tau
        self.dt_max, self.grid_x, self.N = float(dt_max), grid_x, W.shape[0]


# ---------------------------------------------------------------------------------------------------------------- data
def window_pairs(times, dt_max):
    """(k, j): every pair of event indices with j < k and times[j] > times[k] - dt_max (float64), k ascending."""
    t = np.asarray(times, dtype=np.float64)
    M = len(t)
    first = np.searchsorted(t, t - dt_max, side="right")                   # first j with t_j > t_k - Δtmax
    first = np.minimum(first, np.arange(M))
    cnt = np.arange(M) - first
    k = np.repeat(np.arange(M), cnt)
    j = np.arange(len(k)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(first, cnt)
    return k, j


def _columns(N, times, nodes, dt_max):
    """Per column c: the events of node c (its children, in time order) and its pairs as (child slot, parent node, Δt)."""
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    k, j = window_pairs(t, dt_max)
    slot_of = np.zeros(len(t), dtype=np.int64)
    cols = []
    order = np.argsort(n0[k], kind="stable")
    bounds = np.searchsorted(n0[k][order], np.arange(N + 1))
    for c in range(N):
        ev = np.nonzero(n0 == c)[0]
        slot_of[ev] = np.arange(len(ev))
        sel = order[bounds[c]:bounds[c + 1]]
        cols.append((ev, slot_of[k[sel]], n0[j[sel]], t[k[sel]] - t[j[sel]]))
    return cols


def _pair_x(b, model, q, c, dt):
    """W[q,c]·ħ(Δt) of pairs with parent nodes q (array), child node c, float64 delays dt."""
    w = b.arr(model.W[q, c])
    d = b.arr(dt)
    if model.theta is not None:
        th = b.arr(model.theta[q, c])
        return w * (th * b.exp(-(th * d)))
    out = b.zeros(len(dt))
    x64 = dt / model.dt_max
    ok = (x64 > 0.0) & (x64 < 1.0)
    if ok.any():
        x = d[ok] / b.num(model.dt_max)
        one = b.num(1.0)
        mu, tau = b.arr(model.mu[q[ok], c]), b.arr(model.tau[q[ok], c])
        z = (b.log(x / (one - x)) - mu) * b.sqrt(tau)
        out[ok] = w[ok] * (b.exp(-(z * z) / b.num(2.0)) * b.sqrt(tau / (b.num(2.0) * b.pi())) / (x * (one - x)))
    return out


def _baseline(b, model, c, t):
    """λ0_c at the float64 times t: constant, or the piecewise-linear interpolant through (grid_x, lambda0[c])."""
    if model.grid_x is None:
        return b.zeros(len(t)) + b.num(model.lambda0[c])
    gx = np.asarray(model.grid_x, dtype=np.float64)
    y = b.arr(np.asarray(model.lambda0)[c])
    G = len(gx)
    i = np.clip(np.searchsorted(gx, t, side="right") - 1, 0, G - 2)        # x[i] <= t < x[i+1]
    x0, x1, tt = b.arr(gx[i]), b.arr(gx[i + 1]), b.arr(t)
    out = (y[i + 1] * (tt - x0) + y[i] * (x1 - tt)) / (x1 - x0)
    last = ~(t < gx[G - 1])
    if last.any():
        out[last] = y[G - 1]
    return out


# --------------------------------------------------------------------------------------------------------------- sweep
def _logit(b, u):
    """logit of the stored double u in the evaluation's type; -inf at 0."""
    uu = b.num(float(u))
    if float(u) <= 0.0:
        return -np.inf
    return b.log(uu / (b.num(1.0) - uu))


def _walk(model, times, nodes, T, rho, A0, choose, real):
    """The walk shared by sweep and adversarial_uniforms.  choose(p, c, d, delta, B) returns the logit that decides the
    entry.  Returns A, d, B and the data term Δ = Σ_k [...] of every entry."""
    b = backend(real)
    N = model.N
    A0 = np.asarray(A0, dtype=np.float64)
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (N, N))
    cnt = np.bincount(np.asarray(nodes, dtype=np.int64) - 1, minlength=N)
    t64 = np.asarray(times, dtype=np.float64)
    A = A0.copy()
    d_out, B_out, delta_out = b.zeros((N, N)), np.zeros((N, N)), b.zeros((N, N))
    for c, (ev, slot, q, dt) in enumerate(_columns(N, t64, nodes, model.dt_max)):
        nch = len(ev)
        lam0 = _baseline(b, model, c, t64[ev])
        X = b.zeros((nch, N))
        C = np.zeros((nch, N), dtype=np.int64)
        if len(slot):
            np.add.at(X, (slot, q), _pair_x(b, model, q, c, dt))
            np.add.at(C, (slot, q), 1)
        a = b.arr(A0[:, c].copy())
        lam = lam0 + (X @ a if nch else b.zeros(0))
        Lmax = lam.copy()
        n = (C * (A0[:, c] != 0)[None, :]).sum(axis=1)
        prior = b.log(b.arr(rho[:, c])) - b.log(b.num(1.0) - b.arr(rho[:, c]))
        bias = -(b.arr(model.W[:, c]) * b.arr(cnt.astype(np.float64))) + prior
        for p in range(N):
            rows = np.nonzero(C[:, p])[0]
            delta, Bpc = b.num(0.0), 0.0
            if len(rows):
                x = X[rows, p]
                a[p] = b.num(0.0)
                l0 = lam0[rows] + X[rows] @ a
                lg0, lg1 = b.log(l0), b.log(l0 + x)
                delta = (lg1 - lg0).sum()
                n[rows] += C[rows, p]
                terms = b.arr((n[rows] + 2).astype(np.float64)) * Lmax[rows] / l0 + abs(lg0) + abs(lg1) + b.num(4.0)
                Bpc = EPS * float(terms.sum())
            dd = bias[p] + delta
            ell = choose(b, p, c, dd, delta, Bpc)
            anew = 1.0 if ell <= dd else 0.0
            A[p, c] = anew
            a[p] = b.num(anew)
            if len(rows):
                Lmax[rows] = np.maximum(Lmax[rows], l0 + x if anew else l0)
            d_out[p, c], B_out[p, c], delta_out[p, c] = dd, Bpc, delta
    return A, d_out, B_out, delta_out


def sweep(model, times, nodes, T, rho, u, A0, real=None, parts=False):
    """One sweep from A0 with the uniforms u [parent, child] and link probabilities rho (scalar or matrix).  Returns the new A,
    the log-odds d of every entry at the state the walk had reached, and the bound B; with parts, the data term Δ as well."""
    u = np.asarray(u, dtype=np.float64)
    out = _walk(model, times, nodes, T, rho, A0, lambda b, p, c, d, delta, B: _logit(b, u[p, c]), real)
    return out if parts else out[:3]


OFFSETS = ((1e-9, False), (1e-6, False), (3e-4, True), (1.1e-3, True), (2e-3, True), (0.1, False))
"""(magnitude, scaled by 1 + Δ) of the adversarial offsets, each taken with both signs: class 2·i is +, 2·i + 1 is -."""

Adversarial = collections.namedtuple("Adversarial", "u A margins fallbacks cls d B delta")


def adversarial_uniforms(model, times, nodes, T, rho, A0, offsets, rng, real=None):
    """Walks like sweep; at each entry draws an offset δ from `offsets`, stores u = sigmoid(d + δ) rounded to double, takes
    ℓ' = logit(u) back from the STORED u and decides with it.  The draw is kept when |d + δ| <= 30, ℓ' - d has δ's sign,
    |ℓ' - d| >= |δ|/2 and |ℓ' - d| >= 64·B; otherwise the entry gets a plain random u (class -1) and is counted."""
    N = model.N
    u = np.zeros((N, N))
    margins, cls = np.zeros((N, N)), np.zeros((N, N), dtype=np.int64)

    def choose(b, p, c, d, delta, B):
        i = int(rng.integers(2 * len(offsets)))
        mag, scaled = offsets[i // 2]
        dl = (b.num(mag) * (b.num(1.0) + delta) if scaled else b.num(mag)) * (-1 if i & 1 else 1)
        target = d + dl
        keep = False
        if abs(float(target)) <= 30.0:
            uu = float(b.num(1.0) / (b.num(1.0) + b.exp(-target)))
            if 0.0 < uu < 1.0:
                ell = _logit(b, uu)
                m = float(ell - d)
                keep = (m > 0) == (float(dl) > 0) and m != 0 and abs(m) >= abs(float(dl)) / 2 and abs(m) >= 64 * B
        if not keep:
            i, uu = -1, float(rng.uniform())
            ell = _logit(b, uu)
            m = float(ell - d)
        u[p, c], margins[p, c], cls[p, c] = uu, m, i
        return ell

    A, d, B, delta = _walk(model, times, nodes, T, rho, A0, choose, real)
    return Adversarial(u, A, margins, int((cls < 0).sum()), cls, d, B, delta)


# -------------------------------------------------------------------------------------------------------------- census
Census = collections.namedtuple("Census", "lengths repeats codes steps cuts")


def census(N, times, nodes, dt_max):
    """What the grouping rules in the header comment of the build kernel make of the data, in integers:

    lengths [p, c]  entries of the list of parent node p in column c
    repeats [p, c]  the list names a child more than once
    codes   [p, c]  255: p is decided alone by the general step (more than 16 entries); g = 1..4: p heads a group of g
                    consecutive parents, each list at most 16 entries, no child named by two lists of the group, no group
                    across a multiple of 64; 0: member of the group before it
    steps   [c]     steps of the column (groups + general steps)
    cuts            groups that end below four parents only because the next parent starts a 64-chunk"""
    lengths = np.zeros((N, N), dtype=np.int64)
    repeats = np.zeros((N, N), dtype=bool)
    codes = np.zeros((N, N), dtype=np.int64)
    steps = np.zeros(N, dtype=np.int64)
    cuts = 0
    for c, (ev, slot, q, dt) in enumerate(_columns(N, times, nodes, dt_max)):
        kids = [set() for _ in range(N)]
        for s, p in zip(slot.tolist(), q.tolist()):
            lengths[p, c] += 1
            if s in kids[p]:
                repeats[p, c] = True
            kids[p].add(s)
        p = 0
        while p < N:
            steps[c] += 1
            if lengths[p, c] > 16:
                codes[p, c] = 255
                p += 1
                continue
            seen = set(kids[p])
            g = 1
            while g < 4 and p + g < N:
                nxt = p + g
                fits = lengths[nxt, c] <= 16 and not (kids[nxt] & seen)
                if nxt % 64 == 0:
                    cuts += bool(fits)
                    break
                if not fits:
                    break
                seen |= kids[nxt]
                g += 1
            codes[p, c] = g
            p += g
    return Census(lengths, repeats, codes, steps, cuts)


def census_summary(cs):
    """The counts the tests assert on."""
    L, heads = cs.lengths, cs.codes[(cs.codes >= 1) & (cs.codes <= 4)]
    short = (L >= 2) & (L <= 16)
    return {"short": int(short.sum()), "mid": int(((L > 16) & (L <= 64)).sum()), "long": int((L > 64).sum()),
            "folded": int((short & cs.repeats).sum()), "groups": [int((heads == g).sum()) for g in (1, 2, 3, 4)],
            "general": int((cs.codes == 255).sum()), "cuts": int(cs.cuts),
            "residues": sorted(set((cs.steps % 3).tolist())), "empty_columns": np.nonzero(L.sum(axis=0) == 0)[0].tolist(),
            "max_list": int(L.max())}


# --------------------------------------------------------------------------------------------------------------- cases
def adjacency_case(N, M, T, dt_max=1.0, hot=0.0, bursts=0, empty=(), seed=0, kind="exponential", lgcp=False,
                   lam0_scale=1.0, w_scale=1.0):
    """Input builder.  Times uniform and sorted; nodes uniform over the non-empty nodes; a share `hot` of the events moved to
    one node; `bursts` triples of consecutive events put on one node at t, t, t + 1e-3·Δtmax (a tie and a near-tie, hence
    lists that name a child twice); the 1-based nodes in `empty` get no event.  Parameters drawn like helpers.random_case
    (λ0 and W times the given scales).  Returns a dict: times, nodes, T, data, N, dt_max, kind, lam0, grid_x, W, theta, mu,
    tau, A0, hot_node."""
    rng = np.random.default_rng(seed)
    times = np.sort(rng.uniform(0.0, T, M))
    live = np.array([n for n in range(1, N + 1) if n not in set(empty)], dtype=np.int64)
    nodes = live[rng.integers(0, len(live), M)]
    hot_node = int(live[len(live) // 3])
    if hot > 0:
        nodes[rng.uniform(size=M) < hot] = hot_node
    if bursts:
        at = np.sort(rng.choice((M - 3) // 4, bursts, replace=False)) * 4       # disjoint triples
        for i in at:
            times[i + 1] = times[i]
            times[i + 2] = times[i] + 1e-3 * dt_max
            nodes[i + 1] = nodes[i + 2] = nodes[i]
        order = np.argsort(times, kind="stable")
        times, nodes = times[order], nodes[order]
    W = rng.uniform(0.0, 1.0, (N, N)) / max(N, 2) * 2.0 * w_scale
    A0 = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
    if lgcp:
        gx = np.linspace(0.0, T, 17)
        lam0 = np.exp(rng.normal(0.0, 0.5, (N, 17))) * lam0_scale
    else:
        gx = None
        lam0 = rng.uniform(0.5, 1.5, N) * lam0_scale
    theta = rng.uniform(1.0, 5.0, (N, N)) / dt_max
    mu = rng.normal(0.0, 1.0, (N, N))
    tau = rng.uniform(0.5, 2.0, (N, N))
    return {"times": times, "nodes": nodes, "T": float(T), "data": (times, nodes, float(T)), "N": N, "dt_max": float(dt_max),
            "kind": kind, "lam0": lam0, "grid_x": gx, "W": W, "theta": theta, "mu": mu, "tau": tau, "A0": A0,
            "hot_node": hot_node}


def second_parameters(case, seed=1):
    """Another W and other impulse parameters for the same data (and the same baseline)."""
    rng = np.random.default_rng(seed)
    c = dict(case)
    c["W"] = case["W"] * rng.uniform(0.5, 1.5, case["W"].shape)
    c["theta"] = case["theta"] * rng.uniform(0.7, 1.3, case["theta"].shape)
    c["mu"] = case["mu"] + rng.normal(0.0, 0.3, case["mu"].shape)
    c["tau"] = case["tau"] * rng.uniform(0.7, 1.3, case["tau"].shape)
    return c


def model_of(case):
    expo = case["kind"] == "exponential"
    return Model(case["lam0"], case["W"], theta=case["theta"] if expo else None, mu=None if expo else case["mu"],
                 tau=None if expo else case["tau"], dt_max=case["dt_max"], grid_x=case["grid_x"])


def oracle_model(orc, case, A):
    expo = case["kind"] == "exponential"
    return orc.ContModel(case["lam0"], case["W"], theta=case["theta"] if expo else None, mu=None if expo else case["mu"],
                         tau=None if expo else case["tau"], dt_max=case["dt_max"], A=A, grid_x=case["grid_x"])


def process_of(nhp, case, A, rho):
    """The package's network process for a case's arrays (copies: the package may write to its own)."""
    if case["grid_x"] is not None:
        baseline = nhp.LogGaussianCoxProcess(case["grid_x"].copy(), [row.copy() for row in case["lam0"]])
    else:
        baseline = nhp.HomogeneousProcess(case["lam0"].copy())
    if case["kind"] == "exponential":
        impulses = nhp.ExponentialImpulseResponse(case["theta"].copy(), 1.0, 1.0, case["dt_max"])
    else:
        impulses = nhp.LogitNormalImpulseResponse(case["mu"].copy(), case["tau"].copy(), case["dt_max"])
    return nhp.ContinuousNetworkHawkesProcess(baseline, impulses, nhp.DenseWeightModel(case["W"].copy()), A.copy(),
                                              nhp.BernoulliNetworkModel(rho, case["N"]))


RHO = 0.35

SHAPES = {
    # name: builder arguments; see the table in tests/test_adjacency_edges_gpu.py
    "A-exp": dict(N=130, M=4000, T=500.0, hot=0.25, bursts=40, empty=(1, 77, 130), seed=11, kind="exponential"),
    "A-logit": dict(N=130, M=4000, T=500.0, hot=0.25, bursts=40, empty=(1, 77, 130), seed=11, kind="logitnormal"),
    "A-lgcp": dict(N=130, M=4000, T=500.0, hot=0.25, bursts=40, empty=(1, 77, 130), seed=11, kind="exponential", lgcp=True),
    "B-64": dict(N=64, M=1500, T=300.0, bursts=10, seed=12, kind="logitnormal"),
    "B-65": dict(N=65, M=1500, T=300.0, bursts=10, empty=(65,), seed=12, kind="exponential"),
    "C": dict(N=1, M=300, T=100.0, seed=57, kind="exponential"),
    "D": dict(N=5, M=6000, T=1500.0, hot=0.6, seed=146, kind="exponential", w_scale=0.06),
    "E": dict(N=130, M=4000, T=500.0, hot=0.25, bursts=40, empty=(1, 77, 130), seed=11, kind="exponential",
              lam0_scale=1e-4, w_scale=13.0),
}

Stage = collections.namedtuple("Stage", "name case A_start u A cls margins d B delta")


@functools.lru_cache(maxsize=None)
def prepared(name):
    """The four sweeps every case is run through, computed once per session and shared by the host and the GPU tests:
    random u from A0; adversarial u from A0; adversarial u from the matrix that sweep left; adversarial u with other W and
    impulse parameters on the same data, from the matrix the third left.  Returns (case, census, [Stage])."""
    case = adjacency_case(**SHAPES[name])
    cs = census(case["N"], case["times"], case["nodes"], case["dt_max"])
    rng = np.random.default_rng(1000 + SHAPES[name]["seed"])
    m, data, N = model_of(case), case["data"], case["N"]
    u1 = rng.uniform(size=(N, N))
    A1, d1, B1, D1 = sweep(m, *data, RHO, u1, case["A0"], parts=True)
    stages = [Stage("random", case, case["A0"], u1, A1, None, None, d1, B1, D1)]
    start = case["A0"]
    for label, cc in (("adversarial", case), ("second", case), ("parameters", second_parameters(case))):
        r = adversarial_uniforms(model_of(cc), *data, RHO, start, OFFSETS, rng)
        stages.append(Stage(label, cc, start, r.u, r.A, r.cls, r.margins, r.d, r.B, r.delta))
        start = r.A
    return case, cs, stages


@functools.lru_cache(maxsize=None)
def prepared_rho_matrix():
    """Case F: link probabilities as a MATRIX with entries exactly 0 and 1 mixed in, uniforms with exactly 0 and 1 - 2⁻⁵³ mixed
    in, every combination of the two present and more than one of them per column.  Returns (case, rho, u, A, d)."""
    case = adjacency_case(N=9, M=800, T=200.0, seed=15, kind="logitnormal")
    rng = np.random.default_rng(1015)
    N = case["N"]
    rho, u = rng.uniform(0.1, 0.9, (N, N)), rng.uniform(size=(N, N))
    top = 1.0 - 2.0 ** -53
    for (p, c), (r, v) in {(0, 0): (0.0, 0.0), (1, 0): (0.0, None), (5, 0): (None, top), (2, 1): (1.0, top), (3, 1): (1.0, None),
                           (8, 1): (0.0, top), (4, 2): (None, 0.0), (5, 2): (None, top), (6, 3): (1.0, 0.0), (7, 3): (0.0, top),
                           (0, 8): (0.0, 0.0), (8, 8): (1.0, top), (3, 5): (None, 0.0), (4, 5): (0.0, None)}.items():
        if r is not None:
            rho[p, c] = r
        if v is not None:
            u[p, c] = v
    A, d, B = sweep(model_of(case), *case["data"], rho, u, case["A0"])
    return case, rho, u, A, d
