"""numpy restatement of map_parents and cascades, written from their definitions (include/nhp.h: nhp_cont_map_parents,
nhp_cont_cascades), not from the kernels, and the generator of the parity cases.  Plain loops; test code only.

map_parents_ref: for event i the categories are the events i-1, i-2, ..., first (first = the first event with
t > t_i - Δtmax: the dataset's window rule) with weight W·A·ħ(t_i - t_j), then the baseline λ0_c(t_i); the mode is the
FIRST maximum in that order and prob = w_max / Σw with one math.fsum.

forest_ref: one forward pass gives root and generation (a parent precedes its child), one backward pass the descendants;
the cascade and node tables follow by bincount-style reductions."""
import collections
import functools
import math

import numpy as np

import compensator_ref as cr

MapRef = collections.namedtuple("MapRef", "parents parentnodes prob gap wmax total")
Forest = collections.namedtuple("Forest", "root generation descendants cascade_root cascade_size cascade_depth cascade_end "
                                          "immigrants offspring reach")
FOREST_INT_FIELDS = tuple(f for f in Forest._fields if f != "cascade_end")


def _baseline(model, c, t):
    if model.grid_x is None:
        return model.lam0[c]
    x, y = model.grid_x, model.lam0[c]
    if t >= x[-1]:
        return y[-1]
    g = int(np.searchsorted(x, t, side="right")) - 1
    return (y[g + 1] * (t - x[g]) + y[g] * (x[g + 1] - t)) / (x[g + 1] - x[g])


def _impulse(model, p, c, d):
    """ħ_{p,c}(d) as the likelihood evaluates it: exponential pdf; logit-normal pdf at d/Δtmax, not divided by Δtmax."""
    if model.theta is not None:
        th = model.theta[p, c]
        return th * np.exp(-th * d)
    x = d / model.dt_max
    ok = (x > 0.0) & (x < 1.0)
    xs = np.where(ok, x, 0.5)
    tau, mu = model.tau[p, c], model.mu[p, c]
    z = np.log(xs / (1.0 - xs)) - mu
    return np.where(ok, np.sqrt(tau / (2.0 * np.pi)) * np.exp(-0.5 * tau * z * z) / (xs * (1.0 - xs)), 0.0)


def category_weights(model, times, nodes0, i):
    """(weights, first): the categories of event i in the sampler's order -- parents i-1 .. first, then the baseline."""
    t, c = times[i], nodes0[i]
    first = min(int(np.searchsorted(times, t - model.dt_max, side="right")), i)
    j = np.arange(i - 1, first - 1, -1)
    p = nodes0[j]
    w = model.WA[p, c] * _impulse(model, p, c, t - times[j])
    return np.append(w, _baseline(model, c, t)), first


def map_parents_ref(model, times, nodes):
    """MapRef(parents, parentnodes, prob, gap, wmax, total); gap = (w1 - w2) / w1 of the two largest weights (1 when an
    event has one category only); the first event is (0, 0) with prob 1."""
    times, nodes = np.asarray(times, float), np.asarray(nodes, np.int64)
    nodes0, M = nodes - 1, len(times)
    par, pno = np.zeros(M, np.int64), np.zeros(M, np.int64)
    prob, gap, wmax, total = np.ones(M), np.ones(M), np.zeros(M), np.zeros(M)
    for i in range(M):
        w, _ = category_weights(model, times, nodes0, i)
        total[i] = math.fsum(w)
        if i == 0:
            wmax[i] = w[-1]
            continue
        k = int(np.argmax(w))                              # the first maximum
        if k < len(w) - 1:
            par[i] = i - k                                 # 1-based index of event i-1-k
            pno[i] = nodes[i - 1 - k]
        wmax[i] = w[k]
        prob[i] = w[k] / total[i]
        if len(w) > 1:
            rest = np.delete(w, k)
            gap[i] = (w[k] - rest.max()) / w[k]
    return MapRef(par, pno, prob, gap, wmax, total)


def forest_ref(parents, times, nodes, N):
    parents, times, nodes0 = np.asarray(parents, np.int64), np.asarray(times, float), np.asarray(nodes, np.int64) - 1
    M = len(parents)
    root, gen, desc = np.zeros(M, np.int64), np.zeros(M, np.int64), np.zeros(M, np.int64)
    for k in range(M):
        p = parents[k]
        if not (p == 0 or 1 <= p <= k):
            raise ValueError("parents[k] must be 0 or the index of an earlier event")
        if p == 0:
            root[k] = k + 1
        else:
            root[k], gen[k] = root[p - 1], gen[p - 1] + 1
    for k in range(M - 1, -1, -1):
        if parents[k]:
            desc[parents[k] - 1] += desc[k] + 1
    roots = np.flatnonzero(parents == 0)
    rank = np.zeros(M + 1, np.int64)
    rank[roots + 1] = np.arange(len(roots))
    depth, end = np.zeros(len(roots), np.int64), np.zeros(len(roots))
    np.maximum.at(depth, rank[root], gen)
    np.maximum.at(end, rank[root], times)
    imm = np.bincount(nodes0[roots], minlength=N).astype(np.int64)
    off = np.zeros(N, np.int64)
    np.add.at(off, nodes0, desc)
    reach = np.zeros((N, N), np.int64)
    if M:
        np.add.at(reach, (nodes0[root - 1], nodes0), 1)
    return Forest(root, gen, desc, roots + 1, desc[roots] + 1, depth, end, imm, off, reach)


def doubling_ref(parents):
    """(root, generation, descendants, rounds) by the pointer-doubling recurrence the kernels use: up_k[i] the ancestor at
    distance exactly 2^k (-1: none), c_k[j] the descendants of j, itself included, at distance < 2^k:
        c_{k+1}[j] = c_k[j] + Σ_{i: up_k[i] = j} c_k[i],   up_{k+1}[i] = up_k[up_k[i]]
    and the saturating form a <- a[a], d[i] += d[a[i]] for root and generation; rounds stop when no up-pointer is left."""
    parents = np.asarray(parents, np.int64)
    M = len(parents)
    idx = np.arange(M)
    up = parents - 1
    a, d, c = np.where(parents > 0, parents - 1, idx), (parents > 0).astype(np.int64), np.ones(M, np.int64)
    rounds = 0
    while np.any(up >= 0):
        has = up >= 0
        cn = c.copy()
        np.add.at(cn, up[has], c[has])
        nup = np.full(M, -1, np.int64)
        nup[has] = up[up[has]]
        a, d, c, up = a[a], d + d[a], cn, nup
        rounds += 1
    return a + 1, d, c - 1, rounds


# ---- the parity cases -------------------------------------------------------------------------------------------------
SHAPES = ((4, 450.0, 2.0), (7, 250.0, 0.5))
KINDS = ("exponential", "logitnormal")


def make_process(nhp, kind, N, dt_max, A=None, lgcp_T=None):
    """N nodes, default_rng(3): W = 0.7/N·U(0.5, 1.5), λ0 = 0.25·U(0.5, 1.5), θ = U(2, 6)/Δtmax (Δtmax = ∞: /1) or
    μ ~ N(-1, 0.5), τ ~ U(0.5, 2); lgcp_T: the baseline as a 9-point piecewise-linear grid on [0, lgcp_T] instead."""
    r = np.random.default_rng(3)
    W = 0.7 / N * r.uniform(0.5, 1.5, (N, N))
    lam0 = 0.25 * r.uniform(0.5, 1.5, N)
    if kind == "exponential":
        imp = nhp.ExponentialImpulseResponse(r.uniform(2.0, 6.0, (N, N)) / (dt_max if np.isfinite(dt_max) else 1.0), 1.0, 1.0, dt_max)
    else:
        imp = nhp.LogitNormalImpulseResponse(r.normal(-1.0, 0.5, (N, N)), r.uniform(0.5, 2.0, (N, N)), dt_max)
    if lgcp_T is None:
        base = nhp.HomogeneousProcess(lam0)
    else:
        base = nhp.LogGaussianCoxProcess(np.linspace(0.0, lgcp_T, 9), list(lam0[:, None] * r.uniform(0.5, 1.5, (N, 9))))
    if A is not None:
        return nhp.ContinuousNetworkHawkesProcess(base, imp, nhp.DenseWeightModel(W), A, nhp.BernoulliNetworkModel(0.5, N))
    return nhp.ContinuousStandardHawkesProcess(base, imp, nhp.DenseWeightModel(W))


_cache = {}


def case(nhp, kind, N, T, dt_max, **kw):
    """{"proc", "data", "times", "nodes", "T", "model" (compensator_ref.Model), "ref" (MapRef)}: data from the host
    simulator nhp.rand(proc, T, seed=1) (of the standard process, so a mask or an LGCP grid changes the model, not the
    data); made once per process and shared."""
    key = (kind, N, T, dt_max, tuple(sorted((k, None if v is None else np.asarray(v).tobytes()) for k, v in kw.items())))
    if key not in _cache:
        times, nodes, _ = nhp.rand(make_process(nhp, kind, N, dt_max), T, seed=1)
        proc = make_process(nhp, kind, N, dt_max, **kw)
        model = cr.Model.of(proc)
        _cache[key] = dict(proc=proc, data=(times, nodes, T), times=times, nodes=nodes, T=T, model=model,
                           ref=map_parents_ref(model, times, nodes))
    return _cache[key]


def generated_cases(nhp):
    """The four generated parity cases: both shapes, both impulse kinds."""
    return [((kind, N), case(nhp, kind, N, T, dt)) for kind in KINDS for N, T, dt in SHAPES]


def random_forest(M, seed=0, p_immigrant=0.3):
    """Each event an immigrant with probability p_immigrant, else the child of a uniform earlier event."""
    r = np.random.default_rng(seed)
    par = np.zeros(M, np.int64)
    if M < 2:
        return par
    k = np.arange(1, M)
    par[1:] = np.where(r.uniform(size=M - 1) < p_immigrant, 0, 1 + (r.uniform(size=M - 1) * k).astype(np.int64))
    return par


@functools.lru_cache(maxsize=None)
def forest_data(M, N, seed=7):
    """Sorted times and 1-based nodes for a forest test (the dataset a parent vector is laid over)."""
    r = np.random.default_rng(seed)
    return np.sort(r.uniform(0.0, max(M, 1) * 0.5, M)), r.integers(1, N + 1, M).astype(np.int64)
