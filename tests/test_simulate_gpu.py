"""rand(process, duration; device=True): the GPU generator nhp_cont_simulate (csrc/cont_simulate.hip).

Contract of the output, determinism, an exact numpy restatement of the documented counter scheme (include/nhp.h), the
laws of the generative model (counts, child nodes, delays, LGCP positions, stationary rates, agreement with the host
simulator), the explosion path and the metric size end to end.  Tolerances come from the counts: 5σ for Poisson counts,
Kolmogorov-Smirnov and χ² at p > 1e-4."""
import math
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS_CRIT = 2.23            # sqrt(n)·D above this: Kolmogorov p < 1e-4


def _ks_uniform(u):
    u = np.sort(np.asarray(u, float))
    n = len(u)
    i = np.arange(1, n + 1)
    return max(np.max(i / n - u), np.max(u - (i - 1) / n)) * math.sqrt(n)


def _ks_two(a, b):
    a, b = np.sort(a), np.sort(b)
    x = np.concatenate([a, b])
    d = np.max(np.abs(np.searchsorted(a, x, side="right") / len(a) - np.searchsorted(b, x, side="right") / len(b)))
    return d * math.sqrt(len(a) * len(b) / (len(a) + len(b)))


def _chi2_ok(obs, exp):
    """χ² goodness of fit, Wilson-Hilferty normal approximation, p > 1e-4."""
    k = len(obs) - 1
    if k < 1:
        return True
    x = float(np.sum((obs - exp) ** 2 / exp))
    z = ((x / k) ** (1 / 3) - (1 - 2 / (9 * k))) / math.sqrt(2 / (9 * k))
    return z < 3.72


def make(nhp, lam0, W, kind="exponential", theta=None, mu=None, tau=None, A=None, dt_max=1.0):
    base = nhp.HomogeneousProcess(np.asarray(lam0, float))
    if kind == "exponential":
        imp = nhp.ExponentialImpulseResponse(np.asarray(theta, float), 1.0, 1.0, dt_max)
    else:
        imp = nhp.LogitNormalImpulseResponse(np.asarray(mu, float), np.asarray(tau, float), dt_max)
    w = nhp.DenseWeightModel(np.asarray(W, float))
    if A is None:
        return nhp.ContinuousStandardHawkesProcess(base, imp, w)
    return nhp.ContinuousNetworkHawkesProcess(base, imp, w, np.asarray(A, float), nhp.BernoulliNetworkModel(0.5, len(lam0)))


def small(nhp, N=5, kind="exponential", network=False, seed=0, scale=0.15, dt_max=1.0):
    rng = np.random.default_rng(seed)
    A = (rng.uniform(size=(N, N)) < 0.6).astype(float) if network else None
    return make(nhp, rng.uniform(0.5, 1.5, N), rng.uniform(0.0, scale, (N, N)), kind, theta=rng.uniform(1.0, 3.0, (N, N)),
                mu=rng.normal(0.0, 1.0, (N, N)), tau=rng.uniform(0.5, 2.0, (N, N)), A=A, dt_max=dt_max)


def host(sample):
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in sample)


def same(a, b):
    return len(a) == len(b) and all((x == y) if isinstance(x, float) else (x.shape == y.shape and bool((x == y).all()))
                                    for x, y in zip(a, b))


# ---- contract ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,network", [("exponential", False), ("logit-normal", True)])
def test_output_contract(nhp, kind, network):
    import torch
    ctx = nhp.default_context()
    proc = small(nhp, kind=kind, network=network)
    t, n, T, par = nhp.rand(proc, 300.0, seed=3, device=True, return_parents=True)
    assert T == 300.0
    for x, dt in ((t, torch.float64), (n, torch.int64), (par, torch.int64)):
        assert x.dtype == dt and x.device.type == "cuda" and x.device.index == ctx.device and x.dim() == 1
    tt, nn, pp = host((t, n, par))
    assert len(tt) == len(nn) == len(pp) > 500
    assert np.all(np.diff(tt) >= 0) and tt[0] >= 0.0 and tt[-1] <= T
    assert nn.min() >= 1 and nn.max() <= proc.ndims()
    i = np.arange(len(tt))
    assert np.all(pp >= 0) and np.all(pp < i + 1)
    kid = pp > 0
    assert kid.any() and (~kid).any()
    assert np.all(tt[pp[kid] - 1] <= tt[kid])


def test_empty_results(nhp):
    proc = small(nhp)
    t, n, T = nhp.rand(proc, 0.0, seed=1, device=True)
    assert len(t) == len(n) == 0 and T == 0.0
    quiet = make(nhp, np.zeros(5), proc.weights.W, theta=proc.impulses.θ)
    t, n, T, par = nhp.rand(quiet, 100.0, seed=1, device=True, return_parents=True)
    assert len(t) == len(n) == len(par) == 0


# ---- determinism ------------------------------------------------------------------------------------------------------

def test_same_seed_same_bits_other_seed_other_sample(nhp):
    import ctypes as C
    from nhp_amd import _lib
    ctx = nhp.default_context()
    proc = small(nhp, N=6, network=True, seed=4)
    a = host(nhp.rand(proc, 400.0, seed=7, device=True, return_parents=True))
    b = host(nhp.rand(proc, 400.0, seed=7, device=True, return_parents=True))
    assert same(a, b)
    c = host(nhp.rand(proc, 400.0, seed=8, device=True, return_parents=True))
    assert not same(a, c)
    big = host(nhp.rand(proc, 400.0, seed=7, device=True, return_parents=True, max_events=4 * len(a[0])))
    assert same(a, big)
    # host output buffers through the C ABI: the same sample
    m = proc.device_model(ctx)
    cap = len(a[0]) + 3
    ht, hn, hp = np.full(cap, -1.0), np.full(cap, -1, np.int64), np.full(cap, -1, np.int64)
    k = C.c_int64()
    rc = _lib.lib().nhp_cont_simulate(ctx.h, m.h, 400.0, 7, cap, 0, ht.ctypes.data, hn.ctypes.data, hp.ctypes.data, C.byref(k))
    assert rc == 0 and k.value == len(a[0])
    assert np.array_equal(ht[:k.value], a[0]) and np.array_equal(hn[:k.value], a[1]) and np.array_equal(hp[:k.value], a[3])
    assert ht[k.value] == -1.0 and hn[k.value] == -1            # nothing written past the events


def test_the_device_resident_tables_are_what_is_read(nhp):
    ctx = nhp.default_context()
    p = small(nhp, N=4, seed=1)
    q = small(nhp, N=4, seed=2)                                 # same kinds, other values
    m = p.device_model(ctx)
    m.set_params(q.params())
    got = host(m.simulate(300.0, seed=5, return_parents=True))
    want = host(nhp.rand(q, 300.0, seed=5, device=True, return_parents=True))
    assert same(got, want)
    assert not same(got, host(nhp.rand(p, 300.0, seed=5, device=True, return_parents=True)))


# ---- exact restatement of the counter scheme (include/nhp.h) -----------------------------------------------------------

K_IMM_COUNT, K_IMM_POS = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9
K_CHILD_COUNT, K_CHILD = 0x94D049BB133111EB, 0xD6E8FEB86659FD93
M32 = 0xFFFFFFFF
U53 = 2.0 ** -53


def philox(key, step, e, attempt):
    c0, c1, c2, c3 = e & M32, ((e >> 32) ^ (attempt << 8)) & M32, step & M32, (step >> 32) & M32
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u2(key, step, e, attempt):
    w = philox(key, step, e, attempt)
    return ((((w[0] << 32) | w[1]) >> 11) + 1) * U53, ((((w[2] << 32) | w[3]) >> 11) + 1) * U53


def normal(key, step, e):
    w = philox(key, step, e, 1)
    ua = ((((w[0] << 32) | w[1]) >> 11) + 1) * U53
    return math.sqrt(-2.0 * math.log(ua)) * math.cos(2.0 * math.pi * w[2] / 2.0 ** 32)


def loggam(x):
    if x == 1.0 or x == 2.0:
        return 0.0
    n = int(7.0 - x) if x < 7.0 else 0
    x0 = x + n
    x2 = (1.0 / x0) * (1.0 / x0)
    c = (8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04,
         -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e+00)
    g = c[9]
    for k in range(8, -1, -1):
        g = g * x2 + c[k]
    gl = g / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * math.log(x0) - x0
    for _ in range(n):
        gl -= math.log(x0 - 1.0)
        x0 -= 1.0
    return gl


def poisson(mean, key, step, e, branches=None):
    if not mean > 0.0:
        return 0
    if mean < 10.0:
        if branches is not None:
            branches.add("inversion")
        ua, _ = u2(key, step, e, 0)
        u = ua - U53
        p = math.exp(-mean)
        F, k = p, 0.0
        while u >= F and k < 100.0:
            k += 1.0
            p = p * mean / k
            F = F + p
        return int(k)
    if branches is not None:
        branches.add("ptrs")
    slam, loglam = math.sqrt(mean), math.log(mean)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha, vr = 1.1239 + 1.1328 / (b - 3.4), 0.9277 - 3.6224 / (b - 2.0)
    lia = math.log(invalpha)
    for att in range(4096):
        ua, V = u2(key, step, e, att)
        U = (ua - U53) - 0.5
        us = 0.5 - abs(U)
        if us == 0.0:
            continue
        k = float(math.floor((2.0 * a / us + b) * U + mean + 0.43))
        if us >= 0.07 and V <= vr:
            return int(k)
        if k < 0.0 or (us < 0.013 and V > us):
            continue
        if math.log(V) + lia - math.log(a / (us * us) + b) <= -mean + k * loglam - loggam(k + 1.0):
            return int(k)
    raise AssertionError("PTRS did not accept")


def restate(proc, T, seed, branches=None):
    lam0 = np.asarray(proc.baseline.λ, float)
    N = len(lam0)
    A = getattr(proc, "adjacency_matrix", None)
    V = proc.weights.W * A if A is not None else np.array(proc.weights.W, float)
    G = np.cumsum(V, axis=1)                          # sequential row prefix, the device's order of additions
    R = G[:, -1]
    imp = proc.impulses
    expo = hasattr(imp, "θ")
    at, an, ap = [], [], []
    for c in range(N):
        for _ in range(poisson(lam0[c] * T, seed ^ K_IMM_COUNT, 0, c, branches)):
            ua, _ = u2(seed ^ K_IMM_POS, 0, len(at), 0)
            at.append((ua - U53) * T); an.append(c); ap.append(-1)
    g0, g1, gen = 0, len(at), 0
    kids = [poisson(R[an[i]], seed ^ K_CHILD_COUNT, 0, i, branches) for i in range(g0, g1)]
    while sum(kids):
        s = 0
        for i, k in zip(range(g0, g1), kids):
            p = an[i]
            for _ in range(k):
                ua, ub = u2(seed ^ K_CHILD, gen, s, 0)
                x = (ua - U53) * R[p]
                c = int(np.searchsorted(G[p], x, side="right"))
                if c == N:
                    c = int(np.searchsorted(G[p], x, side="left"))
                if expo:
                    dt = -math.log(ub) / imp.θ[p, c]
                else:
                    z = normal(seed ^ K_CHILD, gen, s)
                    dt = imp.Δtmax / (1.0 + math.exp(-(imp.μ[p, c] + z / math.sqrt(imp.τ[p, c]))))
                t = at[i] + dt
                if t <= T:
                    at.append(t); an.append(c); ap.append(i)
                s += 1
        g0, g1, gen = g1, len(at), gen + 1
        kids = [poisson(R[an[i]], seed ^ K_CHILD_COUNT, gen, i, branches) for i in range(g0, g1)]
    order = np.argsort(np.array(at), kind="stable")
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    parents = np.array([0 if ap[i] < 0 else inv[ap[i]] + 1 for i in order], np.int64)
    return np.array(at)[order], np.array(an, np.int64)[order] + 1, parents


@pytest.mark.parametrize("kind,network", [("exponential", True), ("logit-normal", True), ("exponential", False)])
def test_numpy_restatement_reproduces_the_sample(nhp, kind, network):
    W = np.array([[0.20, 0.30, 0.10], [0.25, 0.15, 0.20], [0.10, 0.30, 0.20]])
    A = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]]) if network else None
    proc = make(nhp, [1.0, 0.8, 1.2], W, kind, theta=[[1.0, 2.0, 3.0], [1.5, 2.5, 1.2], [2.2, 1.1, 1.7]],
                mu=[[0.3, -0.5, 1.0], [-1.0, 0.0, 0.5], [0.7, -0.2, -0.8]], tau=[[1.0, 0.5, 2.0], [1.5, 0.8, 1.2], [0.6, 1.9, 1.0]],
                A=A, dt_max=1.5)
    T, seed = 50.0, 20261016
    branches = set()
    wt, wn, wp = restate(proc, T, seed, branches)
    assert branches == {"inversion", "ptrs"} and len(wt) > 100
    t, n, _, par = host(nhp.rand(proc, T, seed=seed, device=True, return_parents=True))
    assert len(t) == len(wt)
    assert np.array_equal(n, wn) and np.array_equal(par, wp)
    assert np.allclose(t, wt, rtol=1e-12, atol=0.0)


# ---- laws ---------------------------------------------------------------------------------------------------------------

def test_immigrants_without_excitation(nhp):
    N, T = 8, 500.0
    lam0 = np.random.default_rng(1).uniform(0.5, 2.0, N)
    proc = make(nhp, lam0, np.zeros((N, N)), theta=np.ones((N, N)))
    t, n, _, par = host(nhp.rand(proc, T, seed=11, device=True, return_parents=True))
    assert np.all(par == 0)
    cnt = np.bincount(n - 1, minlength=N)
    assert np.all(np.abs(cnt - lam0 * T) < 5 * np.sqrt(lam0 * T)), (cnt, lam0 * T)
    assert _ks_uniform(t / T) < KS_CRIT


def _cascade(nhp, kind, seed=21):
    N, T = 4, 3000.0
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.05, 0.3, (N, N))
    A = np.ones((N, N))
    A[0, 1] = A[2, 3] = A[3, 0] = 0.0
    W[1, 2] = 0.0                                       # a zero weight on a linked pair
    proc = make(nhp, rng.uniform(0.5, 1.0, N), W, kind, theta=rng.uniform(1.0, 3.0, (N, N)), mu=rng.normal(0.0, 1.0, (N, N)),
                tau=rng.uniform(0.5, 2.0, (N, N)), A=A, dt_max=0.5)
    t, n, _, par = host(nhp.rand(proc, T, seed=seed, device=True, return_parents=True))
    return proc, T, t, n - 1, par


@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_children_nodes_and_delays(nhp, kind):
    proc, T, t, node, par = _cascade(nhp, kind)
    N = proc.ndims()
    V = proc.weights.W * proc.adjacency_matrix
    R = V.sum(axis=1)
    q = -math.log(1e-12) / proc.impulses.θ.min() if kind == "exponential" else proc.impulses.Δtmax
    kid = np.flatnonzero(par > 0)
    pe = par[kid] - 1                                   # parent event of each child
    # children per event (events far enough from T to have all of theirs)
    nkids = np.bincount(pe, minlength=len(t))
    early = t < T - q
    for p in range(N):
        sel = early & (node == p)
        mean = R[p] * sel.sum()
        assert abs(nkids[sel].sum() - mean) < 5 * math.sqrt(mean), (p, nkids[sel].sum(), mean)
    # child node given parent node: W[p,:]·A[p,:] / R_p, exactly nothing on a zero link
    pn, cn = node[pe], node[kid]
    for p in range(N):
        obs = np.bincount(cn[pn == p], minlength=N).astype(float)
        assert np.all(obs[V[p] == 0] == 0)
        live = V[p] > 0
        assert _chi2_ok(obs[live], obs.sum() * V[p, live] / R[p]), (p, obs, V[p])
    # delays, through their own CDFs (children of early parents: not censored by T)
    ok = t[pe] < T - q
    dt = (t[kid] - t[pe])[ok]
    p_, c_ = pn[ok], cn[ok]
    if kind == "exponential":
        assert dt.max() > proc.impulses.Δtmax            # Δtmax does not cut exponential delays
        u = 1.0 - np.exp(-proc.impulses.θ[p_, c_] * dt)
    else:
        dmax = proc.impulses.Δtmax
        assert np.all(dt > 0.0) and np.all(dt < dmax)
        x = dt / dmax
        z = (np.log(x / (1.0 - x)) - proc.impulses.μ[p_, c_]) * np.sqrt(proc.impulses.τ[p_, c_])
        u = 0.5 * (1.0 + np.vectorize(math.erf)(z / math.sqrt(2.0)))
    assert len(u) > 2000
    assert _ks_uniform(u) < KS_CRIT


def test_lgcp_baseline(nhp):
    T = 200.0
    x = np.linspace(0.0, T, 11)
    lam = [np.array([0.5, 1.0, 2.0, 3.0, 2.5, 1.0, 0.0, 0.0, 1.5, 2.0, 1.0]), np.linspace(3.0, 0.2, 11)]
    base = nhp.LogGaussianCoxProcess(x, lam)
    proc = nhp.ContinuousStandardHawkesProcess(base, nhp.ExponentialImpulseResponse(np.ones((2, 2)), 1.0, 1.0, 1.0),
                                               nhp.DenseWeightModel(np.zeros((2, 2))))
    t, n, _ = host(nhp.rand(proc, T, seed=5, device=True))
    for c in range(2):
        y = lam[c]
        seg = 0.5 * (y[:-1] + y[1:]) * np.diff(x)
        I = seg.sum()
        tc = t[n == c + 1]
        assert abs(len(tc) - I) < 5 * math.sqrt(I), (c, len(tc), I)
        i = np.clip(np.searchsorted(x, tc, side="right") - 1, 0, len(x) - 2)
        f = (y[i + 1] * (tc - x[i]) + y[i] * (x[i + 1] - tc)) / (x[i + 1] - x[i])
        F = (np.concatenate([[0.0], np.cumsum(seg)])[i] + 0.5 * (tc - x[i]) * (y[i] + f)) / I
        assert _ks_uniform(F) < KS_CRIT
        if c == 0:
            assert not np.any((tc > x[6]) & (tc < x[7]))    # λ_1 = 0 there
    with pytest.raises(ValueError, match=re.escape("Sample duration does not match process duration.")):
        nhp.rand(proc, T + 1.0, seed=5, device=True)


def test_stationary_rates(nhp):
    W = np.array([[0.2, 0.1, 0.0], [0.0, 0.3, 0.2], [0.25, 0.0, 0.1]])
    A = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.0, 1.0]])
    lam0 = np.array([0.5, 1.0, 0.8])
    proc = make(nhp, lam0, W, theta=2 * np.ones((3, 3)), A=A)
    T = 40000.0
    t, n, _ = host(nhp.rand(proc, T, seed=9, device=True))
    rate = np.linalg.solve(np.eye(3) - (W * A).T, lam0)
    got = np.bincount(n - 1, minlength=3) / T
    assert np.all(np.abs(got - rate) / rate < 0.05), (got, rate)


def test_agrees_with_the_host_simulator(nhp):
    proc = small(nhp, N=4, kind="logit-normal", network=True, seed=6, scale=0.3)
    T = 300.0
    hs = [nhp.rand(proc, T, seed=s) for s in range(6)]
    ds = [host(nhp.rand(proc, T, seed=s, device=True)) for s in range(6)]
    ht, hn = np.concatenate([h[0] for h in hs]), np.concatenate([h[1] for h in hs])
    dt_, dn = np.concatenate([d[0] for d in ds]), np.concatenate([d[1] for d in ds])
    assert _ks_two(ht, dt_) < KS_CRIT
    rho = np.max(np.abs(np.linalg.eigvals(proc.weights.W * proc.adjacency_matrix)))
    for c in range(1, 5):
        a, b = (hn == c).sum(), (dn == c).sum()
        assert abs(a - b) < 5 * math.sqrt(a + b) / (1.0 - rho), (c, a, b)
    # within-cluster structure: gaps to the previous event on the same node
    def gaps(samples):
        out = []
        for t, n in samples:
            for c in range(1, 5):
                out.append(np.diff(t[n == c]))
        return np.concatenate(out)
    assert _ks_two(gaps([(h[0], h[1]) for h in hs]), gaps([(d[0], d[1]) for d in ds])) < KS_CRIT


# ---- explosion ----------------------------------------------------------------------------------------------------------

def test_explosion_is_an_error_and_the_context_stays_usable(nhp):
    hot = make(nhp, [1.0, 1.0, 1.0], 0.8 * np.ones((3, 3)), theta=np.ones((3, 3)))        # spectral radius 2.4
    with pytest.raises(RuntimeError, match="exploded"):
        nhp.rand(hot, 100.0, seed=1, device=True, max_events=20_000)
    with pytest.raises(RuntimeError, match="exploded"):                                  # the immigrants alone overflow
        nhp.rand(hot, 100.0, seed=1, device=True, max_events=100)
    proc = small(nhp, N=5, seed=3)
    t, n, T = nhp.rand(proc, 500.0, seed=2, device=True)
    assert len(t) > 1000
    ll_dev = nhp.loglikelihood(proc, (t, n, T), recursive=False)
    ll_host = nhp.loglikelihood(proc, (t.cpu().numpy(), n.cpu().numpy(), T), recursive=False)
    assert np.isfinite(ll_dev) and abs(ll_dev - ll_host) <= 1e-12 * abs(ll_host)


# ---- the metric size ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["exponential", "logit-normal"])
def test_metric_size_end_to_end(nhp, kind):
    N, T = 1024, 125_000.0
    proc = nhp.synthetic.s_metric_process(N, 1_000_000, T, kind)
    lam0 = np.asarray(proc.baseline.λ)
    expect = np.linalg.solve(np.eye(N) - proc.weights.W.T, lam0).sum() * T
    t, n, T_ = nhp.rand(proc, T, seed=1, device=True)
    assert 0.8e6 < len(t) < 1.2e6
    assert abs(len(t) - expect) < 0.02 * expect, (len(t), expect)
    ll_dev = nhp.loglikelihood(proc, (t, n, T_), recursive=False)
    ll_host = nhp.loglikelihood(proc, (t.cpu().numpy(), n.cpu().numpy(), T_), recursive=False)
    assert abs(ll_dev - ll_host) <= 1e-12 * abs(ll_host), (ll_dev, ll_host)
