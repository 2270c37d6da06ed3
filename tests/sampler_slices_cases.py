"""The inputs of tests/test_sampler_slices_gpu.py, built once and shared with tests/test_sampler_slices_host.py, which proves on
the CPU that every one of them keeps its child slices (tests/slices_ref.py) and holds what its case is named for.

    A  the data of test_cont_sampler_gpu's slice-sampler test (N = 9, M = 7000, Δtmax = 1.2, ties, a burst of 60), with items of
       256 and of 4096 children
    B  walk_data(k) of test_slices_walk_gpu: items of k, k and 0 slices, k at the edges of 4 and 8 waves
    C  a ladder: runs of 24 events after gaps longer than Δtmax, so every window length 0..23 occurs M/24 times, under a model
       whose weights are nearly flat across a window and whose baseline is comparable to one of them (runs of 20 leave only
       the windows of 18 and 19 parents to draw weight 17 from: as few as 7 draws, under the 10 the census asks for)
    D  a burst of B events inside half a window: the longest window has B - 1 parents, B at the pairwise-sum threshold
    E  a time origin of 5e5, ties
    F  mostly empty windows"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from helpers import random_case

WALK_K = (1, 3, 4, 5, 7, 8, 9, 17)
BURSTS = (1023, 1024, 1025)
KINDS = ("exponential", "logitnormal")
VARIANTS = ((False, False), (True, True))                # (network, lgcp): standard, network with an LGCP baseline


@dataclass(frozen=True, eq=False)
class Input:
    name: str
    times: np.ndarray
    nodes: np.ndarray
    T: float
    N: int
    dt_max: float
    chunk: int
    seed: int                                            # of the model
    flat: bool = False

    @property
    def data(self):
        return self.times, self.nodes, self.T


def data_a():
    c = random_case(9, 7000, 350.0, "exponential", 1.2, seed=41)
    t = c["times"].copy()
    t[500:530:2] = t[501:531:2]
    t[3000:3060] = np.sort(np.random.default_rng(8).uniform(t[3000], t[3000] + 0.9, 60))
    return np.sort(t), c["nodes"], c["T"]


def data_ladder(runs=167, run=24, seed=5):
    """`runs` runs of `run` events spread over 0.9·Δtmax (Δtmax = 1), 1.15 apart: event j of a run has exactly j parents."""
    rng = np.random.default_rng(seed)
    step = 0.9 / (run - 1)
    t = np.concatenate([r * 2.05 + 0.3 + step * np.arange(run) + rng.uniform(-0.2, 0.2, run) * step for r in range(runs)])
    assert np.all(np.diff(t) > 0.0)
    nodes = rng.integers(1, 3, len(t)).astype(np.int64)
    return t, nodes, float(runs * 2.05 + 1.0)


def data_burst(B, seed=31):
    rng = np.random.default_rng(seed + B)
    bg = np.sort(rng.uniform(0.0, 500.0, 4000))
    burst = np.sort(rng.uniform(502.0, 502.5, B))
    tail = np.sort(rng.uniform(504.5, 504.5 + 125.0, 1000))
    t = np.concatenate([bg, burst, tail])
    nodes = rng.integers(1, 4, len(t)).astype(np.int64)
    return t, nodes, 630.0


def data_far_origin():
    c = random_case(6, 4000, 300.0, "logitnormal", 1.0, seed=1)
    t = np.sort(c["times"] + 5e5)
    t[100:160:3] = t[101:161:3]
    t = np.sort(t)
    return t, c["nodes"], float(t[-1] + 1.0)


def data_sparse(N, M, T, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, T, M))
    t[10:40:3] = t[11:41:3]
    t = np.sort(t)
    n = rng.integers(1, N + 1, M).astype(np.int64)
    if N > 2:
        n[n == 2] = 1                                    # node 2 has no events
    return t, n, float(T + 1.0)


@lru_cache(maxsize=None)
def inputs():
    from test_slices_walk_gpu import walk_data
    out = []
    t, n, T = data_a()
    for chunk in (256, 4096):
        out.append(Input(f"A-{chunk}", t, n, T, 9, 1.2, chunk, 41))
    for k in WALK_K:
        t, n, T = walk_data(k)
        out.append(Input(f"B-{k}", t, n, T, 3, 1.0, 4096, 21))
    t, n, T = data_ladder()
    out.append(Input("C", t, n, T, 2, 1.0, 4096, 3, flat=True))
    for B in BURSTS:
        t, n, T = data_burst(B)
        out.append(Input(f"D-{B}", t, n, T, 3, 1.0, 4096, 6))
    t, n, T = data_far_origin()
    out.append(Input("E", t, n, T, 6, 1.0, 4096, 1))
    # the two shapes of test_derived_layouts_agree_on_awkward_data, and each again with a window short enough that more than a
    # quarter of the children have no parent (a mean window of 2 leaves e^-2 = 14 % of them without one)
    for name, N, M, T, dtm in (("F-9", 9, 4000, 2.0, 1e-3), ("F-9-short", 9, 4000, 2.0, 4e-4), ("F-1", 1, 800, 90.0, 0.5),
                               ("F-1-short", 1, 800, 90.0, 0.08)):
        t, n, T1 = data_sparse(N, M, T, 123 + N)
        out.append(Input(name, t, n, T1, N, dtm, 4096, 50 + N))
    return {i.name: i for i in out}


MAIN = tuple(["A-256", "A-4096"] + [f"B-{k}" for k in WALK_K] + ["C", "E", "F-9", "F-9-short", "F-1", "F-1-short"])
BURST = tuple(f"D-{B}" for B in BURSTS)


def flat_parameters(inp, network, lgcp):
    """Case C: θ·Δt <= 0.5 and a wide logit-normal (μ = 0, τ = 0.5), so the weights of a window differ by less than a factor of
    two; a baseline of the size of one weight."""
    N = inp.N
    rng = np.random.default_rng(inp.seed)
    W = rng.uniform(0.9, 1.1, (N, N))
    A = np.array([[1.0, 1.0], [1.0, 0.0]]) if network else None
    if lgcp:
        gx = np.linspace(0.0, inp.T, 17)
        lam0 = np.exp(rng.normal(0.0, 0.3, (N, 17)))
    else:
        gx, lam0 = None, rng.uniform(0.8, 1.2, N)
    return dict(lam0=lam0, W=W, A=A, gx=gx, theta=rng.uniform(0.4, 0.6, (N, N)), mu=rng.normal(0.0, 0.1, (N, N)),
                tau=rng.uniform(0.45, 0.55, (N, N)))


def models(inp, kind, network, lgcp, nhp=None, orc=None):
    """(process, oracle model) of an input: random_case's model for its node count, seed and Δtmax; the flat one for case C."""
    if not inp.flat:
        c = random_case(inp.N, 8, inp.T, kind, inp.dt_max, network=network, lgcp=lgcp, seed=inp.seed, nhp=nhp, orc=orc)
        return c.get("proc"), c.get("om")
    p = flat_parameters(inp, network, lgcp)
    proc = om = None
    if orc is not None:
        if kind == "exponential":
            om = orc.ContModel(p["lam0"], p["W"], theta=p["theta"], dt_max=inp.dt_max, A=p["A"], grid_x=p["gx"])
        else:
            om = orc.ContModel(p["lam0"], p["W"], mu=p["mu"], tau=p["tau"], dt_max=inp.dt_max, A=p["A"], grid_x=p["gx"])
    if nhp is not None:
        baseline = nhp.LogGaussianCoxProcess(p["gx"], list(p["lam0"])) if lgcp else nhp.HomogeneousProcess(p["lam0"])
        if kind == "exponential":
            impulses = nhp.ExponentialImpulseResponse(p["theta"], 1.0, 1.0, inp.dt_max)
        else:
            impulses = nhp.LogitNormalImpulseResponse(p["mu"], p["tau"], inp.dt_max)
        weights = nhp.DenseWeightModel(p["W"])
        if network:
            proc = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, p["A"], nhp.BernoulliNetworkModel(0.5, inp.N))
        else:
            proc = nhp.ContinuousStandardHawkesProcess(baseline, impulses, weights)
    return proc, om


def uniforms(M, seed=17):
    """One uniform per event with 0 and the largest double below 1 planted at fixed strides."""
    u = np.random.default_rng(seed).uniform(size=M)
    u[::97] = 0.0
    u[5::89] = np.nextafter(1.0, 0.0)
    return u


def threshold_uniforms(orc, om, inp, window, seed=23):
    """Uniforms that sit ON the oracle's thresholds, found with the oracle alone.  The weight index a child draws is a step
    function of its own uniform, and the scan goes past weight k while cp_k <= u: so for a parent k of each child, drawn at
    random, the smallest double at which the oracle goes past k IS its cp_k = w_0/s + ... + w_k/s, to the bit -- bisected here
    over the doubles of [0, 1) for all children at once (62 oracle calls).  Returns (u_at, u_below, found): with u_at the
    oracle goes past k, with u_below (the double before) it stops at or before k, for the children marked `found` (the
    others keep a random uniform: no parent, or weights of 0 in front that even u = 0 goes past).  A kernel whose sum, weight
    or cumulated share differs from the oracle's in the last bit draws another index for one of the two."""
    M = len(inp.times)
    rng = np.random.default_rng(seed)
    idx = np.arange(M)
    k = np.floor(rng.uniform(size=M) * window).astype(np.int64)
    rand = rng.uniform(size=M)

    def past(bits):
        p, _ = orc.resample_parents(om, inp.times, inp.nodes, bits.view(np.float64), flags=orc.MATH_DET)
        return np.where(p > 0, idx - p, window) > k

    lo = np.zeros(M, dtype=np.int64)
    hi = np.full(M, np.array(np.nextafter(1.0, 0.0)).view(np.int64))
    found = (window > 0) & ~past(lo) & past(hi)
    while np.any(hi - lo > 1):
        mid = lo + (hi - lo) // 2
        g = past(mid)
        hi = np.where(g, mid, hi)
        lo = np.where(g, lo, mid)
    u_at = np.where(found, hi.view(np.float64), rand)
    u_below = np.where(found, lo.view(np.float64), rand)
    return u_at, u_below, found


_thresholds = {}


def thresholds(orc, inp, kind, network, lgcp, window):
    """threshold_uniforms of an input under one of its models, computed once and left unchanged."""
    key = (inp.name, kind, network, lgcp)
    if key not in _thresholds:
        _, om = models(inp, kind, network, lgcp, orc=orc)
        out = threshold_uniforms(orc, om, inp, window)
        for a in out:
            a.setflags(write=False)
        _thresholds[key] = out
    return _thresholds[key]


def check_planted_uniforms(inp, kind, network, window, u, p, pn):
    """What the planted uniforms mean.  u = 0 stops the scan at its first entry: the most recent parent, where the window is
    not empty and that parent's weight is positive (no mask, and not a logit-normal pdf at a delay of 0).  The largest double
    below 1 is past every parent's cumulated share: the baseline.  An empty window has only the baseline."""
    t, idx = inp.times, np.arange(len(inp.times))
    zero, top = u == 0.0, u == np.nextafter(1.0, 0.0)
    assert zero.sum() >= 1 and top.sum() >= 1
    assert np.all(p[top] == 0) and np.all(pn[top] == 0)
    empty = window == 0
    assert np.all(p[empty] == 0) and np.all(pn[empty] == 0)
    if not network:
        positive = ~empty & zero
        if kind == "logitnormal":
            positive &= np.concatenate([[False], t[1:] > t[:-1]])
        assert np.array_equal(p[positive], idx[positive])               # the 1-based index of event i - 1 is i
        assert np.array_equal(pn[positive], inp.nodes[idx[positive] - 1])
    return int(np.sum(zero & ~empty)), int(top.sum())
