"""The recursive route's truncated window, restated on the host from the comment at the top of the truncated-window section of
csrc/cont_recursive.hip and DESIGN.md 3.2 -- not from rec_cut_for or k_rec_windows:

    The recursion adds, for child i on node c, every earlier event j with t_j > 0 with weight a·W·θ·e^{-θ(t_i - t_j)}.  Events
    more than `cut` before the child are at most `count` "events at distance cut", each below max(W·θ)·e^{-θmin·cut}; with

        count = min(M, min_q slab_max[q] / (1 - e^{-θmin·L_q}))          slab_max[q] = most events in any closed window of length L_q
        mass  = count · max(W·θ)
        cut   = (ln(mass / λmin) + 60 ln 2) / θmin

    all of them together stay below 2⁻⁶⁰·λmin <= 2⁻⁶⁰·λ_i.  The extremes run over EVERY entry of the tables, whatever A and W
    say about it; λmin over the grid intensities for a grid baseline.  cut = 1e-300 when mass = 0 (no excitation: the empty
    window is exact) or the quotient is not positive; cut = 0 (no bound: the recursion runs) when θmin <= 0, λmin <= 0 or
    anything is not finite.  The empty window is exact for λ_i, not for its derivatives -- ∂/∂W[p,c] = -cnt[p] + Σ g_i·a·θ·e^{-θΔ}
    keeps its pair sums at W = 0 -- so the gradient and the information take the recursion at cut = 1e-300.

slab_stats, cut, window_starts (first j in [n_zero, i] with times[j] > fl(t_i - cut), clamped as the kernel clamps it),
dropped_tail (what the window leaves out, per child, in long double) and route (the cost model's verdict from the constants in
nhp_recursive_window; used to CHOOSE inputs with margin, never as an expected value).  The full-history log-likelihood and
gradient come from cont_grad_ref.evaluate(..., recursive=True), whose bound has the `tail` term.

The cases of tests/test_rec_window_host.py (census, tail, route margin; no GPU) and tests/test_rec_window_gpu.py are built
here, once per session.  Test code only."""
import functools
import math

import numpy as np

import cont_grad_ref as cr
from adjacency_ref import backend

TAIL = 2.0 ** -60
COSTS = (1.0, 1.2, 1e9)                   # log-likelihood, gradient, observed information
THREADS = 64 * 256                        # k_rec_stats: 64 blocks of 256; entries from here on are the loop's second trip


# ------------------------------------------------------------------------------------------------------------ the bound
def slab_stats(times):
    """(lengths, most events in any closed window of that length): lengths double from span/M while below the span."""
    t = np.asarray(times, dtype=np.float64)
    M = len(t)
    if M <= 1 or not t[-1] > t[0]:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    span = t[-1] - t[0]
    lens = []
    L = span / M
    while L < span:
        lens.append(L)
        L *= 2.0
    idx = np.arange(M)
    best = []
    for L in lens:
        lo = np.searchsorted(t, t - L, side="left")                   # a first guess; the window is decided on fl(t_i - t_j) <= L
        for _ in range(4):
            down = (lo > 0) & (t - t[np.maximum(lo - 1, 0)] <= L)
            up = t - t[lo] > L
            if not (down.any() or up.any()):
                break
            lo = lo - down + up
        assert not ((lo > 0) & (t - t[np.maximum(lo - 1, 0)] <= L)).any() and not (t - t[lo] > L).any()
        best.append(int((idx - lo + 1).max()))
    return np.array(lens), np.array(best, dtype=np.int64)


def slab_stats_brute(times):
    """The same by an O(M²) count."""
    t = np.asarray(times, dtype=np.float64)
    lens, _ = slab_stats(t)
    D = t[:, None] - t[None, :]
    earlier = np.arange(len(t))[None, :] <= np.arange(len(t))[:, None]
    return lens, np.array([int(((D <= L) & earlier).sum(axis=1).max()) for L in lens], dtype=np.int64)


def extremes(m):
    """(θmin, max W·θ, λmin) over every entry; NaN wins."""
    return float(np.min(m.theta)), float(np.max(m.W * m.theta)), float(np.min(m.lam0))


def cut(m, times, count_only_M=False):
    tmin, wmax, lmin = extremes(m)
    if not (np.isfinite(tmin) and np.isfinite(wmax) and np.isfinite(lmin)) or tmin <= 0.0 or lmin <= 0.0 or wmax < 0.0:
        return 0.0
    M = len(times)
    count = float(max(M, 1))
    if not count_only_M:
        for L, mx in zip(*slab_stats(times)):
            geo = 1.0 - math.exp(-tmin * L)
            if geo > 0.0:
                count = min(count, float(mx) / geo)
    mass = count * wmax
    if mass == 0.0 or not mass / lmin > 0.0:
        return 1e-300
    c = (math.log(mass / lmin) + 60.0 * math.log(2.0)) / tmin
    return c if c > 0.0 else 1e-300


def window_starts(times, cut_, n_zero):
    """Per event i (time order): the first j in [n_zero, i] with times[j] > fl(t_i - cut); i itself for i < n_zero."""
    t = np.asarray(times, dtype=np.float64)
    i = np.arange(len(t))
    lo = np.searchsorted(t, t - cut_, side="right")
    return np.minimum(np.maximum(lo, n_zero), i)


def _column_terms(b, m, n0, c):
    A = np.ones((m.N, m.N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    return b.arr(A[n0, c] * m.W[n0, c]) * b.arr(m.theta[n0, c]), b.arr(m.theta[n0, c])


def pair_sums(m, times, nodes, lo, hi, real=None):
    """Σ_{j in [lo_i, hi_i)} a·W·θ·e^{-θ(t_i - t_j)} per event i (time order), in long double (real=None)."""
    b = backend(real)
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    out = b.zeros(len(t))
    tt = b.arr(t)
    for c in range(m.N):
        coef, th = _column_terms(b, m, n0, c)
        for i in np.nonzero(n0 == c)[0]:
            a, z = int(lo[i]), int(hi[i])
            if z > a:
                out[i] = (coef[a:z] * b.exp(-th[a:z] * (tt[i] - tt[a:z]))).sum()
    return out


def node_floor(m):
    """λ0_c, the least baseline intensity of node c (its smallest grid intensity for a grid baseline)."""
    return m.lam0 if m.grid_x is None else m.lam0.min(axis=1)


def dropped_tail(m, times, nodes, starts):
    """(what the window starting at starts[i] leaves out of λ_i: Σ_{t_j > 0, j < start}, long double [M]; 2⁻⁶⁰·λ0_c [M])."""
    t = np.asarray(times, dtype=np.float64)
    n_zero = int((t <= 0.0).sum())
    lo = np.minimum(np.full(len(t), n_zero), np.arange(len(t)))
    tail = pair_sums(m, t, nodes, lo, np.maximum(starts, lo))
    return tail, TAIL * node_floor(m)[np.asarray(nodes, dtype=np.int64) - 1]


def loglik_with_starts(m, times, nodes, T, starts):
    """The recursive form's log-likelihood with every λ_i summed from starts[i] on (homogeneous baseline): with the full
    history's starts it is the reference, with a stale cut's it is what a stale cache would return."""
    assert m.grid_x is None
    b = backend()
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    lam = b.arr(m.lam0[n0]) + pair_sums(m, t, nodes, starts, np.arange(len(t)))
    cnt = np.bincount(n0, minlength=m.N).astype(np.float64)
    return float(b.log(lam).sum() - b.arr(m.lam0).sum() * b.num(T) - (b.arr(cnt)[:, None] * b.arr(m.W)).sum())


def full_starts(times):
    t = np.asarray(times, dtype=np.float64)
    return np.minimum(int((t <= 0.0).sum()), np.arange(len(t)))


def route(case, cut_, cost=1.0, mean_window=None):
    """nhp_recursive_window's decision from its constants: dict(used, t_window, t_recursion, margin) with margin =
    t_recursion / t_window (inf / 0 where the bound, not the cost, decides)."""
    t, M, N = case["times"], len(case["times"]), case["N"]
    if M == 0 or not cut_ > 0.0 or (cut_ == 1e-300 and cost != 1.0):    # the empty window serves the log-likelihood alone
        return dict(used=False, t_window=math.inf, t_recursion=0.0, margin=0.0)
    rate = M / t[-1] if t[-1] > 0.0 else 0.0
    kc = cut_ * rate
    if kc > 8192.0:
        return dict(used=False, t_window=math.inf, t_recursion=0.0, margin=0.0)
    biggest = max(1, int(np.bincount(np.asarray(case["nodes"]) - 1, minlength=N).max()))
    t_rec = cost * ((N + 1023) // 1024) * biggest * (0.6e-6 + 1.25e-9 * N)
    if mean_window is None:
        st = window_starts(t, cut_, int((t <= 0.0).sum()))
        mean_window = float((np.arange(M) - st).sum()) / M
    t_win = max(30e-6 + M * k / (9.5e11 if k >= 128.0 else 5.5e11) for k in (kc, mean_window))
    return dict(used=t_win < t_rec, t_window=t_win, t_recursion=t_rec, margin=t_rec / t_win)


# ---------------------------------------------------------------------------------------------------------------- cases
def _times(rng, M, T, zeros=3, ties=True):
    t = np.sort(rng.uniform(0.0, T, M))
    t[:zeros] = 0.0
    if ties and M > 240:
        t[200:220:2] = t[201:221:2]
    return np.sort(t)


def _nodes(rng, M, N, busy_node, busy):
    nodes = rng.integers(1, N + 1, M).astype(np.int64)
    nodes[rng.choice(M, busy, replace=False)] = busy_node
    return nodes


def _case(N, T, t, nodes, lam0, W, theta, A=None, grid_x=None):
    return dict(N=N, T=T, times=t, nodes=nodes, kind="exponential", dt_max=0.05, lam0=lam0, W=W, theta=theta, mu=None, tau=None,
                A=A, grid_x=grid_x, recursive=True)


def uniform_case(N, seed=0):
    """The base: uniform times, three events at t = 0, ten ties, θ in [20, 40]; a busy column so the window wins by a margin."""
    rng = np.random.default_rng(900 + N + seed)
    M, T = {1: 1500, 3: 2000, 64: 3000}[N], {1: 150.0, 3: 200.0, 64: 300.0}[N]
    t = _times(rng, M, T)
    nodes = _nodes(rng, M, N, min(N, 2), {1: M, 3: 1200, 64: 700}[N])
    return _case(N, T, t, nodes, rng.uniform(0.5, 1.5, N), rng.uniform(0.1, 1.0, (N, N)) / max(N, 2), rng.uniform(20.0, 40.0, (N, N)))


def spread_case():
    """θ over two orders of magnitude; every extreme of the bound sits on an entry that contributes nothing: min θ = 2 where
    W = 0 and A = 0, max W·θ = 400 at flat index N² - 1 under A = 0, min λ0 at the last node."""
    rng = np.random.default_rng(911)
    N, M, T = 3, 2000, 200.0
    t = _times(rng, M, T)
    nodes = _nodes(rng, M, N, 1, 1200)
    theta = np.exp(rng.uniform(np.log(5.0), np.log(300.0), (N, N)))
    W = rng.uniform(0.05, 0.3, (N, N))
    A = np.ones((N, N))
    theta[0, 1], W[0, 1], A[0, 1] = 2.0, 0.0, 0.0
    theta[2, 2], W[2, 2], A[2, 2] = 400.0, 1.0, 0.0
    lam0 = np.array([1.2, 0.9, 0.05])
    return _case(N, T, t, nodes, lam0, W, theta, A=A)


def second_trip_case():
    """N = 130: N² = 16 900 entries against k_rec_stats' 16 384 threads.  min θ = 5 at flat index 16 899, max W·θ = 20 at flat
    index 16 384; every other θ in [20, 40] and W·θ <= 0.31."""
    rng = np.random.default_rng(912)
    N, M, T = 130, 3000, 300.0
    t = _times(rng, M, T)
    nodes = _nodes(rng, M, N, 1, 2000)
    theta = rng.uniform(20.0, 40.0, (N, N))
    W = rng.uniform(0.0, 1.0, (N, N)) / N
    theta[N - 1, N - 1] = 5.0                                           # flat p + c·N = 16 899
    p, c = THREADS % N, THREADS // N                                    # flat 16 384
    theta[p, c], W[p, c] = 40.0, 0.5
    return _case(N, T, t, nodes, rng.uniform(0.5, 1.5, N), W, theta)


def grid_case():
    """N = 130 on a grid of G = 127 points: 16 510 grid intensities, the least at the last point of the last node (flat
    16 509); events on grid points and at t = T."""
    rng = np.random.default_rng(913)
    N, G, M, T = 130, 127, 3000, 300.0
    gx = np.linspace(0.0, T, G)
    t = _times(rng, M, T)
    for i, g in ((400, 10), (1500, 60), (2200, 100), (M - 1, G - 1)):
        t[i] = gx[g]
    order = np.argsort(t, kind="stable")
    nodes = _nodes(rng, M, N, 1, 2000)[order]
    lam0 = np.exp(rng.normal(0.0, 0.3, (N, G)))
    lam0[N - 1, G - 1] = 0.01
    return _case(N, T, t[order], nodes, lam0, rng.uniform(0.0, 1.0, (N, N)) / N, rng.uniform(20.0, 40.0, (N, N)), grid_x=gx)


BURST_AT = (0.5, 0.9, 0.999, 1.0, 1.001, 1.1, 2.0)


def burst_case(with_burst=True):
    """400 events inside 0.01 at t = 100, seven children at 100.005 + f·cut for f in BURST_AT and one event at exactly
    fl(t_i - cut) of the child at f = 1.1 (the window's edge is open: `>`): the cut depends on the data's crowding and the
    events' places on the cut, so the case is the fixed point of the reference's own cut (reached in two rounds).  Without the burst: the same M and span, the 400 events spread out (the two-dataset case)."""
    rng = np.random.default_rng(914)
    N, T = 3, 200.0
    base = np.sort(rng.uniform(0.0, T, 1900))[:1899]                     # (one more event is placed below)
    base[0], base[-1] = 0.25, 199.75
    extra = 100.0 + np.sort(rng.uniform(0.0, 0.01, 400)) if with_burst else np.sort(rng.uniform(1.0, 199.0, 400))
    lam0, W, theta = rng.uniform(0.5, 1.5, N), rng.uniform(0.1, 1.0, (N, N)) / 2.0, rng.uniform(20.0, 40.0, (N, N))
    node_pool = _nodes(rng, 2307, N, 1, 1400)
    m = cr.model(lam0, W, theta=theta)
    c, rounds = 1.0, 0
    while True:
        kids = 100.005 + np.array(BURST_AT) * c
        edge = kids[5] - c                                              # an event at exactly fl(t_i - cut) of the child at 1.1 cuts: not a parent
        t = np.sort(np.concatenate([base, extra, kids, [edge]]))
        new = cut(m, t)
        rounds += 1
        if new == c:
            break
        c = new
        assert rounds < 6
    case = _case(N, T, t, node_pool, lam0, W, theta)
    case["rounds"] = rounds
    return case


def net_case():
    """uniform N = 64 under a network: half of A zero, a zero row and a zero column; the integral is not masked (D7)."""
    case = uniform_case(64, seed=1)
    rng = np.random.default_rng(915)
    A = (rng.uniform(size=(64, 64)) < 0.5).astype(np.float64)
    A[7, :] = 0.0
    A[:, 1] = 0.0                                                       # the busy column: its λ is its baseline
    case["A"] = A
    return case


def early_case():
    """Five events at t = 0 (children with idx < n_zero on every node) and the first events right behind them."""
    rng = np.random.default_rng(916)
    N, M, T = 3, 1500, 150.0
    t = _times(rng, M, T, zeros=5)
    t[5:10] = (2.0 ** -40, 1e-6, 1e-3, 0.01, 0.011)
    t = np.sort(t)
    nodes = _nodes(rng, M, N, 3, 900)
    nodes[:12] = np.tile((1, 2, 3), 4)
    return _case(N, T, t, nodes, rng.uniform(0.5, 1.5, N), rng.uniform(0.1, 1.0, (N, N)) / 2.0, rng.uniform(20.0, 40.0, (N, N)))


def tiny_case(N, M):
    rng = np.random.default_rng(917 + 10 * N + M)
    t = np.array([0.3, 0.35][:M]) if M == 2 else np.array([0.7])
    nodes = np.array([1, N][:M], dtype=np.int64)
    return _case(N, 1.0, t, nodes, rng.uniform(0.5, 1.5, N), rng.uniform(0.1, 1.0, (N, N)), rng.uniform(20.0, 40.0, (N, N)))


def silent_case():
    """All W = 0: mass = 0, cut = 1e-300, every window empty; ll is the baseline's closed form."""
    case = uniform_case(3, seed=2)
    case["W"] = np.zeros((3, 3))
    return case


def no_bound_case(which):
    """λ0 = 0 on a node without events, or θ = 0 under W = 0: no bound, the recursion runs, the values stay finite."""
    case = uniform_case(3, seed=3)
    if which == "lam":
        case["nodes"][case["nodes"] == 3] = 1
        case["lam0"][2] = 0.0
    else:
        case["theta"][1, 0], case["W"][1, 0] = 0.0, 0.0
    return case


def nan_case():
    case = uniform_case(3, seed=4)
    case["theta"][2, 1] = np.nan
    return case


def slow_case():
    """θ near 0.01: the cut is thousands of time units, more than 8192 expected parents per window."""
    case = uniform_case(3, seed=5)
    case["theta"] = np.random.default_rng(918).uniform(0.008, 0.012, (3, 3))
    return case


def cache_case(which="fast"):
    """The staleness cases' data (N = 3, M = 1500, five events per unit time) with fast θ in [200, 400] (cut near 0.22) or
    the same θ / 100 (cut near 20)."""
    rng = np.random.default_rng(919)
    N, M, T = 3, 1500, 300.0
    t = _times(rng, M, T)
    nodes = _nodes(rng, M, N, 1, 900)
    theta = rng.uniform(200.0, 400.0, (N, N))
    case = _case(N, T, t, nodes, rng.uniform(0.5, 1.5, N), rng.uniform(0.2, 0.6, (N, N)), theta)
    if which == "slow":
        case["theta"] = theta / 100.0
    return case


CASES = {
    "uniform-1": lambda: uniform_case(1), "uniform-3": lambda: uniform_case(3), "uniform-64": lambda: uniform_case(64),
    "spread": spread_case, "second_trip": second_trip_case, "grid": grid_case, "burst": burst_case, "net": net_case,
    "early": early_case, "silent": silent_case,
    "tiny-1-1": lambda: tiny_case(1, 1), "tiny-1-2": lambda: tiny_case(1, 2), "tiny-3-1": lambda: tiny_case(3, 1),
    "tiny-3-2": lambda: tiny_case(3, 2),
    "no_bound-lam": lambda: no_bound_case("lam"), "no_bound-theta": lambda: no_bound_case("theta"), "nan": nan_case, "slow": slow_case,
    "cache-fast": lambda: cache_case("fast"), "cache-slow": lambda: cache_case("slow"), "no_burst": lambda: burst_case(False),
}
WINDOW = ["uniform-1", "uniform-3", "uniform-64", "spread", "second_trip", "grid", "burst", "net", "early", "silent",
          "cache-fast", "cache-slow", "no_burst"]
TINY = ["tiny-1-1", "tiny-1-2", "tiny-3-1", "tiny-3-2"]
RECURSION = ["no_bound-lam", "no_bound-theta", "slow"]
# the route at recursion_cost 1.0, 1.2 and 1e9: the window everywhere; for one or two events only where the cost is waived
EXPECT = {name: (1, 1, 1) for name in WINDOW}
EXPECT["silent"] = (1, 0, 0)              # ∂/∂W keeps its pair sums at W = 0: the empty window serves the log-likelihood alone
EXPECT.update({name: (0, 0, 1) for name in TINY})
EXPECT.update({name: (0, 0, 0) for name in RECURSION + ["nan"]})
MARGIN = 3.0


@functools.lru_cache(maxsize=None)
def case_of(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def prepared(name, columns=None):
    """(case, full-history Result) once per session; the arrays are shared, nobody writes to them."""
    case = case_of(name)
    return case, cr.evaluate(cr.model_of(case), case["times"], case["nodes"], case["T"], recursive=True, columns=columns)


@functools.lru_cache(maxsize=None)
def cut_of(name):
    case = case_of(name)
    return cut(cr.model_of(case), case["times"])
