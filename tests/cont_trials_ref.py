"""Several independent trials of a continuous Hawkes process (nhp_cont_dataset_create_trials), restated from the
definition:

    trial r = (events_r, nodes_r, T_r); stacked, it owns the events [f_r, f_{r+1}) and the clock interval [o_r, o_{r+1}],
    o_0 = 0, o_{r+1} = o_r + T_r, its events moved to o_r + t.  The event INDEX decides the trial of an event.
    window of event i of trial r: the j with f_r <= j < i and t_i - Δtmax < t_j       first[i] = max(f_r, first_plain[i])
    g_r: the first index in [f_r, f_{r+1}] whose stacked time is not exactly o_r     (the recursion's D9 per trial)
    every quantity = the sum over the trials of the quantity of the trial ALONE, on its own unshifted times

All inputs here have times and durations on the grid 2⁻¹⁰ (a multiple of 2⁻²⁰) with ΣT_r <= 2¹⁰, so the shift is exact, the
delays inside a trial keep their bits and "the trial alone" is a legitimate reference at the existing tolerances.  Values and
bounds come from the existing restatements, trial by trial -- cont_grad_ref.evaluate (log-likelihood and gradient, windowed
and recursive), compensator_exact_ref.evaluate -- and add:

    bound(sum) = Σ_r bound_r + 2⁻⁵³·(R + 1)·Σ_r |part_r|                          the final additions, in any order
    compensator: + 2⁻⁵³·((d(ws) + 1)·P_c(ws) + d(f_r)·P_c(f_r)) where the kernel subtracts two stacked prefixes, i.e. where f_r
    lies before the start of ws's chunk of 128 events; P_c(j) = Σ_{i<j} V[n_i, c] the stacked saturated mass before j, d(.) the
    prefix depth of compensator_exact_ref (csrc/cont_compensator.hip derives it: both prefixes are sums of non-negative terms,
    S_c(f_r) is the chunk-start prefix plus the chunk's events before f_r added from 0).  0 where no prefix is used.

Test code only."""
import functools

import numpy as np

import compensator_exact_ref as ce
import cont_grad_ref as gr
import information_ref as ir

EPS = 2.0 ** -53
GRID = 2.0 ** -10
REL_LL = 1e-11                                  # the suites' log-likelihood tolerance (test_cont_grad_edges_gpu.py)


# ------------------------------------------------------------------------------------------------------------ stacking
def stack(trials):
    """(times, nodes, f, o) of the stacked trials; plain numpy, independent of the package's stack_event_trials."""
    R = len(trials)
    f, o = np.zeros(R + 1, dtype=np.int64), np.zeros(R + 1)
    for r, (e, n, T) in enumerate(trials):
        f[r + 1], o[r + 1] = f[r] + len(e), o[r] + T
    t = np.concatenate([np.asarray(e, dtype=np.float64) + o[r] for r, (e, n, T) in enumerate(trials)] + [np.zeros(0)])
    nd = np.concatenate([np.asarray(n, dtype=np.int64) for e, n, T in trials] + [np.zeros(0, dtype=np.int64)])
    return t, nd, f, o


def trial_of(f, M):
    """The trial of every event index: the last r with f[r] <= i."""
    return np.searchsorted(f[1:], np.arange(M), side="right")


def window_starts(t, f, dt_max):
    """first[i] = max(f_r, first j with t_j > fl(t_i - Δtmax)), j <= i."""
    M = len(t)
    plain = np.minimum(np.searchsorted(t, t - dt_max, side="right"), np.arange(M))
    return np.maximum(plain, f[trial_of(f, M)]).astype(np.int64)


def first_positive(t, f, o):
    """g_r: the first index in [f_r, f_{r+1}] whose stacked time is not exactly o_r."""
    g = np.array(f[:-1], dtype=np.int64)
    for r in range(len(g)):
        while g[r] < f[r + 1] and t[g[r]] == o[r]:
            g[r] += 1
    return g


def recursive_starts(t, f, g, cut):
    """The recursive route's window starts: max(g_r, first j with t_j > fl(t_i - cut)), never above i.  cut = inf: g_r."""
    M = len(t)
    plain = np.searchsorted(t, t - cut, side="right") if np.isfinite(cut) else np.zeros(M, dtype=np.int64)
    return np.minimum(np.maximum(plain, g[trial_of(f, M)]), np.arange(M)).astype(np.int64)


def pair_offsets(first, nodes, N):
    """[N + 1] prefix over child nodes of the window lengths."""
    out = np.zeros(N + 1, dtype=np.int64)
    np.add.at(out, np.asarray(nodes, dtype=np.int64) + 1, np.arange(len(first)) - first)      # nodes 0-based
    return np.cumsum(out)


# --------------------------------------------------------------------------------------- log-likelihood and its gradient
def _sum_results(parts):
    keys = ("const", "S", "Q", "R", "U", "n", "tiny")
    out = {k: sum(getattr(p, k) for p in parts) for k in keys}
    grad = parts[0].grad
    for p in parts[1:]:
        grad = grad + p.grad
    ll = parts[0].ll
    for p in parts[1:]:
        ll = ll + p.ll
    return gr.Result(ll=ll, grad=grad, theta_col=np.max([p.theta_col for p in parts], axis=0), nb=parts[0].nb,
                     blocks=parts[0].blocks, **out)


def evaluate(m, trials, recursive=False, real=None):
    """(Result of the per-trial sum, tail): tail [P] = the allowance of the final additions, 2⁻⁵³·(R + 1)·Σ_r |grad_r|, to be
    passed to cont_grad_ref.check / bound as `tail` (added where the entry has pairs; an entry without any equals const)."""
    parts = [gr.evaluate(m, e, n, T, recursive=recursive, real=real) for e, n, T in trials]
    tail = EPS * (len(trials) + 1) * sum(np.abs(np.asarray(p.grad, dtype=np.float64)) for p in parts)
    return _sum_results(parts), tail


def window_tail(res, m, trials):
    """cont_grad_ref.window_tail of every trial, added (the truncated window drops less than 2⁻⁶⁰·λ_i per child)."""
    return sum(gr.window_tail(res, m, np.asarray(e, dtype=np.float64), n, T) for e, n, T in trials if len(e))


def naive_ll(m, trials, recursive=False):
    """The log-likelihood of the naive concatenation (one recording of length ΣT_r) in float64: what leaks across the seams."""
    t, nd, f, o = stack(trials)
    return float(gr.evaluate(m, t, nd, o[-1], recursive=recursive, real=np.float64).ll)


# ------------------------------------------------------------------------------------------------- observed information
def information(m, trials, recursive=False):
    """(information_ref.Result of the per-trial sum, tails): tails[k] [D, D] = the allowance of the final additions,
    2⁻⁵³·(R + 1)·Σ_r |block_r|, for information_ref.check / bound as `tail` (added where the entry has terms)."""
    parts = [ir.evaluate(m, np.asarray(e, dtype=np.float64), n, T, recursive=recursive) for e, n, T in trials]
    K = len(parts[0].columns)
    assert all(list(p.columns) == list(parts[0].columns) for p in parts)
    add = lambda xs: [sum(x[k] for x in xs[1:]) + xs[0][k] for k in range(K)]
    ll = parts[0].ll
    for p in parts[1:]:
        ll = ll + p.ll
    res = ir.Result(ll=ll, columns=parts[0].columns, kinds=parts[0].kinds, blocks=add([p.blocks for p in parts]),
                    **{f: add([getattr(p, f) for p in parts]) for f in ("S", "R", "U", "n", "tiny")})
    tails = [EPS * (len(trials) + 1) * sum(np.abs(np.asarray(p.blocks[k], dtype=np.float64)) for p in parts) for k in range(K)]
    return res, tails


def information_window_tail(res, k, m, trials):
    """information_ref.window_tail of every trial, added."""
    return sum(ir.window_tail(res, k, m, np.asarray(e, dtype=np.float64), n) for e, n, T in trials if len(e))


# ------------------------------------------------------------------------------------------------------------ compensator
def _prefix_depth(j):
    j = np.asarray(j, dtype=np.int64)
    c = j // ce.COMP_CHUNK
    return np.where(j > 0, np.minimum(j, ce.COMP_CHUNK) + np.minimum(c, ce.COMP_GROUP - 1) + c // ce.COMP_GROUP + 2, 0).astype(np.float64)


def saturated_masses(m):
    """V[p, c] = W·A·H(Δtmax) in float64 (0 without a finite Δtmax: nothing saturates)."""
    A = np.ones((m.N, m.N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    WA = A * m.W
    if not np.isfinite(m.dt_max):
        return np.zeros_like(WA)
    return WA * -np.expm1(-m.theta * m.dt_max) if m.theta is not None else WA * m.dt_max


def _extra(m, cumV, ws, fr, c):
    """2⁻⁵³·((d(ws) + 1)·P_c(ws) + d(f_r)·P_c(f_r)) where f_r lies before the start of ws's chunk, else 0 (ws, c arrays)."""
    used = np.isfinite(m.dt_max) & (fr < ws // ce.COMP_CHUNK * ce.COMP_CHUNK)
    return np.where(used, EPS * ((_prefix_depth(ws) + 1.0) * cumV[ws, c] + _prefix_depth(fr) * cumV[fr, c]), 0.0)


def compensator(m, trials, real=None):
    """compensator_exact_ref.Result of the per-trial compensators: at_events / residuals concatenated, total added; the
    bounds carry the allowances of the module docstring."""
    t, nd, f, o = stack(trials)
    M, N, R = len(t), m.N, len(trials)
    n0 = nd - 1
    cumV = np.zeros((M + 1, N))
    cumV[1:] = np.cumsum(saturated_masses(m)[n0, :], axis=0)
    parts = [ce.evaluate(m, np.asarray(e, dtype=np.float64), n, T, real=real) for e, n, T in trials]
    fields = {}
    for name in ("at_events", "residuals"):
        ps = [getattr(p, name) for p in parts if p.at_events is not None]
        fields[name] = {k: np.concatenate([getattr(q, k) for q in ps]) for k in ce.Part._fields}
    ws = np.concatenate([p.ws + f[r] for r, p in enumerate(parts)]).astype(np.int64)
    fr = f[trial_of(f, M)]
    ex = _extra(m, cumV, ws, fr, n0)
    prev = np.full(M, -1)
    for r in range(R):
        for c in range(N):
            ev = f[r] + np.nonzero(n0[f[r]:f[r + 1]] == c)[0]
            prev[ev[1:]] = ev[:-1]
    ex_res = ex + np.where(prev >= 0, ex[np.maximum(prev, 0)], 0.0)
    at = ce.Part(**{**fields["at_events"], "bound": np.where(fields["at_events"]["bound"] > 0, fields["at_events"]["bound"] + ex, 0.0)})
    res = ce.Part(**{**fields["residuals"], "bound": np.where(fields["residuals"]["bound"] > 0, fields["residuals"]["bound"] + ex_res, 0.0)})
    tot = {k: sum(getattr(p.total, k) for p in parts) for k in ("S", "R", "n", "bound")}
    value = parts[0].total.value
    for p in parts[1:]:
        value = value + p.total.value
    for r, p in enumerate(parts):                                    # the window start of Λ(T_r): the trial's first event inside (T - Δtmax, T]
        e, T = np.asarray(trials[r][0], dtype=np.float64), trials[r][2]
        jT = f[r] + int(np.searchsorted(e, T - m.dt_max, side="right"))
        tot["bound"] = tot["bound"] + _extra(m, cumV, np.full(N, jT), np.full(N, f[r]), np.arange(N))
    tot["bound"] = tot["bound"] + EPS * (R + 1) * sum(np.abs(np.asarray(p.total.value, dtype=np.float64)) for p in parts)
    total = ce.Part(value=value, d=np.max([p.total.d for p in parts], axis=0), **tot)
    return ce.Result(at, res, total, ws)


def naive_total(m, trials):
    t, nd, f, o = stack(trials)
    return np.asarray(ce.evaluate(m, t, nd, o[-1], real=np.float64, parts=("total",)).total.value, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_trials(counts, T, N, seed, near=0.25, tie_seams=False, zeros=0):
    """Trials with the given event counts on the grid 2⁻¹⁰ of [0, T].  Every trial of two or more events has one within `near`
    of its start and one within `near` of its end (events within Δtmax on both sides of every seam); tie_seams: the last event
    at exactly T_r and `zeros` + 1 events at exactly 0 (stacked: equal times in two trials)."""
    rng = np.random.default_rng(seed)
    out = []
    for r, n in enumerate(counts):
        k = np.sort(rng.integers(1, int(T / GRID), n))
        if n >= 2:
            k[0] = rng.integers(1, int(near / GRID))
            k[-1] = int(T / GRID) - rng.integers(1, int(near / GRID))
            k = np.sort(k)
        if tie_seams and n >= 3 + zeros:
            k[:1 + zeros] = 0
            k[-1] = int(T / GRID)
        nodes = rng.integers(1, N + 1, n).astype(np.int64)
        out.append((k * GRID, nodes, float(T)))
    return out


def _model(N, kind, dt_max, seed, network=False, theta_range=(1.0, 5.0)):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.05, 1.0, (N, N)) / N * 2.0
    scale = dt_max if np.isfinite(dt_max) else 1.0
    A = None
    if network:
        A = (rng.uniform(size=(N, N)) < 0.6).astype(np.float64)
        A[0, 0] = 1.0
    return dict(N=N, kind=kind, dt_max=dt_max, lam0=rng.uniform(0.5, 1.5, N), W=W,
                theta=rng.uniform(*theta_range, (N, N)) / scale, mu=rng.normal(0.0, 1.0, (N, N)), tau=rng.uniform(0.5, 2.0, (N, N)),
                A=A, grid_x=None)


LAYOUT_COUNTS = (0, 1, 1, 2, 63, 64, 65)


def case(name):
    """A named input: the model dict of cont_grad_ref's cases (process_of / model_of take it) + "trials"."""
    kind = "logitnormal" if name.endswith("-logit") else "exponential"
    base = name[:-6] if name.endswith("-logit") else name
    net = base.endswith("-net")
    base = base[:-4] if net else base
    if base == "counts":                 # the layout ladder: empty, single, pairs, one below / at / above a slice of 64
        c = _model(4, kind, 1.0, 11, net)
        c["trials"] = make_trials(LAYOUT_COUNTS, 8.0, 4, 1)
    elif base == "empty-ends":           # an empty first and an empty last trial (an empty one between the two would keep
        c = _model(3, kind, 1.0, 12, net)  # them Δtmax apart: nothing could leak, and the host test would reject the case)
        c["trials"] = make_trials((0, 40, 50, 0), 8.0, 3, 2)
    elif base == "ties":                 # an event at exactly T_r, then events at exactly 0: equal stacked times in two trials
        c = _model(4, kind, 1.0, 13, net)
        c["trials"] = make_trials((30, 30, 30), 8.0, 4, 3, tie_seams=True, zeros=1)
    elif base == "wide":                 # Δtmax larger than every trial
        c = _model(3, kind, 64.0, 14, net)
        c["trials"] = make_trials((20, 35, 1, 28), 8.0, 3, 4)
    elif base == "inf":                  # Δtmax = ∞ (exponential only)
        assert kind == "exponential"
        c = _model(3, kind, np.inf, 15, net)
        c["trials"] = make_trials((25, 0, 31, 22), 8.0, 3, 5)
    elif base == "dense":                # ~8 parents a window, 6 trials of ~330 events: the shape that keeps its child slices
        c = _model(4, kind, 1.0, 16, net)
        c["trials"] = make_trials((330, 350, 0, 310, 340, 330), 40.0, 4, 6, tie_seams=True)
    elif base == "cut":                  # θ in [20, 40]: a usable cut near 2 on trials of length 32
        c = _model(5, kind, 0.05, 17, net, theta_range=(1.0, 2.0))
        c["trials"] = make_trials((150, 170, 0, 160), 32.0, 5, 7, tie_seams=True, zeros=1)
    elif base == "slow":                 # "ties" with θ = 1e-6 on the diagonal: the cut's expected window is far above 8192 parents
        c = case("ties" + ("-net" if net else ""))
        c["theta"] = np.where(np.eye(c["N"]) > 0, 1e-6, c["theta"])
    elif base == "silent":               # "ties" with W = 0: the empty cut, which no derivative may use.  Nothing can leak across
        c = case("ties" + ("-net" if net else ""))      # a seam here (there is no excitation at all): the leak check does not
        c["W"] = np.zeros_like(c["W"])                  # apply, the starts themselves are held to the restatement
    elif base == "chunk-edge":           # trial starts at stacked indices 127, 256, 513 (a chunk's last, first, second event); node 2
        c = _model(3, kind, 1.0, 21, net)                # absent from trial 1
        c["trials"] = chunk_edge_trials((127, 128 + 128, 129 + 3 * 128, 700), 900, 3, 16.0, 9)
        e, n, T = c["trials"][1]
        c["trials"][1] = (e, np.where(n == 2, 1, n), T)
    elif base == "group-edge":           # 8300 events, N = 2, trial starts on either side of index 8192 (64 chunks: a group's end)
        c = _model(2, kind, 0.5, 22, net)
        c["trials"] = chunk_edge_trials((4000, 8191, 8193), 8300, 2, 200.0, 10)
    else:
        raise KeyError(name)
    c["name"] = name
    return c


LL_CASES = ("counts", "empty-ends", "ties", "wide", "inf", "dense", "counts-logit", "ties-logit", "dense-logit", "ties-net",
            "dense-net", "ties-net-logit")
REC_CASES = ("ties", "inf", "cut", "cut-net", "empty-ends")
REC_NO_CUT = ("slow", "silent")
COMP_SMALL = ("counts", "ties", "inf", "ties-logit", "empty-ends", "dense-net")
COMP_EDGES = ("chunk-edge", "chunk-edge-logit", "group-edge")


@functools.lru_cache(maxsize=None)
def prepared(name, recursive=False):
    """(case, model, Result, tail) computed once per session."""
    c = case(name)
    m = gr.model_of(c)
    res, tail = evaluate(m, c["trials"], recursive=recursive)
    return c, m, res, tail


def chunk_edge_trials(starts, M, N, T, seed):
    """Trials whose first events have the given stacked indices (after index 0), M events in all, on [0, T] each."""
    edges = [0] + list(starts) + [M]
    return make_trials([b - a for a, b in zip(edges[:-1], edges[1:])], T, N, seed)
