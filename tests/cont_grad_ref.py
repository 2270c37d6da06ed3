"""Extended-precision restatement of the continuous log-likelihood and its gradient in params! order
[params(baseline); θ | μ; τ; W], written from the formulas at the top of csrc/cont_grad.hip and the conventions the oracle
documents (oracle/mp_eval.py), not from the kernels or the oracle's C:

    λ_i        = base_c(t_i) + Σ_j a[p_j,c]·W[p_j,c]·ħ(Δ_ij),   c the node of event i,  Δ_ij = fl(t_i - t_j),  g_i = 1/λ_i
    ħ(Δ)       = θ e^{-θΔ}   or the logit-normal density at x = Δ/Δtmax (not divided by Δtmax), counted only for 0 < x < 1
    ll         = -Σ_c ∫base_c - Σ_{p,c} cnt[p]·W[p,c]·mask[p,c] + Σ_i log λ_i
    ∂/∂λ0[c]   = -T + Σ_{i on c} g_i
    ∂/∂y[g,c]  = -(trapezoid weight of grid point g, duration ignored) + Σ_{i on c} g_i·w_g(t_i)           (grid baseline)
    ∂/∂W[p,c]  = -cnt[p]·mask[p,c] + a Σ g_i ħ                 ∂/∂θ[p,c] = a·w Σ g_i (1 - θΔ) e^{-θΔ}
    ∂/∂μ[p,c]  = a·w Σ g_i ħ·τ(ℓ - μ)                          ∂/∂τ[p,c] = a·w Σ g_i ħ·(1/τ - (ℓ - μ)²)/2,   ℓ = logit(x)

Conventions.  Windowed form: event j < i is a parent of i when times[j] > fl(t_i - Δtmax), decided in float64 as the data
layout decides it (a tie is a pair, Δ exactly Δtmax is not); the network integral is masked (mask = A).  Recursive form
(exponential only): every j < i with t_j > 0 (D9), mask = 1 in the integral although a = A still multiplies the sum (D7).
x = fl(Δ·fl(1/Δtmax)) in float64 (exact where Δtmax is a power of two, as in every logit-normal case of the suites).
w_g(t): t in [x[a], x[a+1]) gives w_a = (x[a+1] - t)/(x[a+1] - x[a]), w_{a+1} = (t - x[a])/(x[a+1] - x[a]); t >= x[G-1]
goes wholly to the last point, where base = y[G-1].  A column shard (columns = (begin, end)) owns the terms of its child
nodes; every other entry is an exact zero and ll is the sum over its columns.  Matrices are [parent, child], stored
p fastest; the grid block is g fastest, one run of G per node.

Next to every gradient entry stand its parameter-independent term `const` (float64, as the formula above gives it in double:
-T, -0.5·((x[g]-x[g-1]) + (x[g+1]-x[g])), -cnt·mask, 0) and the ingredients of a rounding bound, all sums over the entry's
terms with every difference split into its two parts ((1 - θΔ) -> 1 and θΔ, (ℓ - μ) -> ℓ and μ, (1/τ - (ℓ-μ)²)):

    S   Σ |term|                                    Q   Σ |∂term/∂Δ|   (exponential; 0 for the logit-normal routes, which read
    n   number of terms                                  exact delays)
    R   Σ |term|·ρ_term   (+ absolute extras)       U   Σ |term| over the terms whose e^{-θΔ} is below the smallest double
                                                         (θΔ > 708: a float64 evaluation may drop them entirely)

    bound = 2⁻⁵³·(R + (n + 8)·(S + |const|)) + δ·(Q + Θ_c·S) + U (+ tail),        r = R/S + n + 8 in the issue's r·2⁻⁵³·S + δ·Q

ρ_term counts the roundings that reach one term, read off the kernels' arithmetic:
  * 1/λ_i: λ_i is a sum of K_i + 1 non-negative numbers (W >= 0, base > 0), so K_i + 8 (the sum in any order, the baseline's
    interpolation, the division) plus the mean over its own terms of their amplified argument error, 4·Σ_j λterm_j·amp_j/λ_i;
    the recursion adds its N-term sum over parents and 7 roundings per decay step between the fold of parent j and child i;
  * the term: 12 (the table exponential is within 2 ulp = 4·2⁻⁵³; the products with θ, g, a·w; θΔ and 1 - θΔ) + 4·amp_term;
    amp = θΔ for the exponential (the argument θ·Δ·64/ln 2 carries 4 relative roundings: Δ, the rate constant, two products;
    the recursion's product of per-gap decays sums to the same θΔ), and |z|·√τ(|ℓ| + 4 + |ℓ-μ|) + 3z², z = √τ(ℓ-μ), for the
    logit-normal exponent -z²/2 (ℓ = log(x²/(x(1-x))) carries 4 argument roundings and its own);
    the recursion: + 7 (S) or 10 (R = Σ Δ e^{-θΔ}, one product and one sum more) per decay step;
  * absolute extras: the μ and τ entries see the error of ℓ - μ outside the exponent too: u·8 and v/τ·2|z|√τ(|ℓ| + 4 + |ℓ-μ|).
(n + 8): the sum of the entry's terms in any order, its scaling by a, a·w, 0.5/τ and the addition to const.  δ is the record
format's delay step of the route under test (0 for the exact 16-byte records): the slices round the delay to
Δtmax·2^-(48 - bits) and keep it inside [1, 2^(48-bits) - 1] (a tie moves by one whole step), bits the longer of the bit
lengths of N and of the largest item; the 8-byte pair list of pass A has 48 bits.  δ·Q is the terms' own shift, δ·Θ_c·S that
of g_i (|∂λ_i/∂Δ| <= Θ_c·λ_i, Θ_c the largest θ of column c).  `far`: pairs with θΔ > 1416 stay out of the sums (each
term is below e^-1416 of its coefficient, nothing even long double registers next to 2⁻⁵³·S).  `tiny` = 2⁻¹⁰⁰⁰ per pair of
the entry with a != 0, far ones included, is added to the bound: below 2⁻¹⁰²² a double has no relative precision, and a
float64 recursion may keep a subnormal of a far pair.  Entries whose bound is 0 have no pair at all: they equal const.  The truncated window drops less than 2⁻⁶⁰·λ_i per child
(csrc/cont_recursive.hip): `tail`.  First order and worst case; derived, not measured.  Entries with S = 0 equal const.

Everything is evaluated in numpy's long double where that is the x87 80-bit format or wider, otherwise in mpmath numbers of
40 digits (tests/adjacency_ref.backend); real=np.float64 gives the plain double evaluation of the same sums, `order` the
order in which the pairs enter them.  Test code only."""
import collections
import functools

import numpy as np

from adjacency_ref import backend

EPS = 2.0 ** -53
FLUSH = 708.0

Model = collections.namedtuple("Model", "N lam0 W theta mu tau dt_max A grid_x")
Result = collections.namedtuple("Result", "ll grad const S Q R U n tiny theta_col nb blocks")
"""grad in the evaluation's number type; const, S, Q, R, U, n, theta_col float64 [P]; blocks = ((name, start, stop), ...)."""


def model(lam0, W, theta=None, mu=None, tau=None, dt_max=1.0, A=None, grid_x=None):
    W = np.asarray(W, dtype=np.float64)
    return Model(W.shape[0], np.asarray(lam0, dtype=np.float64), W, theta, mu, tau, float(dt_max), A,
                 None if grid_x is None else np.asarray(grid_x, dtype=np.float64))


class _Seg:
    """Sums of per-pair values by an integer key, in the order the pairs are given."""

    def __init__(self, b, key, nseg):
        self.b, self.nseg = b, nseg
        self.o = np.argsort(key, kind="stable")
        ks = key[self.o]
        self.starts = np.searchsorted(ks, np.arange(nseg), side="left")
        self.full = np.searchsorted(ks, np.arange(nseg), side="right") > self.starts

    def sum(self, v, real=True):
        out = self.b.zeros(self.nseg) if real else np.zeros(self.nseg)
        if len(v) and self.full.any():
            out[self.full] = np.add.reduceat(v[self.o], self.starts[self.full])
        return out


def column_pairs(t, n0, c, dt_max, recursive):
    """Children of node c (event indices, time order) and its pairs as (child slot, parent event index)."""
    ev = np.nonzero(n0 == c)[0]
    if recursive:
        first = np.minimum(int((t <= 0.0).sum()), ev)                  # sorted, non-negative times: the t = 0 events lead
    else:
        first = np.minimum(np.searchsorted(t, t[ev] - dt_max, side="right"), ev)
    cnt = ev - first
    slot = np.repeat(np.arange(len(ev)), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(first, cnt)
    return ev, slot, j


def grid_weights(b, gx, t):
    """(a, w_a, w_{a+1}, last) of the float64 times t on the grid gx; last: t >= gx[-1]."""
    G = len(gx)
    last = ~(t < gx[G - 1])
    a = np.clip(np.searchsorted(gx, t, side="right") - 1, 0, G - 2)
    x0, x1, tt = b.arr(gx[a]), b.arr(gx[a + 1]), b.arr(t)
    return a, (x1 - tt) / (x1 - x0), (tt - x0) / (x1 - x0), last


def evaluate(m, times, nodes, T, recursive=False, columns=None, real=None, order="forward", seed=0):
    b = backend(real)
    f = lambda v: np.asarray(v, dtype=np.float64)                       # scales are kept in double
    N = m.N
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    assert np.all(np.diff(t) >= 0) and (len(t) == 0 or t[0] >= 0.0) and np.all(m.W >= 0)
    expo = m.theta is not None
    assert expo or not recursive
    cnt = np.bincount(n0, minlength=N).astype(np.float64)
    G = 0 if m.grid_x is None else len(m.grid_x)
    nb = N * G if G else N
    NN = N * N
    names = ("theta",) if expo else ("mu", "tau")
    blocks = (("base", 0, nb),) + tuple((nm, nb + i * NN, nb + (i + 1) * NN) for i, nm in enumerate(names + ("W",)))
    off = {nm: lo for nm, lo, hi in blocks}
    P = blocks[-1][2]
    grad = b.zeros(P)
    out = {k: np.zeros(P) for k in ("const", "S", "Q", "R", "U", "n", "tiny", "theta_col")}
    c0, c1 = (0, N) if columns is None else columns
    A = np.ones((N, N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    mask = A if not recursive else np.ones((N, N))
    rng = np.random.default_rng(seed)
    one, two = b.num(1.0), b.num(2.0)
    ll = b.num(0.0)
    if G:
        gx = m.grid_x
        left, right = np.concatenate([[0.0], np.diff(gx)]), np.concatenate([np.diff(gx), [0.0]])
        trap = 0.5 * (left + right)                                     # float64, as the formula gives it in double
    for c in range(c0, c1):
        ev, slot, j = column_pairs(t, n0, c, m.dt_max, recursive)
        nch = len(ev)
        if order == "reversed":
            slot, j = slot[::-1], j[::-1]
        elif order == "permuted":
            q = rng.permutation(len(j))
            slot, j = slot[q], j[q]
        p = n0[j]
        d64 = t[ev][slot] - t[j]
        nfar = np.zeros(N)
        if expo:                                                        # θΔ > 1416: below e^-1416 of θ, see `far` in the docstring
            far = m.theta[p, c] * d64 > 2.0 * FLUSH
            nfar = np.bincount(p[far & (A[p, c] != 0)], minlength=N).astype(np.float64)
            slot, j, p, d64 = slot[~far], j[~far], p[~far], d64[~far]
        a, w = A[p, c], m.W[p, c]
        by_child, by_parent = _Seg(b, slot, nch), _Seg(b, p, N)
        steps = np.zeros(len(j))
        if recursive:                                                   # decay steps between the fold of parent j and child i
            steps = (slot - np.searchsorted(ev, j, side="right")).astype(np.float64)
        # ---- baseline at the children, integral terms
        tc = t[ev]
        if G:
            y = b.arr(m.lam0[c])
            ga, w_lo, w_hi, last = grid_weights(b, gx, tc)
            base = y[ga + 1] * w_hi + y[ga] * w_lo
            if last.any():
                base[last] = y[G - 1]
            ll = ll - ((y[1:] + y[:-1]) / two * (b.arr(gx[1:]) - b.arr(gx[:-1]))).sum()
            out["const"][c * G:(c + 1) * G] = -trap
        else:
            base = b.zeros(nch) + b.num(m.lam0[c])
            ll = ll - b.num(m.lam0[c]) * b.num(float(T))
            out["const"][c] = -float(T)
        ll = ll - (b.arr(cnt) * b.arr(m.W[:, c]) * b.arr(mask[:, c])).sum()
        kW = off["W"] + c * N
        out["const"][kW:kW + N] = -cnt * mask[:, c]
        # ---- the pairs' impulse values
        d = b.arr(d64)
        if expo:
            th64 = m.theta[p, c]
            th = b.arr(th64)
            thd = th * d
            e = b.exp(-thd)
            hbar = th * e
            amp = th64 * d64
            flushed = amp > FLUSH
            live = np.ones(len(j), dtype=bool)
        else:
            x64 = d64 * (1.0 / m.dt_max)
            live = (x64 > 0.0) & (x64 < 1.0)
            x = b.arr(np.where(live, x64, 0.5))
            mu, tau = b.arr(m.mu[p, c]), b.arr(m.tau[p, c])
            ell = b.log(x / (one - x))
            dl = ell - mu
            z2 = tau * dl * dl
            hbar = b.exp(-z2 / two) * b.sqrt(tau / (two * b.pi())) / (x * (one - x))
            hbar[~live] = b.zeros(int((~live).sum()))
            z = np.sqrt(f(z2))
            spread = np.abs(f(ell)) + 4.0 + np.abs(f(dl))
            amp = z * np.sqrt(m.tau[p, c]) * spread + 3.0 * f(z2)
            flushed = f(z2) / 2.0 > FLUSH
        lt = b.arr(a * w) * hbar                                         # the pairs' terms of λ
        lam = base + by_child.sum(lt)
        ll = ll + (b.log(lam).sum() if nch else b.num(0.0))
        g = one / lam
        K = np.bincount(slot, minlength=nch).astype(np.float64)
        lam64 = f(lam)
        rho_i = K + 8.0 + (4.0 * by_child.sum(f(lt) * np.where(flushed, 0.0, amp), real=False)
                           + 7.0 * by_child.sum(f(lt) * steps, real=False)) / lam64 + (N + 6.0 if recursive else 0.0)
        gi = g[slot] if len(j) else b.zeros(0)
        rho = (rho_i[slot] if len(j) else np.zeros(0)) + 12.0 + 4.0 * np.where(flushed, 0.0, amp)

        def put(name, value, absterm, qterm, extra=None, rstep=7.0):
            k = off[name] + c * N
            grad[k:k + N] = b.arr(out["const"][k:k + N]) + value
            af = f(absterm)
            out["S"][k:k + N] = by_parent.sum(af, real=False)
            out["R"][k:k + N] = by_parent.sum(af * (rho + rstep * steps) + (0.0 if extra is None else extra), real=False)
            out["U"][k:k + N] = by_parent.sum(np.where(flushed, af, 0.0), real=False)
            out["n"][k:k + N] = by_parent.sum((live & (a != 0)).astype(np.float64), real=False)
            out["tiny"][k:k + N] = 2.0 ** -1000 * (out["n"][k:k + N] + nfar)
            if recursive:                                               # the terms reach the entry through one sum over the children
                out["n"][k:k + N] = np.minimum(out["n"][k:k + N], nch)
            if qterm is not None:
                out["Q"][k:k + N] = by_parent.sum(f(qterm), real=False)
            out["theta_col"][k:k + N] = m.theta[:, c].max() if expo else 0.0

        ba, baw = b.arr(a), b.arr(a * w)
        tW = gi * ba * hbar
        put("W", by_parent.sum(tW), tW, tW * th if expo else None)
        if expo:
            u = gi * baw * e
            put("theta", by_parent.sum(u) - by_parent.sum(u * thd), u * (one + thd), u * th * (two + thd), rstep=10.0)
        else:
            u = gi * baw * hbar * tau
            put("mu", by_parent.sum(u * ell) - by_parent.sum(u * mu), u * (abs(ell) + abs(mu)), None, extra=8.0 * f(u))
            v = gi * baw * hbar / two
            vt = f(v) / m.tau[p, c]
            put("tau", by_parent.sum(v / tau) - by_parent.sum(v * dl * dl), v * (one / tau + dl * dl), None,
                extra=vt * 2.0 * z * np.sqrt(m.tau[p, c]) * spread)
        # ---- the baseline block
        g64 = f(g)
        thc = m.theta[:, c].max() if expo else 0.0
        if G:
            k = c * G
            terms = [(ga[~last], (g * w_lo)[~last]), (ga[~last] + 1, (g * w_hi)[~last]), (np.full(int(last.sum()), G - 1), g[last])]
            rr = [rho_i[~last] + 6.0, rho_i[~last] + 6.0, rho_i[last]]
            val = b.zeros(G)
            for (key, v), r_ in zip(terms, rr):
                sg = _Seg(b, key, G)
                val = val + sg.sum(v)
                out["S"][k:k + G] += sg.sum(f(v), real=False)
                out["R"][k:k + G] += sg.sum(f(v) * r_, real=False)
                out["n"][k:k + G] += sg.sum(np.ones(len(key)), real=False)
            out["tiny"][k:k + G] = 2.0 ** -1000 * out["n"][k:k + G]
            grad[k:k + G] = b.arr(out["const"][k:k + G]) + val
            out["theta_col"][k:k + G] = thc
        else:
            grad[c] = b.num(out["const"][c]) + (g.sum() if nch else b.num(0.0))
            out["S"][c], out["R"][c], out["n"][c], out["theta_col"][c] = g64.sum(), (g64 * rho_i).sum(), nch, thc
            out["tiny"][c] = 2.0 ** -1000 * nch
    return Result(ll=ll, grad=grad, nb=nb, blocks=blocks, **out)


def bound(res, delta=0.0, tail=None):
    """The per-entry bound of the module docstring (float64 [P]); tail: an array added as it is."""
    B = EPS * (res.R + (res.n + 8.0) * (res.S + np.abs(res.const))) + delta * (res.Q + res.theta_col * res.S) + res.U
    B = np.where(res.S > 0, B, 0.0) + res.tiny
    return B if tail is None else B + np.where(res.S > 0, tail, 0.0)


def window_tail(res, m, times, nodes, T):
    """What the truncated window may drop: less than 2⁻⁶⁰·λ_i per child all parents together, so 2⁻⁶⁰ per child of
    Σ_p g·a·w·θ·e: at most children_c·2⁻⁶⁰/W[p,c] in ∂/∂W[p,c], children_c·2⁻⁶⁰·span in ∂/∂θ[p,c] (|1 - θΔ|/θ <= Δ <= span for
    the dropped pairs, θΔ > 41), and a relative 2⁻⁶⁰ of every g_i besides."""
    N = m.N
    kids = np.bincount(np.asarray(nodes, dtype=np.int64) - 1, minlength=N).astype(np.float64)
    span = float(times[-1] - times[0]) if len(times) else 0.0
    tail = 2.0 ** -60 * res.S
    off = {nm: lo for nm, lo, hi in res.blocks}
    with np.errstate(divide="ignore"):
        invW = np.where(m.W > 0, 1.0 / m.W, 0.0)
    tail[off["W"]:off["W"] + N * N] += (2.0 ** -60 * kids[None, :] * invW).ravel(order="F")
    tail[off["theta"]:off["theta"] + N * N] += np.repeat(2.0 ** -60 * kids * span, N)
    return tail


def check(got, res, delta=0.0, tail=None):
    """(largest error/bound over the entries with a bound, indices of the entries outside the bound or, where the bound is 0,
    different from const).  No entry is skipped."""
    got = np.asarray(got, dtype=np.float64)
    B = bound(res, delta, tail)
    err = np.abs(np.asarray(got - res.grad, dtype=np.float64))
    data = B > 0
    ratio = np.zeros(len(got))
    ratio[data] = err[data] / B[data]
    bad = np.nonzero(np.where(data, ~(err <= B), got != res.const))[0]
    return (float(ratio.max()) if data.any() else 0.0), bad, err, B


def explain(got, res, N, bad, err, B, limit=8):
    """The worst entries: block, (p, c), got, want, S, Q, error/bound."""
    lines = []
    worst = sorted(bad, key=lambda k: -(err[k] / B[k] if B[k] > 0 else np.inf))[:limit]
    for k in worst:
        name, lo, hi = next(bl for bl in res.blocks if bl[1] <= k < bl[2])
        i = k - lo
        G = (hi - lo) // N
        where = "(p %d, c %d)" % (i % N, i // N) if name != "base" else "(c %d)" % i if G == 1 else "(g %d, c %d)" % (i % G, i // G)
        lines.append(f"{name} {where}: got {got[k]!r} want {float(res.grad[k])!r} const {res.const[k]!r} S {res.S[k]:.3g} "
                     f"Q {res.Q[k]:.3g} n {res.n[k]:.0f} error/bound {err[k] / B[k] if B[k] > 0 else float('inf'):.3g}")
    return "\n".join(lines)


# -------------------------------------------------------------------------------------------------------------- census
def census(m, times, nodes, recursive=False):
    """What the inputs contain, in integers: ties (pairs with Δ = 0), edge (j < i with Δ exactly Δtmax: not pairs), near
    (pairs with 0 < x < 1 and x or 1 - x within 2⁻⁴⁰), flushed (pairs with θΔ > 708), empty (nodes without events), never
    ((p, c), both with events, that no window joins), single (nodes with one event), zero_time, on_grid / last_cell / at_end
    (events on a grid point / at or beyond the last but one point / at the last point), pairs, longest window."""
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    N = m.N
    out = collections.Counter(ties=0, edge=0, near=0, flushed=0, pairs=0, longest=0)
    joined = np.zeros((N, N), dtype=bool)
    for c in range(N):
        ev, slot, j = column_pairs(t, n0, c, m.dt_max, recursive)
        d = t[ev][slot] - t[j]
        out["pairs"] += len(j)
        out["ties"] += int((d == 0).sum())
        if len(j):
            out["longest"] = max(out["longest"], int(np.bincount(slot).max()))
            joined[np.unique(n0[j]), c] = True
        if not recursive and np.isfinite(m.dt_max):
            lo = np.searchsorted(t, t[ev] - m.dt_max, side="left")
            hi = np.searchsorted(t, t[ev] - m.dt_max, side="right")
            exact = (t[ev] - m.dt_max) + m.dt_max == t[ev]
            out["edge"] += int(((hi - lo) * exact).sum())
        if m.theta is not None:
            out["flushed"] += int((m.theta[n0[j], c] * d > FLUSH).sum())
        else:
            x = d * (1.0 / m.dt_max)
            out["near"] += int(((x > 0) & (x < 1) & ((x <= 2.0 ** -40) | (1.0 - x <= 2.0 ** -40))).sum())
    cnt = np.bincount(n0, minlength=N)
    out["empty"] = int((cnt == 0).sum())
    out["single"] = int((cnt == 1).sum())
    out["never"] = int((~joined & (cnt[:, None] > 0) & (cnt[None, :] > 0)).sum())
    out["zero_time"] = int((t == 0.0).sum())
    if m.grid_x is not None:
        out["on_grid"] = int(np.isin(t, m.grid_x).sum())
        out["last_cell"] = int((t >= m.grid_x[-2]).sum())
        out["at_end"] = int((t == m.grid_x[-1]).sum())
    return dict(out)


# --------------------------------------------------------------------------------------------------------------- cases
GRID5 = np.array([0.0, 0.15, 0.4, 0.85, 1.0])
"""The non-uniform grid of the G cases, as fractions of T."""


def _grid(case, rng):
    gx = GRID5 * case["T"]
    case.update(grid_x=gx, lam0=np.exp(rng.normal(0.0, 0.4, (case["N"], 5))))
    t = case["times"]
    M = len(t)
    for i, v in ((M // 5, gx[1]), (M // 2, gx[2]), (M - 40, gx[3]), (M - 1, gx[4])):       # events exactly on grid points
        t[i] = v
    order = np.argsort(t, kind="stable")
    case["times"], case["nodes"] = t[order], case["nodes"][order]
    return case


def windowed_case(kind="exponential", network=False, lgcp=False, seed=5):
    """W-exp / W-logit / W-net: N = 7, M = 3000, T = 200, Δtmax = 1, times on the dyadic grid 2⁻¹⁰ (so Δ = Δtmax and Δ = 0
    occur exactly), a burst of 90 events in 0.6, node 7 empty, node 6 with one event, node 5 with three events after
    everything else (no window of another column holds them), 15 ties, 12 pairs at Δ = Δtmax, three pairs at Δ = 2⁻⁴¹ and
    three at 1 - 2⁻⁴¹ on nodes (1 -> 2) and (3 -> 4), whose μ = -28 / +28 put the density's mass there."""
    rng = np.random.default_rng(seed)
    N, M, T = 7, 3000, 200.0
    k = np.sort(rng.integers(1, int(196.0 * 1024), M))
    t = k / 1024.0
    nodes = rng.integers(1, 5, M).astype(np.int64)                       # nodes 1..4 carry the bulk
    t[700:730:2] = t[701:731:2]                                          # ties
    t[1200:1224:2] = t[1140:1164:2] + 1.0                                # Δ exactly Δtmax
    t[2000:2090] = t[2000] + np.sort(rng.integers(0, 615, 90)) / 1024.0  # the burst
    for q, (i, dlt) in enumerate(((300, 2.0 ** -41), (900, 2.0 ** -41), (1500, 2.0 ** -41),
                                  (400, 1.0 - 2.0 ** -41), (1000, 1.0 - 2.0 ** -41), (1700, 1.0 - 2.0 ** -41))):
        t[i + 1] = t[i] + dlt
        nodes[i], nodes[i + 1] = (1, 2) if q < 3 else (3, 4)
    t[-3:] = (199.0, 199.25, 199.5)
    nodes[-3:] = 5
    nodes[1600] = 6
    order = np.argsort(t, kind="stable")
    t, nodes = t[order], nodes[order]
    W = rng.uniform(0.05, 1.0, (N, N)) / N * 2.0
    W[1, 2] = W[4, 4] = W[0, 3] = 0.0
    theta = np.exp(rng.uniform(np.log(0.5), np.log(40.0), (N, N)))
    theta[0, 0], theta[3, 1], theta[1, 1] = 0.5, 40.0, 2000.0            # the ends, and one rate whose exponential flushes
    mu = rng.normal(0.0, 1.0, (N, N))
    tau = rng.uniform(0.5, 2.0, (N, N))
    mu[0, 1], mu[2, 3] = -28.0, 28.0
    A = None
    if network:
        A = (rng.uniform(size=(N, N)) < 0.6).astype(np.float64)
        A[2, :] = 0.0
        A[:, 3] = 0.0
        A[0, 0] = A[1, 1] = 1.0
    case = dict(N=N, T=T, times=t, nodes=nodes, kind=kind, dt_max=1.0, lam0=rng.uniform(0.5, 1.5, N), W=W, theta=theta, mu=mu,
                tau=tau, A=A, grid_x=None, recursive=False)
    return _grid(case, rng) if lgcp else case


def sole_case(lgcp=False):
    """D: N = 3, M = 900, node 3 empty: with one item per node the slices store every entry themselves."""
    rng = np.random.default_rng(41)
    N, M, T = 3, 900, 120.0
    t = np.sort(rng.integers(1, int(T * 1024), M)) / 1024.0
    t[100:120:2] = t[101:121:2]
    t = np.sort(t)
    nodes = rng.integers(1, 3, M).astype(np.int64)
    W = rng.uniform(0.05, 1.0, (N, N)) / N * 2.0
    W[0, 1] = 0.0
    case = dict(N=N, T=T, times=t, nodes=nodes, kind="exponential", dt_max=1.0, lam0=rng.uniform(0.5, 1.5, N), W=W,
                theta=rng.uniform(0.5, 8.0, (N, N)), mu=None, tau=None, A=None, grid_x=None, recursive=False)
    return _grid(case, rng) if lgcp else case


def long_case(kind):
    """L: N = 2, M = 600, Δtmax = 64 >= T = 60: every earlier event is a parent, 179 700 pairs in two items."""
    rng = np.random.default_rng(43)
    N, M, T = 2, 600, 60.0
    t = np.sort(rng.integers(1, int(T * 1024), M)) / 1024.0
    t[50:60:2] = t[51:61:2]
    t = np.sort(t)
    nodes = rng.integers(1, 3, M).astype(np.int64)
    return dict(N=N, T=T, times=t, nodes=nodes, kind=kind, dt_max=64.0, lam0=rng.uniform(0.5, 1.5, N),
                W=rng.uniform(0.1, 1.0, (N, N)), theta=rng.uniform(0.05, 1.0, (N, N)), mu=rng.normal(-2.0, 1.0, (N, N)),
                tau=rng.uniform(0.5, 2.0, (N, N)), A=None, grid_x=None, recursive=False)


TIME_PART_SHAPES = {"P4": (9, 1000, 4.0, 1.0), "P2": (10, 1000, 5.2, 1.0), "P2-inf": (10, 300, 30.0, np.inf)}
"""(N, M, T, Δtmax) of the cases that the default rule lays out in XCD time parts (tests/slices_ref.time_parts): a mean window
of 218 pairs (TP = 4, 40 items of which 4 are padding), of 175, between the 160 above which the plan does not slice and the
192 of TP = 4 (TP = 2, 24 items, 4 padding), and every earlier event with Δtmax = ∞ (149.5; TP = 2, 24 items, 4 padding)."""


def time_part_case(shape, kind="exponential", network=False, seed=61):
    """P4-exp / P4-logit / P4-net, P2-exp / P2-logit, P2-inf: built like windowed_case on the dyadic grid 2⁻¹⁰, every time
    distinct except 12 planted ties (whose two events sit on different nodes, so that no two categories of a child have the
    same weight: tests/test_cascades_host.py's condition), exact zeros in W, θ·Δtmax from 0.5 to 40 (Δtmax = ∞: θ from 0.05
    to 4).  Nodes 1..N-3 carry the bulk; node N-2 has one event; node N-1 has 40, all inside the last quarter of the event
    indices, so its first item is empty in every time-part layout and still owns the column's constants; node N has none
    and is the node the padding items name."""
    N, M, T, dt_max = TIME_PART_SHAPES[shape]
    rng = np.random.default_rng(seed)
    k = np.sort(rng.choice(np.arange(1, int(T * 1024)), M, replace=False))
    t = k / 1024.0
    tied = np.arange(M // 5, M // 5 + 24, 2)
    t[tied] = t[tied + 1]                                                # sorted still: t[i] moves up to its neighbour
    nodes = rng.integers(1, N - 2, M).astype(np.int64)                   # nodes 1..N-3 carry the bulk
    nodes[tied + 1] = nodes[tied] % (N - 3) + 1                          # a tie's two events on different nodes
    late = 3 * M // 4 + np.sort(rng.choice(M - 3 * M // 4, 40, replace=False))
    nodes[late] = N - 1
    nodes[3 * M // 8] = N - 2
    assert np.all(np.diff(t) >= 0)
    W = rng.uniform(0.05, 1.0, (N, N)) / N * 2.0
    W[1, 2] = W[4, 4] = W[0, 3] = 0.0
    if np.isfinite(dt_max):
        theta = np.exp(rng.uniform(np.log(0.5), np.log(40.0), (N, N))) / dt_max
        theta[0, 0], theta[3, 1] = 0.5 / dt_max, 40.0 / dt_max
    else:
        theta = np.exp(rng.uniform(np.log(0.05), np.log(4.0), (N, N)))
    mu = rng.normal(0.0, 1.0, (N, N))
    tau = rng.uniform(0.5, 2.0, (N, N))
    A = None
    if network:
        A = (rng.uniform(size=(N, N)) < 0.6).astype(np.float64)
        A[2, :] = 0.0
        A[:, 3] = 0.0
        A[0, 0] = A[1, 1] = 1.0
    return dict(N=N, T=T, times=t, nodes=nodes, kind=kind, dt_max=dt_max, lam0=rng.uniform(0.5, 1.5, N), W=W, theta=theta, mu=mu,
                tau=tau, A=A, grid_x=None, recursive=False)


def large_item_data(seed=8):
    """N = 8, M = 140 000 uniform times on T = 680 with Δtmax = 1: about 2.9·10⁷ pairs, a mean window of about 206, so TP = 4 and
    32 items of about 4375 children -- more than the 4096 that bound an item of the default layout."""
    rng = np.random.default_rng(seed)
    N, M, T = 8, 140_000, 680.0
    return np.sort(rng.uniform(0.0, T, M)), rng.integers(1, N + 1, M).astype(np.int64), T, N, 1.0


REC_M = {1: 1500, 64: 2500, 65: 2500, 257: 2000, 513: 2000, 1025: 2000}


def recursive_case(N, lgcp=False):
    """R-N: the full recursion.  Three events at t = 0, 10 ties, node 2 (N > 1) without events (a column without children);
    N = 257: nodes 129..256 without events (a part none of whose nodes has events); a network mask from N = 64 on."""
    rng = np.random.default_rng(300 + N)
    M, T = REC_M[N], 300.0
    t = np.sort(rng.uniform(0.0, T, M))
    t[:3] = 0.0
    t[200:220:2] = t[201:221:2]
    t = np.sort(t)
    nodes = rng.integers(1, N + 1, M).astype(np.int64)
    if N > 1:
        nodes[nodes == 2] = 1
    if N == 257:
        nodes[(nodes >= 129) & (nodes <= 256)] -= 128
    W = rng.uniform(0.0, 1.0, (N, N)) / max(N, 2) * 2.0
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64) if N >= 64 else None
    case = dict(N=N, T=T, times=t, nodes=nodes, kind="exponential", dt_max=1.0, lam0=rng.uniform(0.5, 1.5, N), W=W,
                theta=rng.uniform(1.0, 5.0, (N, N)), mu=None, tau=None, A=A, grid_x=None, recursive=True)
    return _grid(case, rng) if lgcp else case


def window_case(network=False):
    """C, C-net: the data of test_recursive_through_the_truncated_window_matches_the_recursion (homogeneous baseline, standard
    and network process): θ in [20, 40] on T = 400 puts the cut near 2 against 4000 events -- far on the window's side."""
    N, M, T = 64, 4000, 400.0
    rng = np.random.default_rng(77)
    t = np.sort(rng.uniform(0.0, T, M))
    t[:3] = 0.0
    nodes = rng.integers(1, N + 1, M).astype(np.int64)
    th = rng.uniform(20.0, 40.0, (N, N))
    W = rng.uniform(0.0, 1.0, (N, N)) / N
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64) if network else None
    return dict(N=N, T=T, times=t, nodes=nodes, kind="exponential", dt_max=0.05, lam0=rng.uniform(0.5, 1.5, N), W=W, theta=th,
                mu=None, tau=None, A=A, grid_x=None, recursive=True)


CASES = {
    "W-exp": lambda: windowed_case("exponential"), "W-logit": lambda: windowed_case("logitnormal"),
    "W-net": lambda: windowed_case("exponential", network=True), "W-net-logit": lambda: windowed_case("logitnormal", network=True),
    "D": sole_case, "L-exp": lambda: long_case("exponential"), "L-logit": lambda: long_case("logitnormal"),
    "C": window_case, "C-net": lambda: window_case(network=True), "G-W": lambda: windowed_case("exponential", lgcp=True), "G-D": lambda: sole_case(lgcp=True),
    "G-R": lambda: recursive_case(65, lgcp=True),
}
CASES.update({"R-%d" % n: (lambda n=n: recursive_case(n)) for n in REC_M})
TIME_PART_CASES = ("P4-exp", "P4-logit", "P4-net", "P2-exp", "P2-logit", "P2-inf")
CASES.update({"P4-exp": lambda: time_part_case("P4"), "P4-logit": lambda: time_part_case("P4", "logitnormal"),
              "P4-net": lambda: time_part_case("P4", network=True), "P2-exp": lambda: time_part_case("P2"),
              "P2-logit": lambda: time_part_case("P2", "logitnormal"), "P2-inf": lambda: time_part_case("P2-inf")})


def model_of(case):
    expo = case["kind"] == "exponential"
    return model(case["lam0"], case["W"], theta=case["theta"] if expo else None, mu=None if expo else case["mu"],
                 tau=None if expo else case["tau"], dt_max=case["dt_max"], A=case["A"], grid_x=case["grid_x"])


@functools.lru_cache(maxsize=None)
def prepared(name, columns=None):
    """(case, Result) of a named case, computed once per session and shared by the host and the GPU tests."""
    case = CASES[name]()
    return case, evaluate(model_of(case), case["times"], case["nodes"], case["T"], recursive=case["recursive"], columns=columns)


def oracle_model(orc, case):
    expo = case["kind"] == "exponential"
    return orc.ContModel(case["lam0"], case["W"], theta=case["theta"] if expo else None, mu=None if expo else case["mu"],
                         tau=None if expo else case["tau"], dt_max=case["dt_max"], A=case["A"], grid_x=case["grid_x"])


def process_of(nhp, case):
    """The package's process for a case's arrays (copies)."""
    N = case["N"]
    if case["grid_x"] is not None:
        baseline = nhp.LogGaussianCoxProcess(case["grid_x"].copy(), [row.copy() for row in case["lam0"]])
    else:
        baseline = nhp.HomogeneousProcess(case["lam0"].copy())
    if case["kind"] == "exponential":
        impulses = nhp.ExponentialImpulseResponse(case["theta"].copy(), 1.0, 1.0, case["dt_max"])
    else:
        impulses = nhp.LogitNormalImpulseResponse(case["mu"].copy(), case["tau"].copy(), case["dt_max"])
    weights = nhp.DenseWeightModel(case["W"].copy())
    if case["A"] is not None:
        return nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, case["A"].copy(), nhp.BernoulliNetworkModel(0.5, N))
    return nhp.ContinuousStandardHawkesProcess(baseline, impulses, weights)
