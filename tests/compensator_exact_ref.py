"""Extended-precision restatement of the compensator (nhp_cont_compensator) and of the intensity at arbitrary times
(nhp_cont_intensity), written from the definition in include/nhp.h and the header of csrc/cont_compensator.hip, not from the
kernel bodies and not through tests/compensator_ref.py:

    Λ_c(t) = base_c(t) + Σ_{i: t_i < t} W[n_i,c]·A[n_i,c]·H_{n_i,c}(t - t_i)
    H(d)   = 1 - exp(-θ·min(d, Δtmax))                                      exponential (cut, not renormalised)
    H(d)   = Δtmax·Φ(√τ (logit(d/Δtmax) - μ)) for d < Δtmax, else Δtmax     logit-normal (pdf not divided by Δtmax)
    base   = λ0_c·t, or the exact integral of the piecewise-linear interpolant of (grid_x, λ_c) from grid_x[0]

Conventions (those of tests/cont_grad_ref.py).  The threshold thr = fl(t - Δtmax) and the delay d = fl(t - t_i) are taken in
float64, as the data layout takes them.  Event i is inside the window of t when t_i > thr and t_i < t: tied events are not
each other's parents.  An event with t_i <= thr has saturated: it contributes V[p,c] = W·A·H(Δtmax) whatever its age.  The
saturated events enter as (exact per-node count)·V, which keeps the restatement O(pairs + M·N).  The logit-normal takes
x = fl(d/Δtmax).  H(Δtmax) equals the saturated value by construction, so moving the border consistently changes nothing;
what can go wrong is an event on the border counted by neither side or by both, and the first two mutants below do that.

    at_events[k] = Λ_{n_k}(t_k);  residuals[k] = at_events[k] - at_events[previous event of n_k] (a node's first residual
    equals its Λ);  total[c] = Λ_c(T).

Next to every value stand the ingredients of a rounding bound.  All terms are non-negative, so

    bound = 2⁻⁵³·(R + d·S) + tiny                    first order and worst case; derived, not measured

S   the sum of the value's terms: base, saturated masses, window terms.
d   the longest chain of additions that reaches the value, read off the kernel's scheme (COMP_CHUNK = 128 events per chunk,
    COMP_GROUP = 64 chunks per group, COMP_LANES = 8 lanes per child, NHP_BLOCK = 256).  With ws the window start of the value
    (ws_k for an event, the first event inside (T - Δtmax, T] for total), j = ws // 128 its chunk and end = k or M:
        prefix   min(ws, 128) + min(j, 63) + j // 64 + 2    chunk sum, group scan, super scan, G + D, prefix + walk; 0 if ws = 0
        events   prefix + ceil((ws % 128 + k - ws) / 8) + 3 + 1      the 8 lanes' strided walk from the chunk's start, the
                                                                     butterfly, the base
        total    prefix + ceil((ws % 128 + M - ws) / 256) + 6 + 4 + 1    the block's strided walk, the wave sum, the block sum
    Δtmax = ∞ has no prefix: ws = 0.
R   Σ |term|·ρ_term, ρ_term the roundings of the term's own arithmetic, in units of 2⁻⁵³:
        base            1 (λ0·t); a grid baseline G + 12: three roundings a trapezoid and up to G - 1 additions for the whole
                        cells, the interpolant (a convex combination: 5), the last trapezoid (3) and its addition
        saturated       exponential 3 + a_expm1 (W·A, θ·Δtmax whose error H amplifies by x e^{-x}/(1 - e^{-x}) <= 1, the product);
                        logit-normal 2 (W·A, the product with Δtmax)
        window, exp     4 + a_expm1 (the delay, θ·d, W·A, the product)
        window, logit   4 + a_erfc·max(1, z²/2 for z < 0) (the delay, 0.5·erfc·Δtmax, W·A, the product; √τ and the scalings are in
                        |δz|; the library's erfc(x) loses relative accuracy in proportion to x² = z²/2 in its tail, as any
                        evaluation through e^{-x²} with a rounded x² does -- harmless, the tail is small -- so its error is
                        measured and allowed relative to that), and the
                        argument amplification absolutely: W·A·Δtmax·φ(z)·|δz| with
                        |δz| = √τ·(a_logit·(|ℓ| + 2) + |ℓ - μ|) + 4|z|: the error of ℓ = log(x/(1-x)) as measured, the
                        subtraction, then √τ, its product, the constant 1/√2 and its product relative to z
    a_expm1, a_logit, a_erfc: the allowances of the device library's three functions, twice the largest error measured on an
    MI355X through nhp_probe_math ops 9, 10, 11 (tests/test_compensator_edges_gpu.py records the measurements): -expm1(-x)
    and 0.5·erfc(-z/√2) relative to the value (times max(1, z²/2) for z < 0), log(x/(1-x)) relative to |ℓ| + 2 -- the quotient's two roundings are absolute in
    ℓ, so the expression has no relative accuracy where ℓ -> 0 (x near 1/2) and needs none: Φ is sensitive to z absolutely.
tiny  2⁻¹⁰⁰⁰ per term: below 2⁻¹⁰²² a double has no relative precision (Φ(z) for z < -37.5 is subnormal or 0), and the
      allowances are measured down to values of 2⁻¹⁰⁰⁰.
A residual's bound is the sum of its two values' bounds plus 2⁻⁵³·|residual|.  Values without a term (S = 0) are exact zeros.

real=np.float64 gives the double evaluation of the same sums (Φ as 0.5·erfc(-z/√2) from scipy), `order` (forward, reverse,
shuffled) the order of the terms.  mutate= applies exactly one mistake to it:
    le_dtmax          `<=` for `<` at Δtmax on the saturated side only: an event counts as saturated when Δtmax < d, so the one
                      at exactly Δtmax is in neither part (dropped)
    ge_window         `>=` for `>` at the window start on the window's side only: the event at exactly Δtmax is walked AND
                      counted (doubled)
    no_group_prefix   the exclusive prefix inside the group of chunks is dropped: S_c(ws) loses the events between the
                      group's start and the chunk's start
    one_minus_exp     1 - exp(-x) for -expm1(-x)

intensity_at: λ_c(q) = base_c(q) + Σ_j W·A·ħ(fl(q - t_j)) over fl(q - Δtmax) < t_j < q, both strict; ħ as in cont_grad_ref
(the logit-normal at x = fl(d·fl(1/Δtmax)), counted for 0 < x < 1); the baseline interpolated as cont_grad_ref.grid_weights
does.  Bound, the gradient reference's for λ_i: 2⁻⁵³·((K + 8)·S + 4·Σ term·amp) + U + tiny, K the number of parents, amp =
θΔ or |z|√τ(|ℓ| + 4 + |ℓ-μ|) + 3z², U the terms whose exponential a float64 evaluation flushes (θΔ or z²/2 above 708).

Everything is evaluated in numpy's long double where that is wider than double, otherwise in mpmath numbers of 40 digits
(tests/adjacency_ref.backend); Φ comes from mpmath.ncdf in both cases.  Test code only."""
import collections
import functools
import math

import numpy as np

import adjacency_ref as ar
import cont_grad_ref as gr
from adjacency_ref import backend

EPS = 2.0 ** -53
TINY = 2.0 ** -1000
FLUSH = 708.0
COMP_CHUNK, COMP_GROUP, COMP_LANES, NHP_BLOCK = 128, 64, 8, 256
# units of 2⁻⁵³ (one ulp is two): twice the largest error measured on an MI355X, tests/test_compensator_edges_gpu.py
A_EXPM1, A_LOGIT, A_ERFC = 3.0, 2.0, 8.0
MUTANTS = ("le_dtmax", "ge_window", "no_group_prefix", "one_minus_exp")

Part = collections.namedtuple("Part", "value S R d n bound")
"""value in the evaluation's number type; S, R, d, n (number of terms), bound float64."""
Result = collections.namedtuple("Result", "at_events residuals total ws")


# ---------------------------------------------------------------------------------------------------------------- numbers
def _to_mp(mp, v):
    if isinstance(v, mp.mpf):
        return v
    hi = float(v)
    if not math.isfinite(hi):
        return mp.mpf(hi)
    return mp.mpf(hi) + mp.mpf(float(v - type(v)(hi)))


class _Math:
    def __init__(self, real):
        self.b = backend(real)
        self.mpb = isinstance(self.b, ar._Mpmath)
        self.double = not self.mpb and self.b.real is np.float64

    def expm1neg(self, x, naive=False):
        """-expm1(-x) = 1 - e^{-x}"""
        if self.mpb:
            mp = self.b.mp
            return np.frompyfunc(lambda v: -mp.expm1(-v), 1, 1)(x)
        if naive:
            return self.b.num(1.0) - np.exp(-x)
        return -np.expm1(-x)

    def ncdf(self, z):
        if self.double:
            from scipy.special import erfc
            return 0.5 * erfc(-0.7071067811865476 * z)
        import mpmath
        mpmath.mp.dps = max(mpmath.mp.dps, ar.MP_DIGITS)
        if self.mpb:
            return np.frompyfunc(lambda v: mpmath.ncdf(v), 1, 1)(z)
        # every distinct argument once: on a dyadic grid of times many pairs of a link share their delay
        uniq, inverse = np.unique(np.asarray(z, dtype=self.b.real), return_inverse=True)
        out = np.empty(len(uniq), dtype=self.b.real)
        for i, v in enumerate(uniq):
            r = mpmath.ncdf(_to_mp(mpmath, v))
            hi = float(r)
            out[i] = self.b.real(hi) + self.b.real(float(r - mpmath.mpf(hi)))
        return out[inverse]


def erfc_scale(z):
    """What the relative error of 0.5·erfc(-z/√2) is measured against: 1, and z²/2 for z < -√2 -- see the module docstring."""
    z = np.asarray(z, dtype=np.float64)
    return np.where(z < 0, np.maximum(1.0, 0.5 * z * z), 1.0)


def _f(v):
    return np.asarray(v, dtype=np.float64)


def _segsum(b, v, slot, nseg, ext=True):
    """Σ of v by slot (slot ascending), in the order given."""
    out = b.zeros(nseg) if ext else np.zeros(nseg)
    if len(v):
        starts = np.searchsorted(slot, np.arange(nseg), side="left")
        full = np.searchsorted(slot, np.arange(nseg), side="right") > starts
        if full.any():
            out[full] = np.add.reduceat(v, starts[full])
    return out


def _reorder(slot, order, rng):
    """A permutation of the terms that keeps slot ascending: forward, reverse or shuffled inside every slot."""
    n = len(slot)
    if order == "forward" or n == 0:
        return np.arange(n)
    key = np.arange(n)[::-1] if order == "reverse" else rng.permutation(n)
    return np.lexsort((key, slot))


# --------------------------------------------------------------------------------------------------------------- baseline
def _base_integral(b, m, c, t):
    """(∫ of the baseline of node c from 0 (grid_x[0]) to the float64 times t, ρ)."""
    if m.grid_x is None:
        return b.num(m.lam0[c]) * b.arr(t), 1.0
    gx, y = m.grid_x, b.arr(m.lam0[c])
    G = len(gx)
    x = b.arr(gx)
    two = b.num(2.0)
    cells = (x[1:] - x[:-1]) * (y[1:] + y[:-1]) / two
    cum = b.zeros(G)
    for g in range(1, G):
        cum[g] = cum[g - 1] + cells[g - 1]
    g = np.clip(np.searchsorted(gx, t, side="right") - 1, 0, G - 2)
    tt = b.arr(t)
    h = tt - x[g]
    yt = (y[g + 1] * h + y[g] * (x[g + 1] - tt)) / (x[g + 1] - x[g])
    return cum[g] + h * (y[g] + yt) / two, G + 12.0


# ------------------------------------------------------------------------------------------------------------ compensator
def _column(M_, b, m, t, n0, cum, c, tq, end, order, mutate, rng):
    """Λ_c at the float64 times tq, over the events [0, end) (end per time): a Part without its bound, and ws."""
    N, dt_max = m.N, m.dt_max
    expo = m.theta is not None
    finite = np.isfinite(dt_max)
    A = np.ones((N, N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    WA = A[:, c] * m.W[:, c]
    nq = len(tq)
    thr = tq - dt_max
    ws = np.minimum(np.searchsorted(t, thr, side="right"), end)
    ws_cnt = np.minimum(np.searchsorted(t, thr, side="left"), end) if mutate == "le_dtmax" else ws
    ws_win = np.minimum(np.searchsorted(t, thr, side="left"), end) if mutate == "ge_window" else ws
    # ---- saturated masses
    one = b.num(1.0)
    if expo:
        V = b.arr(WA) * M_.expm1neg(b.arr(m.theta[:, c]) * b.num(dt_max), naive=mutate == "one_minus_exp") if finite else b.arr(WA)
        rho_sat = 3.0 + A_EXPM1
    else:
        V = b.arr(WA) * b.num(dt_max)
        rho_sat = 2.0
    cnt = cum[ws_cnt].astype(np.float64)                                  # [nq, N], exact
    if mutate == "no_group_prefix":
        j = ws_cnt // COMP_CHUNK
        cnt = cnt - (cum[j * COMP_CHUNK] - cum[j // COMP_GROUP * COMP_GROUP * COMP_CHUNK])
    cols = np.arange(N)
    if order == "reverse":
        cols = cols[::-1]
    elif order == "shuffled":
        cols = rng.permutation(N)
    sat = b.zeros(nq)
    for p in cols:
        if WA[p] != 0.0:
            sat = sat + b.arr(cnt[:, p]) * V[p]
    V64 = _f(V)
    S_sat = cnt @ V64
    n_sat = cnt @ (WA != 0.0).astype(np.float64)
    # ---- window terms
    num = end - ws_win
    slot = np.repeat(np.arange(nq), num)
    i = np.arange(int(num.sum())) - np.repeat(np.cumsum(num) - num, num) + np.repeat(ws_win, num)
    keep = (t[i] < tq[slot]) & (WA[n0[i]] != 0.0)
    slot, i = slot[keep], i[keep]
    q = _reorder(slot, order, rng)
    slot, i = slot[q], i[q]
    p = n0[i]
    d64 = tq[slot] - t[i]
    w = b.arr(WA[p])
    extra = np.zeros(len(i))
    if expo:
        x = b.arr(m.theta[p, c]) * b.arr(np.minimum(d64, dt_max))
        H = M_.expm1neg(x, naive=mutate == "one_minus_exp")
        rho = np.full(len(i), 4.0 + A_EXPM1)
    else:
        inside = d64 < dt_max
        x64 = np.where(inside, d64, 0.5 * dt_max) / dt_max
        inside &= x64 < 1.0
        x64 = np.where(inside, x64, 0.5)
        xx = b.arr(x64)
        ell = b.log(xx / (one - xx))
        mu, st = b.arr(m.mu[p, c]), b.sqrt(b.arr(m.tau[p, c]))
        z = st * (ell - mu)
        H = b.num(dt_max) * M_.ncdf(z)
        if (~inside).any():
            H[~inside] = b.zeros(int((~inside).sum())) + b.num(dt_max)
        z64, st64, l64 = _f(z), np.sqrt(m.tau[p, c]), _f(ell)
        dz = st64 * (A_LOGIT * (np.abs(l64) + 2.0) + np.abs(l64 - m.mu[p, c])) + 4.0 * np.abs(z64)
        phi = np.exp(-0.5 * z64 * z64) / math.sqrt(2.0 * math.pi)
        extra = np.where(inside, WA[p] * dt_max * phi * dz, 0.0)
        rho = np.where(inside, 4.0 + A_ERFC * erfc_scale(z64), 3.0)
    term = w * H
    t64 = _f(term)
    win = _segsum(b, term, slot, nq)
    base, rho_base = _base_integral(b, m, c, tq)
    base64 = _f(base)
    if order == "forward":
        value = (base + sat) + win
    else:
        value = (win + sat) + base
    S = base64 + S_sat + _segsum(b, t64, slot, nq, ext=False)
    R = base64 * rho_base + S_sat * rho_sat + _segsum(b, t64 * rho + extra, slot, nq, ext=False)
    n = (base64 > 0) + n_sat + np.bincount(slot, minlength=nq)
    return value, S, R, n, ws


def _depth(ws, end, block, finite):
    j = ws // COMP_CHUNK
    prefix = np.where(ws > 0, np.minimum(ws, COMP_CHUNK) + np.minimum(j, COMP_GROUP - 1) + j // COMP_GROUP + 2, 0) if finite else 0
    walk = np.ceil((ws % COMP_CHUNK + end - ws) / block)
    return prefix + walk + (3 + 1 if block == COMP_LANES else 6 + 4 + 1)


def _bound(S, R, d, n):
    return np.where(n > 0, EPS * (R + d * S) + TINY * n, 0.0)


def evaluate(m, times, nodes, T, real=None, order="forward", mutate=None, parts=("events", "total"), seed=0):
    """Result(at_events, residuals, total: Parts; ws [M] the window starts).  parts: what to compute (the rest is None)."""
    assert order in ("forward", "reverse", "shuffled") and (mutate is None or (mutate in MUTANTS and real is np.float64))
    M_ = _Math(real)
    b = M_.b
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    M, N = len(t), m.N
    assert np.all(np.diff(t) >= 0) and (M == 0 or t[0] >= 0.0) and np.all(m.W >= 0)
    rng = np.random.default_rng(seed)
    cum = np.zeros((M + 1, N), dtype=np.int64)
    cum[1:] = np.cumsum(n0[:, None] == np.arange(N)[None, :], axis=0)
    finite = np.isfinite(m.dt_max)
    at = res = tot = None
    ws_all = np.zeros(M, dtype=np.int64)
    if "events" in parts:
        value, S, R, d, n = b.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
        rvalue, rB = b.zeros(M), np.zeros(M)
        prev = np.full(M, -1)
        for c in range(N):
            ev = np.nonzero(n0 == c)[0]
            if len(ev) == 0:
                continue
            v, S[ev], R[ev], n[ev], ws = _column(M_, b, m, t, n0, cum, c, t[ev], ev, order, mutate, rng)
            value[ev] = v
            ws_all[ev] = ws
            d[ev] = _depth(ws, ev, COMP_LANES, finite)
            prev[ev[1:]] = ev[:-1]
        B = _bound(S, R, d, n)
        first = prev < 0
        rvalue[first] = value[first]
        rvalue[~first] = value[~first] - value[prev[~first]]
        rB[first] = B[first]
        rB[~first] = B[~first] + B[prev[~first]] + EPS * np.abs(_f(rvalue[~first]))
        rS = np.where(first, S, S + S[prev])
        rB = np.where(rS > 0, rB, 0.0)
        at = Part(value, S, R, d, n, B)
        res = Part(rvalue, rS, np.where(first, R, R + R[prev]), d, np.where(first, n, n + n[prev]), rB)
    if "total" in parts:
        value, S, R, d, n = b.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
        for c in range(N):
            v, S[c:c + 1], R[c:c + 1], n[c:c + 1], ws = _column(M_, b, m, t, n0, cum, c, np.array([float(T)]), np.array([M]), order,
                                                                mutate, rng)
            value[c] = v[0]
            d[c] = _depth(ws, np.array([M]), NHP_BLOCK, finite)[0]
        tot = Part(value, S, R, d, n, _bound(S, R, d, n))
    return Result(at, res, tot, ws_all)


def check(got, part, extra=0.0):
    """(largest error/bound, indices outside the bound -- or, where the bound is 0, not exactly 0 --, err, B).  No entry is
    skipped.  extra: added to every non-zero bound (an allowance of the implementation compared, in units of 2⁻⁵³·S)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == part.S.shape, (got.shape, part.S.shape)
    B = np.where(part.bound > 0, part.bound + EPS * extra * part.S, 0.0)
    err = np.abs(np.asarray(got - part.value, dtype=np.float64))
    data = B > 0
    ratio = np.zeros(len(got))
    ratio[data] = err[data] / B[data]
    bad = np.nonzero(np.where(data, ~(err <= B), got != 0.0))[0]
    return (float(ratio.max()) if data.any() else 0.0), bad, err, B


def explain(got, part, bad, err, B, limit=6):
    worst = sorted(bad, key=lambda k: -(err[k] / B[k] if B[k] > 0 else np.inf))[:limit]
    return "\n".join(f"[{k}] got {float(got[k])!r} want {float(part.value[k])!r} S {part.S[k]:.3g} d {part.d[k]:.0f} n {part.n[k]:.0f} "
                     f"error/bound {err[k] / B[k] if B[k] > 0 else float('inf'):.3g}" for k in worst)


# -------------------------------------------------------------------------------------------------------------- intensity
Lam = collections.namedtuple("Lam", "value S K bound Qd")
"""Qd: Σ |∂term/∂Δ| = Σ θ·term (exponential; 0 for the logit-normal routes, which read exact delays), for record formats that
round the delay (cont_grad_ref: δ)."""


def _lambda_terms(b, m, WA, p, c, d64):
    """The terms W·A·ħ of λ_c for parents on nodes p at the float64 delays d64: (terms, the same in float64, amp, flushed)."""
    one, two = b.num(1.0), b.num(2.0)
    if m.theta is not None:
        th64 = m.theta[p, c]
        th = b.arr(th64)
        hbar = th * b.exp(-(th * b.arr(d64)))
        amp = th64 * d64
        flushed = amp > FLUSH
    else:
        x64 = d64 * (1.0 / m.dt_max)
        live = (x64 > 0.0) & (x64 < 1.0)
        x = b.arr(np.where(live, x64, 0.5))
        mu, tau = b.arr(m.mu[p, c]), b.arr(m.tau[p, c])
        ell = b.log(x / (one - x))
        dl = ell - mu
        z2 = tau * dl * dl
        hbar = b.exp(-z2 / two) * b.sqrt(tau / (two * b.pi())) / (x * (one - x))
        if (~live).any():
            hbar[~live] = b.zeros(int((~live).sum()))
        z = np.sqrt(_f(z2))
        amp = z * np.sqrt(m.tau[p, c]) * (np.abs(_f(ell)) + 4.0 + np.abs(_f(dl))) + 3.0 * _f(z2)
        flushed = _f(z2) / 2.0 > FLUSH
    term = b.arr(WA[p, c]) * hbar
    return term, _f(term), amp, flushed


def _baseline_at(b, m, c, q):
    if m.grid_x is None:
        return b.zeros(len(q)) + b.num(m.lam0[c])
    y = b.arr(m.lam0[c])
    ga, w_lo, w_hi, last = gr.grid_weights(b, m.grid_x, q)
    base = y[ga + 1] * w_hi + y[ga] * w_lo
    if last.any():
        base[last] = y[len(m.grid_x) - 1]
    return base


def intensity_at(m, times, nodes, q, real=None):
    """Lam(value [Q, N] in the evaluation's number type; S, K [Q], bound [Q, N] float64)."""
    b = backend(real)
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    Q, N = len(q), m.N
    expo = m.theta is not None
    A = np.ones((N, N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    WA = A * m.W
    jb = np.searchsorted(t, q - m.dt_max, side="right")
    je = np.maximum(np.searchsorted(t, q, side="left"), jb)
    K = (je - jb).astype(np.float64)
    slot = np.repeat(np.arange(Q), je - jb)
    j = np.arange(int(K.sum())) - np.repeat(np.cumsum(je - jb) - (je - jb), je - jb) + np.repeat(jb, je - jb)
    p = n0[j]
    d64 = q[slot] - t[j]
    value, S, amps, U = b.zeros((Q, N)), np.zeros((Q, N)), np.zeros((Q, N)), np.zeros((Q, N))
    for c in range(N):
        base = _baseline_at(b, m, c, q)
        term, t64, amp, flushed = _lambda_terms(b, m, WA, p, c, d64)
        value[:, c] = base + _segsum(b, term, slot, Q)
        S[:, c] = _f(base) + _segsum(b, t64, slot, Q, ext=False)
        amps[:, c] = _segsum(b, t64 * np.where(flushed, 0.0, amp), slot, Q, ext=False)
        U[:, c] = _segsum(b, np.where(flushed, t64, 0.0), slot, Q, ext=False)
    bound = EPS * ((K[:, None] + 8.0) * S + 4.0 * amps) + U + TINY * (K[:, None] + 1.0)
    return Lam(value, S, K, bound, np.zeros((Q, N)))


def event_intensity(m, times, nodes, real=None):
    """λ_{n_i}(t_i) at every event in the conventions of total_intensity and the log-likelihood (cont_grad_ref: event j < i is a
    parent when t_j > fl(t_i - Δtmax); a tie is a pair, which the exponential counts at ħ = θ and the logit-normal, x = 0, does
    not): Lam with value, S, K, bound [M], the bound of intensity_at."""
    b = backend(real)
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    M, N = len(t), m.N
    A = np.ones((N, N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    WA = A * m.W
    value, S, K, amps, U, Qd = b.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
    for c in range(N):
        ev, slot, j = gr.column_pairs(t, n0, c, m.dt_max, False)
        if len(ev) == 0:
            continue
        term, t64, amp, flushed = _lambda_terms(b, m, WA, n0[j], c, t[ev][slot] - t[j])
        base = _baseline_at(b, m, c, t[ev])
        value[ev] = base + _segsum(b, term, slot, len(ev))
        S[ev] = _f(base) + _segsum(b, t64, slot, len(ev), ext=False)
        K[ev] = np.bincount(slot, minlength=len(ev))
        amps[ev] = _segsum(b, t64 * np.where(flushed, 0.0, amp), slot, len(ev), ext=False)
        U[ev] = _segsum(b, np.where(flushed, t64, 0.0), slot, len(ev), ext=False)
        if m.theta is not None:
            Qd[ev] = _segsum(b, t64 * m.theta[n0[j], c], slot, len(ev), ext=False)
    return Lam(value, S, K, EPS * ((K + 8.0) * S + 4.0 * amps) + U + TINY * (K + 1.0), Qd)


def check_intensity(got, lam, delta=0.0):
    """(largest error/bound, (query, child) pairs outside the bound).  Every entry is compared; every bound is positive.
    delta: the delay step of the record format under test, δ·Qd is added (0 for exact records)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == lam.bound.shape, (got.shape, lam.bound.shape)
    err = np.abs(np.asarray(got - lam.value, dtype=np.float64))
    B = lam.bound + delta * lam.Qd
    assert np.all(B > 0)
    bad = np.argwhere(~(err <= B))
    return (float((err / B).max()) if err.size else 0.0), bad


# ------------------------------------------------------------------------------------------------------------------ cases
def prefix_case(M):
    """P-M: N = 3, Δtmax = 1, times on the dyadic grid 2⁻⁶ at about 3 events per unit (ties, Δ = Δtmax, empty windows), the
    first event at t = 0 (Λ = 0: a value without a term), node 3 empty.  Logit-normal for M = 128 and 8193."""
    rng = np.random.default_rng(1000 + M)
    N = 3
    t = np.sort(rng.integers(0, max(M // 3, 2) * 64, M)) / 64.0
    t[0] = 0.0
    nodes = rng.integers(1, 3, M).astype(np.int64)
    kind = "logitnormal" if M in (128, 8193) else "exponential"
    return dict(N=N, T=float(t[-1] + 0.25), times=t, nodes=nodes, kind=kind, dt_max=1.0, lam0=rng.uniform(0.5, 1.5, N),
                W=rng.uniform(0.05, 0.6, (N, N)), theta=rng.uniform(0.5, 8.0, (N, N)), mu=rng.normal(0.0, 1.0, (N, N)),
                tau=rng.uniform(0.5, 2.0, (N, N)), A=None, grid_x=None, recursive=False)


def tiny_case():
    """S-tiny: N = 2, λ0 = 1e-12, 200 events inside 2⁻¹⁰ after t = 1 (steps of 2⁻³⁰), θ near 1: Λ is a sum of terms of size
    θ·Δ <= 1e-3, where 1 - exp(-x) has lost 10 of its bits."""
    rng = np.random.default_rng(77)
    t = 1.0 + np.sort(rng.choice(np.arange(1, 2 ** 20), 200, replace=False)) * 2.0 ** -30
    nodes = rng.integers(1, 3, 200).astype(np.int64)
    return dict(N=2, T=1.0 + 2.0 ** -9, times=t, nodes=nodes, kind="exponential", dt_max=1.0, lam0=np.full(2, 1e-12),
                W=rng.uniform(0.3, 1.0, (2, 2)), theta=rng.uniform(0.9, 1.1, (2, 2)), mu=None, tau=None, A=None, grid_x=None,
                recursive=False)


def wide_case(N):
    """N-70 (logit-normal, network) and N-300 (exponential), M = 1500, T = 100, Δtmax = 1: for the intensity only -- several
    transpose tiles of 32, a ragged last tile, and with N = 300 > NHP_BLOCK a second pass of the child loop."""
    rng = np.random.default_rng(2000 + N)
    M, T = 1500, 100.0
    t = np.sort(rng.integers(1, int(T * 1024), M)) / 1024.0
    t[100:110:2] = t[101:111:2]
    t = np.sort(t)
    nodes = rng.integers(1, N + 1, M).astype(np.int64)
    nodes[nodes == 2] = 1
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64) if N == 70 else None
    return dict(N=N, T=T, times=t, nodes=nodes, kind="logitnormal" if N == 70 else "exponential", dt_max=1.0,
                lam0=rng.uniform(0.5, 1.5, N), W=rng.uniform(0.0, 1.0, (N, N)) / N * 2.0, theta=rng.uniform(0.5, 40.0, (N, N)),
                mu=rng.normal(0.0, 1.0, (N, N)), tau=rng.uniform(0.5, 2.0, (N, N)), A=A, grid_x=None, recursive=False)


def _long(kind, dt_max=None):
    case = gr.long_case(kind)
    case["times"], case["nodes"] = case["times"][:300].copy(), case["nodes"][:300].copy()
    if dt_max is not None:
        case["dt_max"] = dt_max
    return case


GRAD_CASES = ("W-exp", "W-logit", "W-net", "W-net-logit", "G-W")
CASES = {name: gr.CASES[name] for name in GRAD_CASES}
CASES.update({"L-exp": lambda: _long("exponential"), "L-logit": lambda: _long("logitnormal"),
              "L-exp-inf": lambda: _long("exponential", np.inf), "S-tiny": tiny_case})
P_SIZES = (127, 128, 129, 8191, 8192, 8193)
CASES.update({"P-%d" % M: (lambda M=M: prefix_case(M)) for M in P_SIZES})
COMPENSATOR_CASES = tuple(CASES)
FAR = ("W-exp", "W-logit", "W-net", "W-net-logit", "L-exp", "L-logit", "S-tiny", "P-129", "P-8193")
"""Run also with T = t_last + 2·Δtmax: no event inside the last window (G-W cannot: its grid ends at T)."""
CASES.update({"N-70": lambda: wide_case(70), "N-300": lambda: wide_case(300)})
TIME_PART_CASES = ("P4-exp", "P4-logit", "P2-inf")
"""cont_grad_ref's cases that the default rule lays out in XCD time parts (tests/test_time_parts_gpu.py); P2-inf: Δtmax = ∞."""
CASES.update({name: gr.CASES[name] for name in TIME_PART_CASES})
INTENSITY_CASES = GRAD_CASES + ("L-exp", "L-logit", "S-tiny", "N-70", "N-300")


@functools.lru_cache(maxsize=None)
def case_of(name):
    return CASES[name]()


def far_T(case):
    return float(case["times"][-1] + 2.0 * case["dt_max"])


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, Result) of a named case, computed once per session and shared by the host and the GPU tests."""
    case = case_of(name)
    return case, evaluate(gr.model_of(case), case["times"], case["nodes"], case["T"])


@functools.lru_cache(maxsize=None)
def prepared_far(name):
    """The Part of total with T pushed to t_last + 2·Δtmax; at_events and residuals do not depend on T."""
    case = case_of(name)
    return evaluate(gr.model_of(case), case["times"], case["nodes"], far_T(case), parts=("total",)).total


def query_times(case):
    """0 and a time before the first event, every tied time, t_j and t_j + Δtmax with the neighbouring doubles of both for a
    dozen j, points inside the densest stretch, every grid point, T, and T + 5 under a homogeneous baseline."""
    t, T, dt_max = case["times"], case["T"], case["dt_max"]
    q = [0.0, T]
    if t[0] > 0:
        q.append(0.5 * t[0])
    u, cnt = np.unique(t, return_counts=True)
    q.extend(u[cnt > 1][:40])
    for j in np.linspace(0, len(t) - 1, 12).astype(int):
        for v in (t[j], t[j] + dt_max):
            q.extend([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])
    k = int(np.argmax(np.arange(len(t)) - np.searchsorted(t, t - dt_max, side="right")))      # the longest window ends here
    q.extend(0.5 * (t[max(k - 5, 0):k] + t[max(k - 4, 1):k + 1]))
    if case["grid_x"] is not None:
        q.extend(case["grid_x"])
    else:
        q.append(T + 5.0)
    q = np.array(q, dtype=np.float64)
    q = q[(q >= 0.0) & np.isfinite(q)]
    if case["grid_x"] is not None:
        q = q[q <= case["grid_x"][-1]]
    return np.sort(q)


@functools.lru_cache(maxsize=None)
def prepared_events(name):
    case = case_of(name)
    return case, event_intensity(gr.model_of(case), case["times"], case["nodes"])


@functools.lru_cache(maxsize=None)
def prepared_intensity(name):
    case = case_of(name)
    q = query_times(case)
    return case, q, intensity_at(gr.model_of(case), case["times"], case["nodes"], q)
