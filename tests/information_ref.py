"""Extended-precision restatement of the observed information of the continuous log-likelihood, block by block, written from
the formulas below and the pair conventions of tests/cont_grad_ref.py (column_pairs: which event is a parent of which), not
from the kernels.  The objective separates by child node c; over the D = 1 + kinds·N parameters of column c,
[λ0[c]; θ[:,c] | μ[:,c]; τ[:,c]; W[:,c]] (row 0 λ0, row 1 + q·N + p impulse kind q of parent p, row 1 + (kinds-1)·N + p W[p,c]),
with g_i = 1/λ_i, a = A[p,c], w = W[p,c] and u_i = ∂λ_i/∂(column parameters):

    J_c = -H_c = Σ_{i on c} g_i²·u_i u_iᵀ - Σ_{i on c} g_i·∇²λ_i
    u_i[λ0] = 1        u_i[W[p]] = a Σ_{j∈p} ħ_ij        u_i[q[p]] = a·w Σ_{j∈p} ∂_qħ_ij
    ∇²λ_i[W[p], q[p]] = a Σ_{j∈p} ∂_qħ_ij              ∇²λ_i[q[p], q'[p]] = a·w Σ_{j∈p} ∂²_{qq'}ħ_ij          (0 elsewhere)
    exponential   ħ = θe^{-θΔ}:  ∂_θħ = (1 - θΔ)e^{-θΔ},  ∂²_θθħ = -Δ(2 - θΔ)e^{-θΔ}
    logit-normal  δ = ℓ - μ, ℓ = logit(Δ/Δtmax), counted for 0 < x < 1:   ∂_μħ = ħτδ,  ∂_τħ = ħ(1/(2τ) - δ²/2),
                  ∂²_μμħ = ħ(τ²δ² - τ),  ∂²_μτħ = ħδ(3/2 - τδ²/2),  ∂²_ττħ = ħ((1/(2τ) - δ²/2)² - 1/(2τ²))

u_i is summed by parent node first (cheap at these N); the outer products are one matrix product per column.

Next to every entry stand the ingredients of a rounding bound, sums over the entry's terms (a term: one child's product
g²·u_x·u_y, or one pair's curvature term) with the differences split into their parts: (1 - θΔ) -> 1 and θΔ, (2 - θΔ) -> 2 and
θΔ, ℓ - μ -> ℓ and μ in ∂_μħ, 1/(2τ) - δ²/2, τ²δ² - τ, 3/2 - τδ²/2 and k² - 1/(2τ²) -> the sum of their two parts:

    S     Σ |term|                      n     children that contribute a term (+ the pairs of a curvature entry)
    R     Σ |term|·ρ_term               U     Σ |term| over the terms that hold a pair whose e^{-θΔ} (e^{-z²/2}) is below the
    tiny  2⁻¹⁰⁰⁰ per contributing child       smallest double (argument beyond 708: a float64 evaluation may drop it entirely)

    bound = 2⁻⁵³·(R + (n + 8)·S) + U + tiny,        r = R/S + n + 8 in the issue's r·2⁻⁵³·S + tiny

ρ_term counts the roundings that reach one term, read off the arithmetic of csrc/cont_information.hip:
  * g_i = 1/λ_i as in cont_grad_ref: λ_i is a sum of K_i + 1 non-negative numbers, so K_i + 8 plus the mean over its own terms
    of their amplified argument error, 4·Σ_j λterm_j·amp_j/λ_i; a product term holds g_i twice (2ρ_i), a curvature term once;
  * a pair's value inside u_x: 16 (the exponential within 2 ulp = 4·2⁻⁵³; θΔ, the differences, up to five products with θ, Δ,
    τ, δ, 1/(2τ); the scale a·w) + 4·amp + K_i (its sum by parent node, LDS adds in any order), amp = θΔ for the exponential
    and |z|√τ(|ℓ| + 4 + |δ|) + 3z², z = √τδ, for the logit-normal exponent; besides, absolutely, the error of δ itself
    (|ℓ| + 4 + |δ| units: four argument roundings of the logarithm, its own, the subtraction) through the factor's derivative
    in δ: τ for ∂_μ, δ for ∂_τ, 2τ²δ for ∂²_μμ, |3/2 - 3τδ²/2| for ∂²_μτ, 2|k|δ for ∂²_ττ, times ħ and the scale;
  * 8 for the two scalings by g, the product and the entry's place in the tile.
(n + 8): the sum of the entry's terms in any order (LDS adds across the children of an item, one global add per item and
tile), the subtraction of the curvature sum and its scaling by a or a·w.  The kernels read exact delays (16-byte records), so
there is no quantisation term.  `far` pairs (θΔ > 1416) stay out of the sums as in cont_grad_ref; they count for `tiny`.
Entries whose bound is 0 have no term at all and must be exact zeros.  The truncated window of the recursive objective drops
less than 2⁻⁶⁰·λ_i per child: window_tail.  First order and worst case; derived, not measured.

Everything is evaluated in numpy's long double where that is the x87 80-bit format or wider, otherwise in mpmath numbers
(tests/adjacency_ref.backend); real=np.float64 gives the plain double evaluation of the same sums, `order` the order in
which the pairs and the children enter them.  Test code only."""
import collections
import functools

import numpy as np

import cont_grad_ref as cr
from adjacency_ref import backend
from cont_grad_ref import CASES, EPS, FLUSH, column_pairs, model_of, process_of  # noqa: F401

Result = collections.namedtuple("Result", "ll columns blocks S R U n tiny kinds")
"""blocks[k] [D, D] in the evaluation's number type (MINUS the Hessian); S, R, U, n, tiny float64 [D, D] per column."""


def big_case(seed=9):
    """B-130: N = 130, M = 3000, T = 200, Δtmax = 1, windowed exponential, built like cont_grad_ref.windowed_case: times on
    the dyadic grid 2⁻¹⁰, ties, pairs at Δ = Δtmax exactly, node 130 empty, node 129 with one event, exact zeros in W.
    D = 261: the packed triangle (273 KB) does not fit the LDS, so the automatic tiling runs."""
    rng = np.random.default_rng(seed)
    N, M, T = 130, 3000, 200.0
    t = np.sort(rng.integers(1, int(196.0 * 1024), M)) / 1024.0
    nodes = rng.integers(1, 129, M).astype(np.int64)
    t[700:730:2] = t[701:731:2]
    t[1200:1224:2] = t[1140:1164:2] + 1.0
    nodes[1600] = 129
    order = np.argsort(t, kind="stable")
    t, nodes = t[order], nodes[order]
    W = rng.uniform(0.05, 1.0, (N, N)) / N * 2.0
    W[1, 2] = W[4, 4] = W[0, 3] = 0.0
    theta = np.exp(rng.uniform(np.log(0.5), np.log(40.0), (N, N)))
    return dict(N=N, T=T, times=t, nodes=nodes, kind="exponential", dt_max=1.0, lam0=rng.uniform(0.5, 1.5, N), W=W, theta=theta,
                mu=None, tau=None, A=None, grid_x=None, recursive=False)


ALL_CASES = dict(CASES)
ALL_CASES["B-130"] = big_case


def block_index(N, kinds, c):
    """Positions in the params!-order vector [λ0; θ | μ; τ; W] of the rows of column c's block."""
    k = np.arange(kinds)[:, None] * N * N + np.arange(N)[None, :] + c * N
    return np.concatenate([[c], N + k.ravel()])


def evaluate(m, times, nodes, T, recursive=False, columns=None, real=None, order="forward", seed=0, curvature=True):
    """The blocks of `columns` (all by default).  curvature=False drops the Σ g·∇²λ term (a planted error for the tests)."""
    b = backend(real)
    f = lambda v: np.asarray(v, dtype=np.float64)
    N = m.N
    t = np.asarray(times, dtype=np.float64)
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    assert np.all(np.diff(t) >= 0) and (len(t) == 0 or t[0] >= 0.0) and m.grid_x is None
    expo = m.theta is not None
    assert expo or not recursive
    KI = 1 if expo else 2
    KK = KI + 1
    D = 1 + KK * N
    A = np.ones((N, N)) if m.A is None else np.asarray(m.A, dtype=np.float64)
    mask = A if not recursive else np.ones((N, N))
    cnt = np.bincount(n0, minlength=N).astype(np.float64)
    cols = list(range(N)) if columns is None else [int(c) for c in columns]
    rng = np.random.default_rng(seed)
    one, two = b.num(1.0), b.num(2.0)
    ll = b.num(0.0)
    out = {k: [] for k in ("blocks", "S", "R", "U", "n", "tiny")}
    for c in range(N):
        ev, slot, j = column_pairs(t, n0, c, m.dt_max, recursive)
        nch = len(ev)
        if order == "reversed":
            slot, j = slot[::-1], j[::-1]
        elif order == "permuted":
            q = rng.permutation(len(j))
            slot, j = slot[q], j[q]
        p = n0[j]
        d64 = t[ev][slot] - t[j]
        if expo:
            live_all = np.ones(len(j), dtype=bool)
        else:
            x_all = d64 * (1.0 / m.dt_max)
            live_all = (x_all > 0.0) & (x_all < 1.0)
        struct_all = np.zeros((nch, N))
        sel = live_all & (A[p, c] != 0)
        np.add.at(struct_all, (slot[sel], p[sel]), 1.0)
        if expo:
            far = m.theta[p, c] * d64 > 2.0 * FLUSH
            slot, j, p, d64 = slot[~far], j[~far], p[~far], d64[~far]
        a, w = A[p, c], m.W[p, c]
        key = slot * N + p
        by_cp, by_child, by_parent = cr._Seg(b, key, nch * N), cr._Seg(b, slot, nch), cr._Seg(b, p, N)
        base = b.zeros(nch) + b.num(m.lam0[c])
        ll = ll - b.num(m.lam0[c]) * b.num(float(T)) - (b.arr(cnt) * b.arr(m.W[:, c]) * b.arr(mask[:, c])).sum()
        d = b.arr(d64)
        # ---- per pair: ħ, its derivatives as (positive part, negative part), and their sensitivity to the error of δ
        if expo:
            th64 = m.theta[p, c]
            th = b.arr(th64)
            thd = th * d
            e = b.exp(-thd)
            hbar = th * e
            amp = th64 * d64
            flushed = amp > FLUSH
            live = np.ones(len(j), dtype=bool)
            d1 = [(e, thd * e)]
            d2 = {(0, 0): (d * thd * e, two * d * e)}                    # -Δ(2 - θΔ)e = ΔθΔe - 2Δe
            ext1, ext2 = [np.zeros(len(j))], {(0, 0): np.zeros(len(j))}
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
            i2t, hd2 = one / (two * tau), dl * dl / two
            k = i2t - hd2
            pos = lambda v: (v + abs(v)) / two
            neg = lambda v: (abs(v) - v) / two
            d1 = [(hbar * tau * (pos(ell) + neg(mu)), hbar * tau * (neg(ell) + pos(mu))), (hbar * i2t, hbar * hd2)]
            m3 = b.num(1.5) - tau * hd2
            d2 = {(0, 0): (hbar * tau * tau * dl * dl, hbar * tau),
                  (0, 1): (hbar * (pos(dl) * b.num(1.5) + neg(dl) * tau * hd2), hbar * (neg(dl) * b.num(1.5) + pos(dl) * tau * hd2)),
                  (1, 1): (hbar * k * k, hbar * two * i2t * i2t)}
            h64, t64, dl64 = f(hbar), m.tau[p, c], np.abs(f(dl))
            ext1 = [h64 * t64 * spread, h64 * dl64 * spread]
            ext2 = {(0, 0): h64 * 2.0 * t64 * t64 * dl64 * spread, (0, 1): h64 * np.abs(f(m3) - 2.0 * t64 * f(hd2)) * spread,
                    (1, 1): h64 * 2.0 * np.abs(f(k)) * dl64 * spread}
        ba, baw = b.arr(a), b.arr(a * w)
        lt = baw * hbar
        lam = base + by_child.sum(lt)
        ll = ll + (b.log(lam).sum() if nch else b.num(0.0))
        if c not in cols:
            continue
        g = one / lam
        g64 = f(g)
        K = np.bincount(slot, minlength=nch).astype(np.float64)
        rho_i = K + 8.0 + 4.0 * by_child.sum(f(lt) * np.where(flushed, 0.0, amp), real=False) / f(lam)
        rho_p = 16.0 + 4.0 * np.where(flushed, 0.0, amp) + (K[slot] if len(j) else np.zeros(0))
        # ---- u_i by parent node: value, Σ|part|, Σ|part|·ρ, flushed part
        U, Ua, Ur, Uf = b.zeros((nch, D)), np.zeros((nch, D)), np.zeros((nch, D)), np.zeros((nch, D))
        U[:, 0] = b.zeros(nch) + one
        Ua[:, 0] = 1.0

        def put(col0, plus, minus, scale, extra):
            sl = slice(col0, col0 + N)
            U[:, sl] = (by_cp.sum(scale * plus) - by_cp.sum(scale * minus)).reshape(nch, N)
            af = f(scale) * (f(plus) + f(minus))
            Ua[:, sl] = by_cp.sum(af, real=False).reshape(nch, N)
            Ur[:, sl] = by_cp.sum(af * rho_p + f(scale) * extra, real=False).reshape(nch, N)
            Uf[:, sl] = by_cp.sum(np.where(flushed, af, 0.0), real=False).reshape(nch, N)

        zero = b.zeros(len(j))
        put(1 + KI * N, hbar, zero, ba, np.zeros(len(j)))
        for q in range(KI):
            put(1 + q * N, d1[q][0], d1[q][1], baw, ext1[q])
        rows = np.arange(nch)
        if order == "reversed":
            rows = rows[::-1]
        elif order == "permuted":
            rows = rng.permutation(nch)
        g2 = g * g
        g2_64 = g64 * g64
        Uo = U[rows]
        J = Uo.T @ (Uo * g2[rows][:, None]) if nch else b.zeros((D, D))
        S = Ua.T @ (Ua * g2_64[:, None])
        R = Ua.T @ (Ua * (g2_64 * (2.0 * rho_i + 8.0))[:, None]) + Ur.T @ (Ua * g2_64[:, None]) + Ua.T @ (Ur * g2_64[:, None])
        Um = Uf.T @ (Ua * g2_64[:, None]) + Ua.T @ (Uf * g2_64[:, None])
        Z = np.zeros((nch, D))
        Z[:, 0] = 1.0
        for q in range(KK):
            Z[:, 1 + q * N:1 + (q + 1) * N] = struct_all > 0
        n = Z.T @ Z
        # ---- the curvature sums, inside one parent's own parameters
        gi = g[slot] if len(j) else b.zeros(0)
        gi64 = f(gi)
        rho_c = (rho_i[slot] if len(j) else np.zeros(0)) + rho_p
        npairs = by_parent.sum(np.ones(len(j)), real=False)
        pidx = np.arange(N)

        def curve(r0, c0, plus, minus, scale, extra):
            val = by_parent.sum(gi * scale * plus) - by_parent.sum(gi * scale * minus)
            af = gi64 * f(scale) * (f(plus) + f(minus))
            for rr, cc in ((r0, c0), (c0, r0)) if r0 != c0 else ((r0, c0),):
                if curvature:
                    J[rr + pidx, cc + pidx] = J[rr + pidx, cc + pidx] - val
                S[rr + pidx, cc + pidx] += by_parent.sum(af, real=False)
                R[rr + pidx, cc + pidx] += by_parent.sum(af * rho_c + gi64 * f(scale) * extra, real=False)
                Um[rr + pidx, cc + pidx] += by_parent.sum(np.where(flushed, af, 0.0), real=False)
                n[rr + pidx, cc + pidx] += npairs

        for q in range(KI):
            curve(1 + KI * N, 1 + q * N, d1[q][0], d1[q][1], ba, ext1[q])
        for (q, q2), (plus, minus) in d2.items():
            curve(1 + q2 * N, 1 + q * N, plus, minus, baw, ext2[(q, q2)])
        out["blocks"].append(J)
        out["S"].append(S)
        out["R"].append(R)
        out["U"].append(Um)
        out["n"].append(n)
        out["tiny"].append(2.0 ** -1000 * n)
    done = sorted(set(cols))                                            # (the loop appends in node order)
    pick = lambda k: [out[k][done.index(c)] for c in cols]
    return Result(ll=ll, columns=cols, kinds=KK, **{k: pick(k) for k in out})


def bound(res, k, tail=None):
    """The per-entry bound of block k (float64 [D, D]); tail: an array added where the entry has terms."""
    S = res.S[k]
    B = np.where(S > 0, EPS * (res.R[k] + (res.n[k] + 8.0) * S) + res.U[k], 0.0) + res.tiny[k]
    return B if tail is None else B + np.where(S > 0, tail, 0.0)


def window_tail(res, k, m, times, nodes):
    """What the truncated window may drop from block k: less than 2⁻⁶⁰·λ_i per child from λ_i (a relative 2⁻⁶⁰ of every g_i,
    twice in a product) and, from the child's own sums, at most 2⁻⁶⁰·λ_i/W[p,c] of a·Σħ, 2⁻⁶⁰·λ_i·span of a·w·Σ∂_θħ
    (|1 - θΔ|/θ <= Δ <= span where θΔ > 41) and 2⁻⁶⁰·λ_i·span² of a·w·Σ∂²_θθħ."""
    N = m.N
    c = res.columns[k]
    kids = float((np.asarray(nodes) - 1 == c).sum())
    span = float(times[-1] - times[0]) if len(times) else 0.0
    with np.errstate(divide="ignore"):
        invW = np.where(m.W[:, c] > 0, 1.0 / m.W[:, c], 0.0)
    kx = np.concatenate([[0.0], np.full(N, span), invW])
    # Σ_i g_i·|u|_iy <= sqrt(kids·S[y, y]) (Cauchy-Schwarz on Σ g²|u|² = S[y, y])
    s = np.sqrt(kids * np.diag(res.S[k]))
    tail = 2.0 ** -60 * (2.0 * res.S[k] + np.outer(kx, s) + np.outer(s, kx))
    th, Wc = 1 + np.arange(N), 1 + N + np.arange(N)
    tail[Wc, th] += 2.0 ** -60 * kids * span * invW
    tail[th, Wc] += 2.0 ** -60 * kids * span * invW
    tail[th, th] += 2.0 ** -60 * kids * span * span
    return tail


def check(got, res, k, tail=None):
    """(largest error/bound over the entries with a bound, (row, column) of the entries outside the bound or, where the bound
    is 0, different from 0, err, B) of block k.  No entry is skipped."""
    got = np.asarray(got, dtype=np.float64)
    B = bound(res, k, tail)
    err = np.abs(np.asarray(got - res.blocks[k], dtype=np.float64))
    data = B > 0
    ratio = np.zeros(got.shape)
    ratio[data] = err[data] / B[data]
    bad = np.argwhere(np.where(data, ~(err <= B), got != 0.0))
    return (float(ratio.max()) if data.any() else 0.0), bad, err, B


def explain(got, res, k, bad, err, B, limit=8):
    lines = []
    for r, q in sorted(map(tuple, bad), key=lambda rq: -(err[rq] / B[rq] if B[rq] > 0 else np.inf))[:limit]:
        lines.append(f"column {res.columns[k]} entry ({r}, {q}): got {got[r, q]!r} want {float(res.blocks[k][r, q])!r} "
                     f"S {res.S[k][r, q]:.3g} n {res.n[k][r, q]:.0f} error/bound {err[r, q] / B[r, q] if B[r, q] > 0 else float('inf'):.3g}")
    return "\n".join(lines)


def hvp(res, v, N):
    """(H·v, bound) in params! order from the blocks of `res` (every column), v float64 [P]: the products in the reference's
    number type, the bound from Σ|term·v| the same way (+ one rounding per product and per row sum)."""
    b = backend(None if res.blocks[0].dtype != np.float64 else np.float64)
    v = np.asarray(v, dtype=np.float64)
    want, B = b.zeros(len(v)), np.zeros(len(v))
    for k, c in enumerate(res.columns):
        idx = block_index(N, res.kinds, c)
        av = np.abs(v[idx])
        want[idx] = -(res.blocks[k] @ b.arr(v[idx]))
        S = res.S[k] @ av
        nz = float((av > 0).sum())
        B[idx] = np.where(S > 0, EPS * (res.R[k] @ av + ((res.n[k] * (av > 0)).max(axis=1) + nz + 8.0) * S) + res.U[k] @ av, 0.0) \
            + res.tiny[k] @ av
    return want, B


@functools.lru_cache(maxsize=None)
def prepared(name, columns=None):
    """(case, Result) of a named case, computed once per session and shared by the host and the GPU tests."""
    case = ALL_CASES[name]()
    return case, evaluate(model_of(case), case["times"], case["nodes"], case["T"], recursive=case["recursive"], columns=columns)
