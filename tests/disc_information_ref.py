"""Extended-precision restatement of the observed and the Fisher information of the discrete log-likelihood and of their
products with a vector, written from the formulas, not from the kernels, on disc_grad_ref's backend, `convolve` and
`evaluate`.

In mle!'s parameters x = [λ0 (N); vec(η)], η = W∘θ as (N, N, B) in column-major order, the intensity is linear,

    λ[t,c] = dt·x_tᵀ z_c,     x_t = [1; Ŝ[t,·,·]] (D = 1 + N·B),     z_c = [λ0[c]; η[·,c,·]],

so minus the Hessian is block diagonal by child node c.  Row 0 of a block is λ0[c], row 1 + b·N + p is η[p,c,b]:

    observed  J_c = dt²·Σ_t w·x_t x_tᵀ,  w = s[t,c]/λ[t,c]²  (exactly 0 where s = 0)        Fisher  w = 1/λ[t,c]

Every term of an entry is >= 0 (Ŝ is clamped at 0), so the entry is its own scale: a rounding-error bound of the sum, in any
order, is a multiple of it.  n_t is the number of bins with a non-zero weight in the column (the terms of an entry).

    (J·v)[i] = dt²·Σ_t w·x_i·(Σ_j x_j v_j)       with the scale       S_hv[i] = dt²·Σ_t w·x_i·Σ_j |x_j v_j|

Test code only."""
import functools

import numpy as np

import disc_grad_ref as ref

KINDS = ("observed", "fisher")


def block_index(N, B, c):
    """Positions in [λ0; vec(η)] of the rows of column c's block."""
    return np.concatenate([[c], N + (np.arange(B)[:, None] * N * N + np.arange(N)[None, :] + c * N).ravel()])


def design(conv, real=None):
    """X [T, D]: column 0 ones, column 1 + b·N + p = Ŝ[t,p,b]."""
    k = ref.backend(real)
    T, N, B = conv.shape
    X = k.zeros((T, 1 + N * B))
    X[:, 0] = k.num(1.0)
    X[:, 1:] = conv.transpose(0, 2, 1).reshape(T, N * B)
    return X


def weights(data, lam, kind, real=None):
    """w [T, N] and the occupied mask: s/λ² with an exact 0 where s = 0, or 1/λ."""
    assert kind in KINDS
    k = ref.backend(real)
    occupied = np.asarray(data).T != 0
    if kind == "fisher":
        return k.num(1.0) / lam, np.ones_like(occupied)
    w = k.zeros(lam.shape)
    s = k.arr(np.asarray(data).T)
    w[occupied] = s[occupied] / (lam[occupied] * lam[occupied])
    return w, occupied


class Result:
    """columns [n], blocks [n, D, D], n_t [n], and what they were made from: X [T, D], w [T, N], lam [T, N], dt."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def evaluate(case, kind, columns=None, real=None, base=None):
    """Blocks of `kind` for the columns (all by default) of a case of tests/disc_edge_cases.py's form (homogeneous baseline).
    base: disc_grad_ref.evaluate's result for the same case and number type, when the caller has it already."""
    k = ref.backend(real)
    data = np.asarray(case["data"])
    N, T = data.shape
    if base is None:
        base = ref.evaluate(data, real=real, **{n: v for n, v in case.items() if n != "data"})
    X = design(base.conv, real)
    w, live = weights(data, base.lam, kind, real)
    cols = list(range(N)) if columns is None else [int(c) for c in columns]
    dt2 = k.num(float(case["dt"])) * k.num(float(case["dt"]))
    D = X.shape[1]
    blocks = k.zeros((len(cols), D, D))
    n_t = np.zeros(len(cols), dtype=np.int64)
    for i, c in enumerate(cols):
        rows = live[:, c]
        n_t[i] = int(rows.sum())
        if n_t[i]:
            Xc = X[rows]
            blocks[i] = (Xc.T @ (Xc * w[rows, c][:, None])) * dt2
    return Result(columns=cols, blocks=blocks, n_t=n_t, X=X, w=w, live=live, lam=base.lam, dt=float(case["dt"]))


def hvp(res, v, N, B, real=None):
    """(J·v [P], S_hv [P], n_t [P]) from a Result over ALL columns."""
    k = ref.backend(real)
    assert res.columns == list(range(N))
    v = k.arr(np.asarray(v, dtype=np.float64))
    P = N + N * N * B
    out, scale = k.zeros(P), k.zeros(P)
    n_t = np.zeros(P, dtype=np.int64)
    dt2 = k.num(res.dt) * k.num(res.dt)
    for c in range(N):
        idx = block_index(N, B, c)
        rows = res.live[:, c]
        n_t[idx] = int(rows.sum())
        if not rows.any():
            continue
        Xc, vc = res.X[rows], v[idx]
        wc = res.w[rows, c]
        out[idx] = (Xc.T @ (wc * (Xc @ vc))) * dt2
        scale[idx] = (Xc.T @ (wc * (Xc @ abs(vc)))) * dt2
    return out, scale, n_t


def block_bound(N, B, n_t, J_ref):
    """(2·N·B + n_t + 48)·2⁻⁵³·J_ref: λ carries at most N·B + 2 roundings (disc_grad_ref.gradient_bound) and enters the
    weight twice; a sum over n_t bins adds at most n_t more, in any order; 48 covers Ŝ's own roundings on both factors
    (L <= 16), the products and dt²."""
    return (2 * N * B + n_t + 48) * 2.0 ** -53 * np.asarray(J_ref, dtype=np.float64)


def hv_bound(N, B, n_t, S_hv):
    """(3·N·B + n_t + 64)·2⁻⁵³·S_hv: as block_bound, plus the N·B + 1 terms of x·v and Ŝ's roundings once more."""
    return (3 * N * B + n_t + 64) * 2.0 ** -53 * np.asarray(S_hv, dtype=np.float64)


def check_blocks(got, res, N, B):
    """(largest error / bound, positions over the bound) of blocks `got` [n, D, D] against the reference Result: entries
    whose reference is 0 have no term and must be exact zeros."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(res.blocks, dtype=np.float64)
    err = np.abs(ref.backend().arr(got) - res.blocks).astype(np.float64)          # the difference in the reference's numbers
    bound = block_bound(N, B, np.asarray(res.n_t)[:, None, None], want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0, np.argwhere(err > bound)


@functools.lru_cache(maxsize=None)
def reference(orc, name, kind, columns=None):
    """The extended-precision blocks of a case of tests/disc_edge_cases.py, once per process (columns: a tuple, or None)."""
    import disc_edge_cases as cases
    return evaluate(cases.case(orc, name), kind, columns=columns, base=cases.reference(orc, name))
