"""Extended-precision restatement of the discrete intensity, Poisson log-likelihood and its gradient, written from the
formulas in the comments of csrc/disc.hip (k_disc_convolve, k_disc_bump, k_disc_base_interp, k_disc_grad_finish,
k_disc_grad_lgcp), not from the kernels:

    Ŝ[t,p,b] = max(0, Σ_{l=1..min(L,t)} data[p,t-l]·ϕ[l,b])             direct form, lag 0 excluded, 0-based t
    λ[t,c]   = base[t,c] + dt·Σ_{p,b} Ŝ[t,p,b]·W[p,c]·θ[p,c,b]         (·A[p,c] for a network process)
    base[t,c] = λ0[c]·dt          or, with a grid,   Σ_g w_g(t+1)·λgrid[g,c]·dt
    ll       = Σ_{t,c} s·log λ - λ - lgamma(s+1),   0·log λ = 0,   s = data[c,t]

w_g(time) are the weights of the piecewise-linear interpolant through the grid points x: time in [x[a], x[a+1]) gives
w_a = (x[a+1] - time)/(x[a+1] - x[a]), w_{a+1} = (time - x[a])/(x[a+1] - x[a]); time >= x[end] gives w_end = 1.

The gradient is in the library's parameter order [params(baseline); vec(η)], η = W∘θ as (N, N, B) in column-major order
(p fastest), params(baseline) = λ0 or vec(λgrid) (G x N, g fastest):

    ∂ll/∂λ0[c] = dt·Σ_t (s/λ - 1)       ∂ll/∂λgrid[g,c] = dt·Σ_t (s/λ - 1)·w_g(t+1)       ∂ll/∂η[p,c,b] = dt·Σ_t (s/λ - 1)·Ŝ[t,p,b]

Next to every gradient entry stands its scale, the sum of the absolute values of its terms (s/λ + 1 in place of s/λ - 1):
what a rounding-error bound of a sum of these terms, in any order, is a multiple of.

Everything is evaluated in numpy's long double where that is the x87 80-bit format or wider (eps < 1e-18), otherwise in
mpmath numbers of 40 digits held in object arrays; `real=np.float64` gives the plain double evaluation of the same
formulas.  Test code only."""
import numpy as np

LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)
MP_DIGITS = 40


class _Numpy:
    """The formulas below in a numpy floating type."""

    def __init__(self, real):
        self.real = real

    def arr(self, a):
        return np.asarray(a, dtype=self.real)

    def num(self, v):
        return self.real(v)

    def zeros(self, shape):
        return np.zeros(shape, dtype=self.real)

    def log(self, a):
        return np.log(a)

    def lgamma1(self, s):
        """lgamma(s + 1) of non-negative integers: Σ_{k<=s} log k up to 255, Stirling's series from there on."""
        s = np.asarray(s, dtype=np.int64)
        r = self.real
        table = np.concatenate([[r(0), r(0)], np.cumsum(np.log(np.arange(2, 256, dtype=r)))])
        out = table[np.minimum(s, 255)]
        big = s > 255
        if big.any():
            x = self.arr(s[big]) + r(1)
            pi = r(4) * np.arctan(r(1))
            x2 = x * x
            series = (r(1) / 12 - (r(1) / 360 - (r(1) / 1260 - r(1) / (1680 * x2)) / x2) / x2) / x      # next term 1/(1188 x^9) < 2e-25
            out[big] = (x - r(1) / 2) * np.log(x) - x + np.log(2 * pi) / 2 + series
        return out


class _Mpmath:
    """The same in mpmath numbers of MP_DIGITS digits, held in numpy object arrays."""

    def __init__(self):
        import mpmath
        self.mp = mpmath
        self._mpf = np.frompyfunc(lambda v: mpmath.mpf(v), 1, 1)
        self._log = np.frompyfunc(lambda v: mpmath.log(v), 1, 1)
        self._lg = np.frompyfunc(lambda v: mpmath.loggamma(mpmath.mpf(int(v)) + 1), 1, 1)

    def arr(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        return self._mpf(a.astype(np.int64).astype(object) if a.dtype.kind in "iu" else a.astype(np.float64).astype(object))

    def num(self, v):
        return self.mp.mpf(v)

    def zeros(self, shape):
        return self._mpf(np.zeros(shape).astype(object))

    def log(self, a):
        return self._log(a)

    def lgamma1(self, s):
        return self._lg(np.asarray(s, dtype=np.int64).astype(object))


def backend(real=None):
    """real = None: long double, or mpmath where long double is no wider than double; np.float64 / np.longdouble: that
    type; "mpmath": the 40-digit numbers."""
    if real is None:
        real = np.longdouble if LONGDOUBLE_OK else "mpmath"
    if isinstance(real, str):
        assert real == "mpmath"
        import mpmath
        mpmath.mp.dps = max(mpmath.mp.dps, MP_DIGITS)
        return _Mpmath()
    return _Numpy(real)


def convolve(data, phi, real=None):
    """Ŝ [T, N, B] of the N x T counts and the L x B basis."""
    k = backend(real)
    data = np.asarray(data)
    N, T = data.shape
    L, B = phi.shape
    d, ph = k.arr(data.T), k.arr(phi)                           # [T, N], [L, B]
    out = k.zeros((T, N, B))
    for l in range(1, min(L, T - 1) + 1):                       # bin t takes data[:, t - l]: lags past the start add nothing
        out[l:] = out[l:] + d[:T - l, :, None] * ph[l - 1][None, None, :]
    neg = out < 0
    if neg.any():
        out[neg] = k.zeros(int(neg.sum()))
    return out


def interp_weights(x, T, real=None):
    """w [T, G]: w[t, g] = w_g(t + 1), the interpolation weights of bin t (evaluated at time t + 1) on the grid x."""
    k = backend(real)
    xf = np.asarray(x, dtype=np.float64)
    G = len(xf)
    xx = k.arr(xf)
    w = k.zeros((T, G))
    for t in range(T):
        time = float(t + 1)
        if not time < xf[G - 1]:
            w[t, G - 1] = k.num(1.0)
            continue
        a = int(np.searchsorted(xf, time, side="right")) - 1   # x[a] <= time < x[a+1]
        tt = k.num(time)
        width = xx[a + 1] - xx[a]
        w[t, a] = (xx[a + 1] - tt) / width
        w[t, a + 1] = (tt - xx[a]) / width
    return w


class Result:
    """conv [T,N,B], lam [T,N], ll, grad [P], scale [P] (same order as grad), base [T,N]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def evaluate(data, phi, W, theta, dt, lam0=None, grid_x=None, lam_grid=None, A=None, real=None):
    """Intensity, log-likelihood, gradient and gradient scales of the N x T counts `data`: basis phi [L, B], W [N, N]
    and theta [N, N, B] indexed [parent, child(, basis)], a homogeneous baseline lam0 [N] or the grid (grid_x [G],
    lam_grid [G, N]).  Arrays of the evaluation's number type."""
    k = backend(real)
    data = np.asarray(data)
    N, T = data.shape
    B = phi.shape[1]
    K = N * B
    dtk = k.num(float(dt))
    conv = convolve(data, phi, real)                            # [T, N, B]
    Wk = k.arr(W) if A is None else k.arr(W) * k.arr(A)
    eta = Wk[:, :, None] * k.arr(theta)                         # [p, c, b]
    S2 = conv.reshape(T, K)                                     # column p·B + b
    E2 = eta.transpose(0, 2, 1).reshape(K, N) * dtk             # row p·B + b, column c
    if lam0 is not None:
        w = None
        base = np.broadcast_to((k.arr(lam0) * dtk)[None, :], (T, N))
    else:
        w = interp_weights(grid_x, T, real)
        base = (w @ k.arr(lam_grid)) * dtk
    lam = base + S2 @ E2
    s = k.arr(data.T)                                           # [T, N]
    occupied = data.T != 0
    slog = k.zeros((T, N))
    slog[occupied] = s[occupied] * k.log(lam[occupied])
    ll = (slog - lam - k.lgamma1(data.T)).sum()
    R = s / lam
    one = k.num(1.0)
    g_eta = (S2.T @ (R - one)) * dtk                            # [p·B + b, c]
    s_eta = (S2.T @ (R + one)) * dtk
    to_vec = lambda m: m.reshape(N, B, N).transpose(0, 2, 1).ravel(order="F")          # -> (p, c, b), p fastest
    if w is None:
        g_base, s_base = (R - one).sum(axis=0) * dtk, (R + one).sum(axis=0) * dtk
    else:
        g_base = ((w.T @ (R - one)) * dtk).ravel(order="F")      # [G, N], g fastest
        s_base = ((w.T @ (R + one)) * dtk).ravel(order="F")
    return Result(conv=conv, base=base, lam=lam, ll=ll, grad=np.concatenate([g_base, to_vec(g_eta)]),
                  scale=np.concatenate([s_base, to_vec(s_eta)]))


def gradient_bound(N, T, B, scale):
    """(N·B + T + 16)·2⁻⁵³·scale: λ carries at most N·B + 2 roundings into R = s/λ, a sum over the bins at most T
    more in whatever order it is taken, and 16 stand for the roundings of Ŝ (L <= 16 lags here), of dt and of the final
    subtraction.  First order and worst case; an entry that lost a term, a slab or a tile is off by scale/T or more."""
    return (N * B + T + 16) * 2.0 ** -53 * scale
