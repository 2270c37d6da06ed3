"""Inputs of the discrete edge tests (tests/test_discrete_edges_gpu.py) as plain arrays, made without a GPU so that
tests/test_disc_grad_host.py can show, on the very same inputs, that a float64 evaluation of the formulas stays inside the
gradient bound.  A case is a dict: data [N, T] int64, phi [L, B], W [N, N], theta [N, N, B], dt, and lam0 [N] or
(grid_x [G], lam_grid [G, N]).  The extended-precision reference of a case is computed once per process."""
import functools

import numpy as np

import disc_grad_ref as ref

# C1: N, T, B, L, LGCP grid points (0 = homogeneous baseline) -- what each walks is in the GPU module's docstring
C1 = {
    "one_element": (1, 1, 1, 2, 0),
    "k_below_bk": (3, 17, 2, 5, 0),
    "fd_shape": (3, 400, 2, 5, 0),
    "ragged": (17, 129, 5, 9, 0),
    "two_column_tiles": (130, 997, 2, 3, 0),
    "whole_tiles": (128, 1280, 2, 4, 0),
    "one_column_over": (129, 65, 2, 3, 0),
    "lgcp": (64, 2000, 4, 8, 9),
}
C2 = ("all_zero", "one_bin", "half", "every_bin")                     # N = 5, T = 300, B = 3, L = 7
C3 = ("max_255", "with_256", "huge")                                  # N = 2, T = 192, B = 2, L = 4
ALL = tuple(C1) + C2 + C3


def _theta(rng, N, B):
    """Dirichlet draws rounded to multiples of 2^-20: every Σ_b θ[p,c,·] is exactly 1, as the constructor demands."""
    q = np.floor(rng.dirichlet(np.ones(B), (N, N)) * 2.0 ** 20)
    q[:, :, -1] = 2.0 ** 20 - q[:, :, :-1].sum(axis=2)
    return q / 2.0 ** 20


def _model(orc, rng, N, B, L, dt, G=0, T=0):
    case = dict(phi=orc.disc_basis(L, B, dt), W=rng.uniform(0.05, 0.3, (N, N)) / max(1, N // 4), theta=_theta(rng, N, B), dt=dt)
    if G:
        case.update(grid_x=np.linspace(0.0, float(T), G), lam_grid=np.exp(rng.normal(-1.0, 0.5, (G, N))))   # bins sit at 1..T
    else:
        case.update(lam0=rng.uniform(0.2, 1.0, N))
    return case


@functools.lru_cache(maxsize=None)
def _case(orc, name):
    if name in C1:
        N, T, B, L, G = C1[name]
        rng = np.random.default_rng(1000 + N + T)
        case = _model(orc, rng, N, B, L, 0.5, G, T)
        case["data"] = rng.poisson(0.4, (N, T)).astype(np.int64)
    elif name in C2:
        N, T, B, L = 5, 300, 3, 7
        rng = np.random.default_rng(2000)
        case = _model(orc, rng, N, B, L, 1.0)
        if name == "all_zero":
            data = np.zeros((N, T), dtype=np.int64)
        elif name == "one_bin":
            data = np.zeros((N, T), dtype=np.int64)
            data[3, 141] = 2
        elif name == "half":
            data = rng.poisson(0.7, (N, T)).astype(np.int64)
        else:
            data = 1 + rng.poisson(3.0, (N, T)).astype(np.int64)
        case["data"] = data
    else:
        N, T, B, L = 2, 192, 2, 4
        rng = np.random.default_rng(3000)
        case = _model(orc, rng, N, B, L, 1.0)
        data = np.minimum(rng.poisson(0.5, (N, T)), 254).astype(np.int64)
        data[0, 40] = 255
        case["lam0"] = np.array([40.0, 0.6])                # the baselines follow the planted counts (an intensity of 0.5 under a
        if name != "max_255":                               # count of 255 is no model of these data; the adjacency test says more)
            data[1, 77] = 256
            case["lam0"] = np.array([40.0, 40.0])
        if name == "huge":
            data[0, 10], data[0, 100], data[0, 150] = 70_000, 65_535, 65_536
            data[1, 120] = 1_200_000
            case["lam0"] = np.array([2.0e4, 2.0e5])
        case["data"] = data
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def case(orc, name):
    """The inputs of case `name` (read-only arrays, shared)."""
    return _case(orc, name)


def _kw(c):
    return {k: v for k, v in c.items() if k != "data"}


@functools.lru_cache(maxsize=None)
def reference(orc, name):
    """disc_grad_ref.evaluate of the case in extended precision, once."""
    c = _case(orc, name)
    return ref.evaluate(c["data"], **_kw(c))


def float64(orc, name):
    c = _case(orc, name)
    return ref.evaluate(c["data"], real=np.float64, **_kw(c))


def shape(orc, name):
    c = _case(orc, name)
    return c["data"].shape + (c["phi"].shape[1],)
