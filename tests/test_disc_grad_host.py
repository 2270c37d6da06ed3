"""The discrete gradient reference (tests/disc_grad_ref.py) checked without a GPU: its intensity and log-likelihood against
the oracle, its gradient against central differences of the oracle's log-likelihood (homogeneous and LGCP baseline), its
two number types against each other; then, on every input of tests/test_discrete_edges_gpu.py (C1-C3), that a plain float64
evaluation of the same formulas stays inside the gradient bound the GPU is held to -- the inputs, not only the kernels, let
the bound be met; and the refusal of a negative count before any device work."""
import numpy as np
import pytest

import disc_edge_cases as cases
import disc_grad_ref as ref


def small(orc, lgcp, seed=12):
    rng = np.random.default_rng(seed)
    N, T, B, L, dt = 3, 400, 2, 5, 0.5
    c = dict(data=rng.poisson(0.4, (N, T)).astype(np.int64), phi=orc.disc_basis(L, B, dt), W=rng.uniform(0.05, 0.3, (N, N)),
             theta=cases._theta(rng, N, B), dt=dt)
    if lgcp:
        c.update(grid_x=np.linspace(0.0, float(T), 7), lam_grid=np.exp(rng.normal(-1.0, 0.5, (7, N))))
    else:
        c.update(lam0=rng.uniform(0.3, 0.8, N))
    return c


def oracle_lambda(orc, c, conv, base_params, eta):
    W = eta.sum(axis=2)
    th = eta / W[:, :, None]
    if "lam0" in c:
        return orc.disc_intensity(conv, base_params, W, th, c["dt"])
    T = c["data"].shape[1]
    base_tn = orc.disc_lgcp_intensity(c["grid_x"], base_params.reshape(c["lam_grid"].shape, order="F"), c["dt"],
                                      np.arange(1, T + 1, dtype=np.float64))
    return orc.disc_intensity_b(conv, base_tn, W, th, c["dt"])


@pytest.mark.parametrize("lgcp", [False, True])
def test_reference_equals_the_oracle_and_its_finite_differences(orc, lgcp):
    c = small(orc, lgcp)
    data = c["data"]
    N, T = data.shape
    B = c["phi"].shape[1]
    r = ref.evaluate(data, **{k: v for k, v in c.items() if k != "data"})
    conv = orc.disc_convolve(data, c["phi"])
    assert np.max(np.abs(r.conv - conv)) <= 1e-15 * np.max(conv)
    x = np.concatenate([(c["lam0"] if not lgcp else c["lam_grid"].ravel(order="F")), (c["W"][:, :, None] * c["theta"]).ravel(order="F")])
    nb = len(x) - N * N * B

    def f(v):
        return orc.disc_loglik(data, oracle_lambda(orc, c, conv, v[:nb], v[nb:].reshape((N, N, B), order="F")))

    want = oracle_lambda(orc, c, conv, x[:nb], x[nb:].reshape((N, N, B), order="F"))
    assert float(np.max(np.abs(r.lam - want) / want)) < 1e-13
    assert abs(float(r.ll) - f(x)) < 1e-13 * abs(f(x))
    assert len(r.grad) == len(r.scale) == len(x)
    assert np.all(r.scale >= np.abs(r.grad))
    for k in range(len(x)):
        h = 1e-6 * max(1.0, abs(x[k]))
        xp, xm = x.copy(), x.copy()
        xp[k] += h
        xm[k] -= h
        fd = (f(xp) - f(xm)) / (2 * h)
        assert abs(float(r.grad[k]) - fd) < 1e-5 * max(1.0, abs(fd)), (k, float(r.grad[k]), fd)


def test_mpmath_route_agrees_with_long_double(orc):
    """The 40-digit route (taken where long double is no wider than double) on a shape small enough for it."""
    rng = np.random.default_rng(5)
    N, T, B, L, dt = 3, 17, 2, 5, 0.5
    data = rng.poisson(0.8, (N, T)).astype(np.int64)
    data[1, 3] = 300                                                  # Stirling's series against mpmath's loggamma
    kw = dict(phi=orc.disc_basis(L, B, dt), W=rng.uniform(0.05, 0.3, (N, N)), theta=cases._theta(rng, N, B), dt=dt)
    for base in (dict(lam0=rng.uniform(0.3, 0.8, N)), dict(grid_x=np.linspace(0.0, 17.0, 4), lam_grid=rng.uniform(0.3, 0.8, (4, N)))):
        a = ref.evaluate(data, real="mpmath", **kw, **base)
        mp = ref.backend("mpmath")

        def lift(v):                                                  # a long double as the exact sum of two doubles
            v = np.atleast_1d(np.asarray(v, dtype=np.longdouble))
            hi = v.astype(np.float64)
            return mp.arr(hi) + mp.arr((v - hi).astype(np.float64))

        def f64(v):
            return np.atleast_1d(v).astype(np.float64)

        for real, tol in ((np.longdouble, 64 * float(np.finfo(np.longdouble).eps)), (np.float64, 64 * 2.0 ** -52)):
            b = ref.evaluate(data, real=real, **kw, **base)
            assert np.all(np.abs(f64(lift(b.ll) - a.ll)) < tol * np.abs(f64(a.ll)))
            assert np.all(np.abs(f64(lift(b.lam) - a.lam)) <= tol * f64(a.lam))
            assert np.all(np.abs(f64(lift(b.grad) - a.grad)) <= tol * f64(a.scale))
            assert np.all(np.abs(f64(lift(b.scale) - a.scale)) <= tol * f64(a.scale))


def test_reference_number_type():
    assert ref.LONGDOUBLE_OK == (np.finfo(np.longdouble).eps < 1e-18)
    k = ref.backend()
    assert isinstance(k, ref._Numpy if ref.LONGDOUBLE_OK else ref._Mpmath)


@pytest.mark.parametrize("name", cases.ALL)
def test_float64_evaluation_meets_the_gpu_gradient_bound(orc, name):
    """|g64 - g_ref| <= (N·B + T + 16)·2⁻⁵³·S entry by entry, λ to 1e-12 and ll to 1e-11 as the GPU tests ask."""
    N, T, B = cases.shape(orc, name)
    r, d = cases.reference(orc, name), cases.float64(orc, name)
    bound = ref.gradient_bound(N, T, B, r.scale)
    err = np.abs(d.grad - r.grad)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
    scaled = float(np.max(np.where(r.scale > 0, err / np.where(r.scale > 0, r.scale, 1), 0.0)))
    print(f"{name}: float64 error / bound = {worst:.3g}, error / scale = {scaled:.3g}")
    assert np.all(err <= bound)
    assert float(np.max(np.abs(d.lam - r.lam) / r.lam)) < 1e-12
    assert abs(float(d.ll - r.ll)) <= 1e-11 * abs(float(r.ll))


def test_a_single_negative_count_is_refused_before_any_device_work(nhp):
    """[-1, 0, 5, ...]: the node's total is positive, the entry is not.  The refusal comes from DiscreteDataset itself,
    ahead of the library call: no context (and no GPU) is touched."""
    data = np.zeros((3, 40), dtype=np.int64)
    data[1, :3] = [-1, 0, 5]
    data[0, 7] = 2
    assert data[1].sum() > 0
    with pytest.raises(nhp.DomainError, match="counts must be non-negative"):
        nhp.DiscreteDataset(None, data)
    with pytest.raises(nhp.DomainError, match="counts must be non-negative"):
        nhp.DiscreteDataset(None, data.astype(np.int32))
