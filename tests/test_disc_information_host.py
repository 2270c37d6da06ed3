"""tests/disc_information_ref.py tied to the definitions, the bounds the GPU is held to shown to be attainable, and the host
part of disc_standard_errors.  No GPU.

  * the reference's observed blocks equal central differences of disc_grad_ref.evaluate(...).grad -- the gradient reference,
    not the code under test -- within a tolerance derived from the step and the third derivative (below);
  * a plain float64 numpy evaluation of the same sums, on the inputs of the GPU cases, stays inside the bounds of
    tests/test_disc_information_gpu.py for the blocks and for J·v (the bounds are not too tight), and the check rejects a
    planted error (not too loose);
  * the free-set, Cholesky, se_W and se_theta logic of disc_standard_errors on hand-made blocks;
  * the argument errors of the three entry points, raised before any device work.

The differencing tolerance.  The gradient is g_i = dt·Σ_t (s/λ - 1)·x_i, so ∂g_i/∂x_j = -J_ij and
∂³g_i/∂x_j³ = -6·dt⁴·Σ_t s·x_i·x_j³/λ⁴.  A central difference with step h is off by (h²/6)·|∂³g_i/∂x_j³| at a point within
h of x; moving x_j down by h divides no λ by less than 1 - h·max_t(dt·x_j/λ) =: 1 - ρ.  To that comes the rounding of the
two gradients, each inside disc_grad_ref.gradient_bound with the reference's own epsilon in place of 2⁻⁵³:

    tol_ij = h²·dt⁴·Σ_t s·x_i·x_j³/λ⁴ / (1 - ρ)⁴  +  (N·B + T + 16)·eps·scale_i / h

Largest difference / tolerance seen (x87 long double, h = 1e-4·x_j): 0.997 to 0.9999 -- the first term IS the leading term of
the differencing error, and the bound on it is rigorous (mean-value form), so the ratio approaches 1 from below."""
import numpy as np
import pytest

import disc_edge_cases as cases
import disc_grad_ref as ref
import disc_information_ref as ir

# the GPU module's cases on the inputs of tests/disc_edge_cases.py: name -> columns (None: all)
GPU_CASES = {"one_element": None, "k_below_bk": None, "ragged": None, "one_column_over": None, "two_column_tiles": (0, 77, 129),
             "all_zero": None, "one_bin": None, "half": None, "every_bin": None, "max_255": None, "with_256": None, "huge": None}
# central differences cost two gradient references per parameter: the small shapes, and two columns of `ragged`
FD_CASES = {"one_element": None, "k_below_bk": None, "fd_shape": (0, 2), "ragged": (0, 16), "one_bin": None, "half": (1, 3),
            "every_bin": (4,), "max_255": None, "huge": None}


def _gradient(c, x, N, B):
    eta = x[N:].reshape((N, N, B), order="F")
    W = eta.sum(axis=2)
    return ref.evaluate(c["data"], c["phi"], W, eta / W[:, :, None], c["dt"], lam0=x[:N])


@pytest.mark.parametrize("name", list(FD_CASES))
def test_observed_blocks_equal_central_differences_of_the_gradient_reference(orc, name):
    c = cases.case(orc, name)
    N, T, B = cases.shape(orc, name)
    k = ref.backend()
    eps = float(np.finfo(np.longdouble).eps) if ref.LONGDOUBLE_OK else 10.0 ** -(ref.MP_DIGITS - 2)
    res = ir.reference(orc, name, "observed", FD_CASES[name])
    x = k.arr(np.concatenate([c["lam0"], (c["W"][:, :, None] * c["theta"]).ravel(order="F")]))
    base = cases.reference(orc, name)
    dt = k.num(float(c["dt"]))
    s = k.arr(c["data"].T)
    worst = 0.0
    for i, col in enumerate(res.columns):
        idx = ir.block_index(N, B, col)
        J = res.blocks[i]
        assert np.all(np.abs(J - J.T) <= 8 * eps * np.abs(J))
        lam = base.lam[:, col]
        for j, pj in enumerate(idx):
            h = x[pj] * k.num(1e-4)
            xp, xm = x.copy(), x.copy()
            xp[pj] = x[pj] + h
            xm[pj] = x[pj] - h
            gp, gm = _gradient(c, xp, N, B), _gradient(c, xm, N, B)
            fd = -(gp.grad[idx] - gm.grad[idx]) / ((xp[pj] - xm[pj]))
            rho = float(np.max(dt * res.X[:, j] / lam)) * float(h)
            third = (dt ** 4) * (res.X.T @ (s[:, col] * res.X[:, j] ** 3 / lam ** 4))
            tol = (h * h * third / (1.0 - rho) ** 4 + (N * B + T + 16) * eps * gp.scale[idx] / h).astype(np.float64)
            err = np.abs(fd - J[:, j]).astype(np.float64)
            worst = max(worst, float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0)))))
            assert np.all(err <= tol), (name, col, j, float(err.max()), np.argwhere(err > tol)[:5])
    print(f"{name}: largest difference / tolerance {worst:.3g}")
    assert worst < 1.0


@pytest.mark.parametrize("kind", ir.KINDS)
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_float64_evaluation_meets_the_gpu_bounds(orc, name, kind):
    """Blocks entry by entry inside (2·N·B + n_t + 48)·2⁻⁵³·J_ref with exact zeros where the reference has no term; J·v
    inside (3·N·B + n_t + 64)·2⁻⁵³·S_hv."""
    N, T, B = cases.shape(orc, name)
    c = cases.case(orc, name)
    res = ir.reference(orc, name, kind, GPU_CASES[name])
    got = ir.evaluate(c, kind, columns=GPU_CASES[name], real=np.float64, base=cases.float64(orc, name))
    assert got.blocks.dtype == np.float64 and np.array_equal(got.n_t, res.n_t)
    ratio, bad = ir.check_blocks(got.blocks, res, N, B)
    line = f"{name}/{kind}: float64 blocks error / bound {ratio:.3g}"
    assert len(bad) == 0, (name, kind, bad[:5])
    assert np.all(np.asarray(got.blocks)[np.asarray(res.blocks, dtype=np.float64) == 0.0] == 0.0)
    if GPU_CASES[name] is None and N <= 17:
        v = np.random.default_rng(7).normal(size=N + N * N * B)
        want, scale, n_t = ir.hvp(res, v, N, B)
        mine, _, _ = ir.hvp(got, v, N, B, real=np.float64)
        bound = ir.hv_bound(N, B, n_t, scale)
        err = np.abs(ref.backend().arr(mine) - want).astype(np.float64)
        assert np.all(err <= bound)
        pos = bound > 0
        line += f"  J·v error / bound {float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0:.3g}"
    print(line)
    assert ratio < 1.0


def test_the_check_rejects_planted_errors(orc):
    """One bin dropped from a column, and one η moved by a relative 1e-9: either is far outside the bound."""
    name = "half"
    N, T, B = cases.shape(orc, name)
    c = cases.case(orc, name)
    res = ir.reference(orc, name, "observed", None)
    short = dict(c)
    data = c["data"].copy()
    t = int(np.flatnonzero(data[2])[-1])
    good = ir.evaluate(c, "observed", real=np.float64)
    dropped = np.array(good.blocks)
    x = good.X[t]
    dropped[2] -= c["dt"] ** 2 * good.w[t, 2] * np.outer(x, x)
    assert len(ir.check_blocks(dropped, res, N, B)[1]), "a dropped bin went unnoticed"
    short["W"] = c["W"].copy()
    short["W"][1, 2] *= 1.0 + 1e-9
    moved = ir.evaluate(short, "observed", real=np.float64)
    assert len(ir.check_blocks(moved.blocks, res, N, B)[1]), "a parameter moved by a relative 1e-9 went unnoticed"


# ---------------------------------------------------------------------------------------------- disc_standard_errors
def test_standard_errors_free_set_pd_and_link_logic(nhp):
    from nhp_amd import discrete as dd
    N, B = 2, 2
    D = 1 + N * B
    P = N + N * N * B
    rng = np.random.default_rng(1)
    Q = rng.normal(size=(D, D))
    good = Q @ Q.T + D * np.eye(D)
    x = rng.uniform(0.1, 0.9, P)
    i0, i1 = dd.disc_block_index(N, B, 0), dd.disc_block_index(N, B, 1)
    assert i0.tolist() == [0, 2, 3, 6, 7] and i1.tolist() == [1, 4, 5, 8, 9]             # λ0[c]; η[p,c,b] at 1 + b·N + p
    assert sorted(i0.tolist() + i1.tolist()) == list(range(P))
    # column 0: positive definite, every parameter inside the box
    blocks = np.stack([good, good.copy()])
    # column 1: η[1,1,1] on the lower bound, the row of η[0,1,0] identically zero (a parent that never precedes the column's events)
    on_bound = int(i1[4])
    x[on_bound] = 1e-6
    zero_row = 1
    blocks[1][zero_row, :] = 0.0
    blocks[1][:, zero_row] = 0.0
    out = dd._disc_standard_errors_from_blocks(blocks, np.array([0, 1]), x, N, B, 1e-6, 10.0, 0.95)
    assert out.pd.tolist() == [True, True]
    cov0 = np.linalg.inv(good)
    assert np.allclose(out.se[i0], np.sqrt(np.diag(cov0)), rtol=1e-12) and out.free[i0].all()
    f1 = np.ones(D, dtype=bool)
    f1[zero_row] = False
    f1[4] = False
    assert out.free[i1].tolist() == f1.tolist()
    assert np.all(np.isnan(out.se[i1][~f1])) and np.all(np.isnan(out.lower_ci[i1][~f1])) and np.all(np.isnan(out.upper_ci[i1][~f1]))
    cov1 = np.linalg.inv(blocks[1][np.ix_(f1, f1)])
    assert np.allclose(out.se[i1][f1], np.sqrt(np.diag(cov1)), rtol=1e-12)
    z = 1.959963984540054
    assert np.allclose(out.upper_ci[i0] - x[i0], z * out.se[i0], rtol=1e-12) and np.allclose(x[i0] - out.lower_ci[i0], z * out.se[i0], rtol=1e-12)
    # se_W against the explicit quadratic form 1ᵀ Cov(η[p,c,·]) 1, se_theta against the delta method written out
    for p in range(N):
        rows = [1 + b * N + p for b in range(B)]
        S = cov0[np.ix_(rows, rows)]
        one = np.ones(B)
        assert np.isclose(out.se_W[p, 0], np.sqrt(one @ S @ one), rtol=1e-12)
        eta = x[i0[rows]]
        w = eta.sum()
        for b in range(B):
            g = (np.eye(B)[b] - eta[b] / w) / w
            assert np.isclose(out.se_theta[p, 0, b], np.sqrt(g @ S @ g), rtol=1e-10)
    # column 1: parent 0 has only η[0,1,1] free (block row 3), parent 1 only η[1,1,0] (block row 2): W's error is that η's
    pos = np.cumsum(f1) - 1
    assert np.isclose(out.se_W[0, 1], np.sqrt(cov1[pos[3], pos[3]]), rtol=1e-12)
    assert np.isclose(out.se_W[1, 1], np.sqrt(cov1[pos[2], pos[2]]), rtol=1e-12)
    # a column that is not positive definite: pd False, NaNs, no exception; the other column is untouched
    bad = good.copy()
    bad[2, 2] = -1.0
    inside = np.where(np.arange(P) == on_bound, 0.4, x)
    out = dd._disc_standard_errors_from_blocks(np.stack([bad, good]), np.array([0, 1]), inside, N, B, 1e-6, 10.0, 0.95)
    assert out.pd.tolist() == [False, True]
    assert np.all(np.isnan(out.se[i0])) and not out.free[i0].any() and np.all(np.isfinite(out.se[i1]))
    assert np.all(np.isnan(out.se_W[:, 0])) and np.all(np.isfinite(out.se_W[:, 1])) and np.all(np.isnan(out.se_theta[:, 0]))
    # an all-zero block (no event in the column): nothing is free, pd False
    out = dd._disc_standard_errors_from_blocks(np.zeros((1, D, D)), np.array([0]), inside, N, B, 1e-6, 10.0, 0.95)
    assert out.pd.tolist() == [False] and not out.free.any() and np.all(np.isnan(out.se))
    # only the listed columns are filled
    out = dd._disc_standard_errors_from_blocks(good[None], np.array([1]), inside, N, B, 1e-6, 10.0, 0.95)
    assert np.all(np.isnan(out.se[i0])) and np.all(np.isfinite(out.se[i1])) and out.pd.tolist() == [True]


def test_argument_errors_come_before_any_device_work(nhp, monkeypatch):
    from nhp_amd import _lib, discrete as dd

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(_lib, "default_context", no_device)
    N, B, T = 3, 2, 40
    data = np.random.default_rng(0).poisson(0.3, (N, T))
    th = np.full((N, N, B), 0.5)
    W = np.full((N, N), 0.1)
    std = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.ones(N), 1.0), nhp.DiscreteGaussianImpulseResponse(th, 4, 1.0),
                                            nhp.DenseWeightModel(W), 1.0)
    lgcp = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteLogGaussianCoxProcess(np.linspace(0.0, T, 5), np.ones((5, N)), None, -1.0, 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(th, 4, 1.0), nhp.DenseWeightModel(W), 1.0)
    net = nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(np.ones(N), 1.0), nhp.DiscreteGaussianImpulseResponse(th, 4, 1.0),
                                           nhp.DenseWeightModel(W), np.ones((N, N)), nhp.DenseNetworkModel(N), 1.0)
    P = N + N * N * B
    calls = [lambda p: nhp.disc_observed_information(p, data), lambda p: nhp.disc_hessian_vector_product(p, data, v=np.zeros(P)),
             lambda p: nhp.disc_standard_errors(p, data)]
    for call in calls:
        with pytest.raises(TypeError):
            call(net)
        with pytest.raises(TypeError):
            call(object())
        with pytest.raises(NotImplementedError):
            call(lgcp)
    with pytest.raises(ValueError):
        nhp.disc_observed_information(std, data, kind="expected")
    with pytest.raises(ValueError):
        nhp.disc_standard_errors(std, data, level=1.0)
    with pytest.raises(ValueError):
        nhp.disc_standard_errors(std, data, lower=1.0, upper=1.0)
    with pytest.raises(TypeError):
        nhp.disc_standard_errors(std, data, regularize=True)              # there is no such argument
    monkeypatch.setattr(dd, "_convolved", lambda *a: type("DS", (), dict(N=N, B=B, T=T))())     # the checks behind the dataset's shape
    for cols in ([3], [-1], [0, 0], [], [0.5]):
        with pytest.raises(ValueError):
            nhp.disc_observed_information(std, data, columns=cols, ctx=object())
    for kw in (dict(tile_rows=-16), dict(slab_bins=-1), dict(tile_rows=1.5)):
        with pytest.raises(ValueError):
            nhp.disc_observed_information(std, data, ctx=object(), **kw)
    with pytest.raises(ValueError):
        nhp.disc_hessian_vector_product(std, data, v=np.zeros(P + 1), ctx=object())


def test_header_and_bindings_declare_the_two_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nhp.h")).read()
    assert "nhp_status nhp_disc_information(" in header and "nhp_status nhp_disc_hessian_vec(" in header
    julia = open(os.path.join(root, "networkhawkesprocesses.jl_amd", "julia", "NetworkHawkesHIP.jl")).read()
    assert ":nhp_disc_information" in julia and ":nhp_disc_hessian_vec" in julia
    binding = open(os.path.join(root, "networkhawkesprocesses.jl_amd", "_lib.py")).read()
    assert '"nhp_disc_information"' in binding and '"nhp_disc_hessian_vec"' in binding
