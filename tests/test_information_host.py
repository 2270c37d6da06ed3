"""tests/information_ref.py tied to the definitions, and the host part of standard_errors.  No GPU.

  * the reference's blocks equal central differences of cont_grad_ref.evaluate(..., real=np.float64) -- the gradient
    reference, not the code under test -- within the differencing error, 1e-6·max|block of the column| for a step of 1e-6 (a parameter
    that sits at 0, where the gradient reference takes no negative weight, gets the one-sided second-order formula);
  * blocks are symmetric;
  * the plain float64 evaluation of the same sums in forward, reversed and permuted order stays inside the bound (the bound
    is not too tight), and the check rejects two planted errors: the curvature term Σ g·∇²λ dropped, and one θ moved by a
    relative 1e-9 (the bound is not too loose);
  * standard_errors' free-set and pd logic on hand-made blocks;
  * the argument errors of the three entry points, raised before any device work."""
import numpy as np
import pytest

import cont_grad_ref as cr
import information_ref as ir

STEP = 1e-6


def _with(case, name, p, c, value):
    out = dict(case)
    if name == "lam0":
        out["lam0"] = case["lam0"].copy()
        out["lam0"][c] = value
    else:
        out[name] = case[name].copy()
        out[name][p, c] = value
    return out


def _grad_rows(case, c, idx):
    res = cr.evaluate(cr.model_of(case), case["times"], case["nodes"], case["T"], recursive=case["recursive"], columns=(c, c + 1),
                      real=np.float64)
    return np.asarray(res.grad, dtype=np.float64)[idx]


@pytest.mark.parametrize("name", ["W-exp", "W-logit", "W-net"])
def test_blocks_equal_central_differences_of_the_gradient_reference(name):
    case, res = ir.prepared(name)
    N = case["N"]
    kinds = ("theta", "W") if case["kind"] == "exponential" else ("mu", "tau", "W")
    worst = 0.0
    for k, c in enumerate(res.columns):
        idx = ir.block_index(N, len(kinds), c)
        J = np.asarray(res.blocks[k], dtype=np.float64)
        assert np.array_equal(J, J.T) or np.abs(J - J.T).max() <= 1e-15 * np.abs(J).max()
        H = np.empty_like(J)
        for r in range(len(idx)):
            nm, p = ("lam0", None) if r == 0 else (kinds[(r - 1) // N], (r - 1) % N)
            x = case["lam0"][c] if r == 0 else case[nm][p, c]
            if x - STEP < 0.0 and nm in ("W", "lam0"):               # one-sided, second order: no negative weight
                g0, g1, g2 = (_grad_rows(_with(case, nm, p, c, x + s * STEP), c, idx) for s in (0, 1, 2))
                H[:, r] = (-3.0 * g0 + 4.0 * g1 - g2) / (2.0 * STEP)
            else:
                gp, gm = (_grad_rows(_with(case, nm, p, c, x + s * STEP), c, idx) for s in (1, -1))
                H[:, r] = (gp - gm) / (2.0 * STEP)
        tol = 1e-6 * np.abs(H).max()                                   # of the column's block
        err = np.abs(H + J)
        if tol > 0:
            worst = max(worst, float(err.max() / tol))
        assert np.all(err <= tol), (name, c, np.argwhere(err > tol)[:5], err.max(), tol)
    print(f"{name}: largest difference / tolerance {worst:.3g}")


@pytest.mark.parametrize("name", ["W-exp", "W-logit", "W-net", "W-net-logit", "D", "L-exp", "L-logit",
                                  "P4-exp", "P4-logit", "P4-net", "P2-inf"])
def test_float64_in_any_order_stays_inside_the_bound(name):
    case, res = ir.prepared(name)
    m = cr.model_of(case)
    worst = 0.0
    for order in ("forward", "reversed", "permuted"):
        got = ir.evaluate(m, case["times"], case["nodes"], case["T"], recursive=case["recursive"], real=np.float64, order=order, seed=3)
        for k in range(len(res.columns)):
            ratio, bad, err, B = ir.check(got.blocks[k], res, k)
            assert len(bad) == 0, f"{name} {order}\n" + ir.explain(got.blocks[k], res, k, bad, err, B)
            worst = max(worst, ratio)
    print(f"{name}: float64 error/bound at most {worst:.3g}")
    assert worst < 1.0


@pytest.mark.parametrize("name", ["W-exp", "W-logit", "W-net"])
def test_the_check_rejects_planted_errors(name):
    case, res = ir.prepared(name)
    m = cr.model_of(case)
    args = (case["times"], case["nodes"], case["T"])
    dropped = ir.evaluate(m, *args, real=np.float64, curvature=False)
    assert any(len(ir.check(dropped.blocks[k], res, k)[1]) for k in range(len(res.columns))), "the curvature term went unnoticed"
    moved = dict(case)
    key = "theta" if case["kind"] == "exponential" else "mu"
    moved[key] = case[key].copy()
    moved[key][0, 0] *= 1.0 + 1e-9
    shifted = ir.evaluate(cr.model_of(moved), *args, real=np.float64, columns=[0])
    k0 = res.columns.index(0)
    assert len(ir.check(shifted.blocks[0], res, k0)[1]), "a parameter moved by a relative 1e-9 went unnoticed"


def test_hvp_reference_is_the_block_product():
    case, res = ir.prepared("W-exp")
    N = case["N"]
    P = N + 2 * N * N
    v = np.random.default_rng(0).normal(size=P)
    want, B = ir.hvp(res, v, N)
    idx = ir.block_index(N, 2, 3)
    k = res.columns.index(3)
    assert np.allclose(np.asarray(want, dtype=np.float64)[idx], -np.asarray(res.blocks[k], dtype=np.float64) @ v[idx], rtol=1e-12, atol=0)
    rows = np.asarray(res.S[k]).sum(axis=1) > 0                        # (an empty parent node has a zero row)
    assert np.all(B[idx][rows] > 0) and np.all(B[idx][~rows] == 0) and rows.sum() > N


# ---------------------------------------------------------------------------------------------------- standard_errors
def test_standard_errors_free_set_and_pd_logic(nhp):
    from nhp_amd import inference as inf
    N, kinds = 2, 2
    D = 1 + kinds * N
    rng = np.random.default_rng(1)
    Q = rng.normal(size=(D, D))
    good = Q @ Q.T + D * np.eye(D)
    x = np.array([0.5, 0.7, 1.0, 2.0, 3.0, 4.0, 0.1, 0.2, 0.3, 0.4])    # [λ0 (2); θ (4); W (4)]
    # column 0: positive definite, every parameter inside the box
    blocks = np.stack([good, good.copy()])
    # column 1: W[1, 1] on the lower bound, θ[0, 1]'s row identically zero (a parent no window joins)
    x[9] = 1e-6
    zero_row = 1                                                        # block row of θ[0, 1]
    blocks[1][zero_row, :] = 0.0
    blocks[1][:, zero_row] = 0.0
    out = inf._standard_errors_from_blocks(blocks, np.array([0, 1]), x, N, kinds, 1e-6, 10.0, 0.95)
    assert out.pd.tolist() == [True, True]
    i0, i1 = inf.block_index(N, kinds, 0), inf.block_index(N, kinds, 1)
    assert np.allclose(out.se[i0], np.sqrt(np.diag(np.linalg.inv(good))), rtol=1e-12)
    assert out.free[i0].all()
    f1 = np.ones(D, dtype=bool)
    f1[zero_row] = False
    f1[list(i1).index(9)] = False
    assert out.free[i1].tolist() == f1.tolist()
    assert np.all(np.isnan(out.se[i1][~f1])) and np.all(np.isnan(out.lower_ci[i1][~f1]))
    assert np.allclose(out.se[i1][f1], np.sqrt(np.diag(np.linalg.inv(blocks[1][np.ix_(f1, f1)]))), rtol=1e-12)
    z = 1.959963984540054
    assert np.allclose(out.upper_ci[i0] - x[i0], z * out.se[i0], rtol=1e-12) and np.allclose(x[i0] - out.lower_ci[i0], z * out.se[i0], rtol=1e-12)
    # a column that is not positive definite: pd False, NaNs, no exception; the other column is untouched
    bad = good.copy()
    bad[2, 2] = -1.0
    out = inf._standard_errors_from_blocks(np.stack([bad, good]), np.array([0, 1]), np.where(np.arange(10) == 9, 0.4, x), N, kinds,
                                           1e-6, 10.0, 0.95)
    assert out.pd.tolist() == [False, True]
    assert np.all(np.isnan(out.se[i0])) and not out.free[i0].any() and np.all(np.isfinite(out.se[i1]))
    # only the listed columns are filled
    out = inf._standard_errors_from_blocks(good[None], np.array([1]), np.where(np.arange(10) == 9, 0.4, x), N, kinds, 1e-6, 10.0, 0.95)
    assert np.all(np.isnan(out.se[i0])) and np.all(np.isfinite(out.se[i1])) and out.pd.tolist() == [True]


def test_argument_errors_come_before_any_device_work(nhp, monkeypatch):
    from nhp_amd import _lib, inference as inf

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(_lib, "default_context", no_device)
    monkeypatch.setattr(inf, "device_dataset", no_device)
    N = 3
    rng = np.random.default_rng(0)
    data = (np.sort(rng.uniform(0, 10, 50)), rng.integers(1, N + 1, 50), 10.0)
    W, th = np.full((N, N), 0.1), np.full((N, N), 2.0)
    std = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.ones(N)), nhp.ExponentialImpulseResponse(th, 1.0, 1.0, 1.0),
                                              nhp.DenseWeightModel(W))
    lgcp = nhp.ContinuousStandardHawkesProcess(nhp.LogGaussianCoxProcess(np.linspace(0, 10, 5), [np.ones(5)] * N),
                                               nhp.ExponentialImpulseResponse(th, 1.0, 1.0, 1.0), nhp.DenseWeightModel(W))
    P = N + 2 * N * N
    calls = [lambda p, d: nhp.observed_information(p, d), lambda p, d: nhp.hessian_vector_product(p, d, np.zeros(P)),
             lambda p, d: nhp.standard_errors(p, d)]
    for call in calls:
        with pytest.raises(TypeError):
            call(object(), data)
        with pytest.raises(NotImplementedError):
            call(lgcp, data)
    shard = object.__new__(nhp.ShardedDataset)
    for call in calls:
        with pytest.raises(NotImplementedError):
            call(std, shard)
    for cols in ([3], [-1], [0, 0], [], [0.5]):
        with pytest.raises(ValueError):
            nhp.observed_information(std, data, columns=cols)
    for tn in (-1, N + 1, 1.5):
        with pytest.raises(ValueError):
            nhp.observed_information(std, data, tile_nodes=tn)
    with pytest.raises(ValueError):
        nhp.hessian_vector_product(std, data, np.zeros(P + 1))
    with pytest.raises(ValueError):
        nhp.standard_errors(std, data, level=1.0)
    with pytest.raises(ValueError):
        nhp.standard_errors(std, data, lower=1.0, upper=1.0)


def test_header_declares_the_two_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nhp.h")).read()
    assert "nhp_status nhp_cont_information(" in header and "nhp_status nhp_cont_hessian_vec(" in header
    julia = open(os.path.join(root, "networkhawkesprocesses.jl_amd", "julia", "NetworkHawkesHIP.jl")).read()
    assert ":nhp_cont_information" in julia and ":nhp_cont_hessian_vec" in julia
