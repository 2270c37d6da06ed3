"""nhp_cont_information and nhp_cont_hessian_vec (csrc/cont_information.hip: k_info_blocks<IMP>, k_info_mirror,
k_info_hvp<IMP,G>) held to tests/information_ref.py entry by entry: |J - J_ref| <= bound, an entry without a single term an
exact zero, no entry skipped; the bound's derivation is in the reference's docstring, tests/test_information_host.py ties the
reference to central differences of the gradient reference.  The log-likelihood keeps the suite's 1e-11.

    W-exp, W-logit, W-net, W-net-logit   N=7 M=3000: ties, Δ = Δtmax exactly, an empty node, a one-event node, zero weights, a
                            flushing θ, A with a zero row and column; about 24 items per busy column; D = 15 | 22: one tile
    D                       N=3, one empty column (an all-zero block)
    L-exp, L-logit          N=2, windows up to 600 pairs: many pairs per parent node in one child's sums
    C, C-net                N=64, recursive=True through the truncated window, against the FULL-history reference + the 2⁻⁶⁰ tail
    W-exp, W-logit          again with tile_nodes=3: node runs of 3, 3 and 1, six tiles, a ragged last one, λ0 in run 0
    W-exp                   columns=[6, 0, 3]: those blocks in that order; device=True: a tensor on the device
    B-130                   N=130 M=3000, D = 261 beyond the LDS-resident limit: the automatic tiling (runs of 88 and 42 nodes, three tiles)

Blocks are sums of LDS and global fp64 atomics and so not bit-reproducible from run to run; what one
call returns is: every block exactly symmetric, and the device=True tensor holds what the same call's kernels wrote (it is
held to the reference like the host output, its structural zeros and its symmetry bit for bit).

hessian_vector_product: against (reference block)·v in long double with the bound built the same way from Σ|term·v|, for a
random v and v = e_k for one k per parameter kind; for v = e_k also against column k of the dense blocks of the other
kernel, within the sum of the two bounds.  regularize=True against the closed form of the prior's second derivatives.
standard_errors on a simulated exponential process of 8229 events at its true parameters.

Largest error/bound seen on an MI355X: 0.24 for the blocks and 0.14 for H·v (both B-130; 0.09 and 0.03 on the other cases);
the float64 host evaluation of the same sums reaches 0.13."""
import ctypes as C

import numpy as np
import pytest

import cont_grad_ref as cr
import information_ref as ir
from helpers import window_routes

pytestmark = pytest.mark.gpu

REL_LL = 1e-11
WINDOWED = ["W-exp", "W-logit", "W-net", "W-net-logit", "D", "L-exp", "L-logit"]


def call(nhp, case, **kw):
    proc = ir.process_of(nhp, case)
    return nhp.observed_information(proc, (case["times"], case["nodes"], case["T"]), recursive=case["recursive"], **kw)


def hold(label, info, case, res, columns=None, tail=False):
    assert abs(info.ll - float(res.ll)) <= REL_LL * abs(float(res.ll)), (label, info.ll, float(res.ll))
    blocks = info.blocks if isinstance(info.blocks, np.ndarray) else info.blocks.cpu().numpy()
    cols = list(range(case["N"])) if columns is None else list(columns)
    assert list(info.columns) == cols and blocks.shape[0] == len(cols)
    worst = 0.0
    m = cr.model_of(case)
    for i, c in enumerate(cols):
        k = res.columns.index(c)
        got = blocks[i]
        assert np.array_equal(got, got.T), f"{label}: block of column {c} is not exactly symmetric"
        t = ir.window_tail(res, k, m, case["times"], case["nodes"]) if tail else None
        ratio, bad, err, B = ir.check(got, res, k, t)
        assert len(bad) == 0, f"{label}: {len(bad)} entries outside the bound\n" + ir.explain(got, res, k, bad, err, B)
        worst = max(worst, ratio)
    print(f"{label}: error/bound {worst:.3g}")
    return blocks


@pytest.mark.parametrize("name", WINDOWED)
def test_blocks_against_the_reference(nhp, name):
    case, res = ir.prepared(name)
    hold(name, call(nhp, case), case, res)


@pytest.mark.parametrize("name", ["C", "C-net"])
def test_recursive_objective_through_its_truncated_window(nhp, name):
    case, res = ir.prepared(name)
    assert window_routes(nhp, ir.process_of(nhp, case), (case["times"], case["nodes"], case["T"])) == [1, 1, 1]
    hold(name, call(nhp, case), case, res, tail=True)


@pytest.mark.parametrize("name", ["W-exp", "W-logit"])
def test_forced_tiles_of_three_nodes(nhp, name):
    case, res = ir.prepared(name)
    hold(name + " tile_nodes=3", call(nhp, case, tile_nodes=3), case, res)
    hold(name + " tile_nodes=1", call(nhp, case, tile_nodes=1), case, res)


def test_selected_columns_come_in_the_order_asked_for(nhp):
    case, res = ir.prepared("W-exp")
    info = call(nhp, case, columns=[6, 0, 3])
    blocks = hold("W-exp columns=[6, 0, 3]", info, case, res, columns=[6, 0, 3])
    assert np.all(blocks[0] == 0.0)                                      # node 7 has no event
    assert info.names[0] == ("λ0", None) and info.names[1] == ("θ", 0) and info.names[8] == ("W", 0) and len(info.names) == 15


def test_device_output(nhp):
    import torch
    case, res = ir.prepared("W-logit")
    info = call(nhp, case, device=True)
    assert isinstance(info.blocks, torch.Tensor) and info.blocks.is_cuda and info.blocks.dtype == torch.float64
    dev = hold("W-logit device=True", info, case, res)
    host = hold("W-logit device=False", call(nhp, case), case, res)
    assert np.array_equal(dev == 0.0, host == 0.0)                      # the same structural zeros, bit for bit
    assert torch.equal(info.blocks, info.blocks.transpose(1, 2))


def test_automatic_tiling_beyond_the_lds_resident_block(nhp):
    case, res = ir.prepared("B-130")
    assert 8 * 261 * 262 // 2 > 160 * 1024
    hold("B-130", call(nhp, case), case, res)


# ------------------------------------------------------------------------------------------------- Hessian-vector product
def _kind_units(N, kinds, rng):
    """One unit vector per parameter kind (λ0, each impulse kind, W), at a random position of the kind."""
    P = N + kinds * N * N
    ks = [int(rng.integers(0, N))] + [N + q * N * N + int(rng.integers(0, N * N)) for q in range(kinds)]
    return ks, P


@pytest.mark.parametrize("name", WINDOWED + ["C", "C-net", "B-130"])
def test_hessian_vector_product(nhp, name):
    case, res = ir.prepared(name)
    N, kinds = case["N"], res.kinds
    proc = ir.process_of(nhp, case)
    data = (case["times"], case["nodes"], case["T"])
    rng = np.random.default_rng(11)
    ks, P = _kind_units(N, kinds, rng)
    m = cr.model_of(case)
    tails = [ir.window_tail(res, k, m, case["times"], case["nodes"]) for k in range(N)] if case["recursive"] else None

    def tail_of(v):
        out = np.zeros(P)
        if tails is not None:
            for k, c in enumerate(res.columns):
                idx = ir.block_index(N, kinds, c)
                out[idx] = tails[k] @ np.abs(v[idx])
        return out

    dense = None
    worst = 0.0
    for label, v in [("random", rng.normal(size=P))] + [("e_%d" % k, np.eye(1, P, k)[0]) for k in ks]:
        got = nhp.hessian_vector_product(proc, data, v, recursive=case["recursive"])
        want, B = ir.hvp(res, v, N)
        B = B + np.where(B > 0, tail_of(v), 0.0)
        err = np.abs(np.asarray(got - want, dtype=np.float64))
        bad = np.nonzero(np.where(B > 0, ~(err <= B), got != 0.0))[0]
        assert len(bad) == 0, (name, label, bad[:8], got[bad[:8]], np.asarray(want, dtype=np.float64)[bad[:8]], B[bad[:8]])
        worst = max(worst, float((err[B > 0] / B[B > 0]).max()) if (B > 0).any() else 0.0)
        if label != "random":                                           # ... and column k of the other kernel's dense block
            if dense is None:
                dense = call(nhp, case).blocks
            k = int(np.nonzero(v)[0][0])
            c = k if k < N else ((k - N) % (N * N)) // N
            idx = ir.block_index(N, kinds, c)
            r = list(idx).index(k)
            i = res.columns.index(c)
            tb = tails[i][:, r] if tails is not None else 0.0
            both = B[idx] + ir.bound(res, i)[:, r] + np.where(res.S[i][:, r] > 0, tb, 0.0)
            diff = np.abs(got[idx] + dense[c][:, r])
            assert np.all(diff <= both), (name, label, float((diff - both).max()))
            rest = np.ones(P, dtype=bool)
            rest[idx] = False
            assert np.all(got[rest] == 0.0)                             # the Hessian is block diagonal
    print(f"{name}: H·v error/bound {worst:.3g}")


def test_hessian_vector_product_on_the_device(nhp):
    import torch
    case, res = ir.prepared("W-net-logit")
    N = case["N"]
    P = N + 3 * N * N
    proc = ir.process_of(nhp, case)
    data = (case["times"], case["nodes"], case["T"])
    v = np.random.default_rng(5).normal(size=P)
    got = nhp.hessian_vector_product(proc, data, torch.as_tensor(v, device="cuda"), recursive=False, device=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    want, B = ir.hvp(res, v, N)
    err = np.abs(np.asarray(got.cpu().numpy() - want, dtype=np.float64))
    assert np.all(np.where(B > 0, err <= B, got.cpu().numpy() == 0.0))


# --------------------------------------------------------------------------------------------------------- regularize
@pytest.mark.parametrize("name", ["W-exp", "W-logit"])
def test_regularize_adds_the_priors_second_derivatives(nhp, name):
    case, _ = ir.prepared(name)
    case = dict(case, W=np.maximum(case["W"], 1e-3))                    # (the Gamma prior's curvature at W = 0 is infinite)
    N = case["N"]
    proc = ir.process_of(nhp, case)
    data = (case["times"], case["nodes"], case["T"])
    cols = [0, 3]
    res = ir.evaluate(cr.model_of(case), *data, columns=cols)
    plain = nhp.observed_information(proc, data, columns=cols, recursive=False)
    reg = nhp.observed_information(proc, data, columns=cols, recursive=False, regularize=True)
    b, w, imp = proc.baseline, proc.weights, proc.impulses
    for i, c in enumerate(cols):
        D = plain.blocks.shape[1]
        want = np.zeros((D, D))
        want[0, 0] = (b.α0 - 1.0) / b.λ[c] ** 2
        r = np.arange(N)
        if name == "W-exp":
            want[1 + r, 1 + r] = (imp.α - 1.0) / imp.θ[:, c] ** 2
            want[1 + N + r, 1 + N + r] = (w.κ - 1.0) / w.W[:, c] ** 2
        else:
            want[1 + r, 1 + r] = imp.κμ * imp.τ[:, c]
            want[1 + N + r, 1 + N + r] = (imp.α0 - 0.5) / imp.τ[:, c] ** 2
            want[1 + r, 1 + N + r] = want[1 + N + r, 1 + r] = imp.κμ * (imp.μ[:, c] - imp.μμ)
            want[1 + 2 * N + r, 1 + 2 * N + r] = (w.κ - 1.0) / w.W[:, c] ** 2
        # the two calls are two runs of the kernels: each is inside the reference's bound, so their difference is inside twice
        # that; the addition itself rounds once
        diff = reg.blocks[i] - plain.blocks[i]
        slack = 2.0 * ir.bound(res, i) + 2.0 ** -52 * (np.abs(reg.blocks[i]) + np.abs(want))
        assert np.all(np.abs(diff - want) <= slack), (name, c, np.abs(diff - want).max())
        assert np.all((diff == 0.0) | (want != 0.0) | (ir.bound(res, i) > 0))
    assert reg.ll == pytest.approx(plain.ll + nhp.logprior(proc), rel=1e-12)


# ---------------------------------------------------------------------------------------------------- standard errors
def test_standard_errors_at_the_true_parameters(nhp):
    from scipy.stats import norm
    lam0 = np.array([0.8, 1.2, 0.5])
    W = np.array([[.3, .1, .2], [.15, .25, .05], [.1, .2, .3]])
    theta = np.array([[2, 4, 3], [5, 2.5, 6], [3, 3.5, 2.0]])
    times, nodes, T = nhp.synthetic.branching_sample(lam0, W, theta, 1500.0, seed=1)
    assert len(times) == 8229
    N, dt_max = 3, 4.0

    def process(Wm):
        return nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0.copy()),
                                                   nhp.ExponentialImpulseResponse(theta.copy(), 1.0, 1.0, dt_max), nhp.DenseWeightModel(Wm.copy()))

    m = cr.model(lam0, W, theta=theta, dt_max=dt_max)
    res = ir.evaluate(m, times, nodes, T)
    grad = np.asarray(cr.evaluate(m, times, nodes, T).grad, dtype=np.float64)
    x = np.concatenate([lam0, theta.ravel(order="F"), W.ravel(order="F")])
    out = nhp.standard_errors(process(W), (times, nodes, T), recursive=False, level=0.9999)
    assert out.pd.tolist() == [True, True, True] and out.free.all()
    z = norm.ppf(0.5 + 0.5 * 0.9999)
    for c in range(N):
        J = np.asarray(res.blocks[c], dtype=np.float64)
        assert np.linalg.cond(J) <= 5.5e4
        idx = ir.block_index(N, 2, c)
        se = np.sqrt(np.diag(np.linalg.inv(J)))
        assert np.allclose(out.se[idx], se, rtol=1e-6, atol=0.0), (c, np.abs(out.se[idx] / se - 1).max())
        # the truth inside the 99.99 % Wald interval: of the call (centred at the parameters it was given), and of the
        # estimate one Newton step away, x + J⁻¹∇ll, built from the same standard errors
        assert np.all(out.lower_ci[idx] < x[idx]) and np.all(x[idx] < out.upper_ci[idx])
        assert np.allclose(out.upper_ci[idx] - x[idx], z * out.se[idx], rtol=1e-12)
        step = np.linalg.solve(J, grad[idx])
        assert np.all(np.abs(step) <= z * out.se[idx]), (c, np.abs(step / out.se[idx]).max())
    # one weight on the lower bound: it drops out of the free set with a NaN standard error, its column stays pd
    Wb = W.copy()
    Wb[1, 2] = 1e-6
    out = nhp.standard_errors(process(Wb), (times, nodes, T), recursive=False)
    k = N + N * N + 1 + 2 * N
    assert not out.free[k] and np.isnan(out.se[k]) and out.pd.tolist() == [True, True, True]
    assert out.free.sum() == len(x) - 1 and np.all(np.isfinite(out.se[np.arange(len(x)) != k]))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(nhp):
    from nhp_amd import _lib, continuous
    case, _ = ir.prepared("W-exp")
    N = case["N"]
    D, P = 1 + 2 * N, N + 2 * N * N
    proc = ir.process_of(nhp, case)
    ctx = nhp.default_context()
    data = (case["times"], case["nodes"], case["T"])
    ds = continuous.DeviceDataset(ctx, data, N, case["dt_max"])
    shard = continuous.DeviceDataset(ctx, data, N, case["dt_max"], columns=(0, 3))
    model = proc.device_model(ctx)
    lib = _lib.lib()
    i32p = C.POINTER(C.c_int32)

    def information(dset, flags=0, columns=None, tile=0):
        out, ll = np.full(N * D * D, np.nan), C.c_double(np.nan)
        cols = None if columns is None else np.asarray(columns, dtype=np.int32)
        rc = lib.nhp_cont_information(ctx.h, dset.h, model.h, flags, None if cols is None else cols.ctypes.data_as(i32p),
                                      0 if cols is None else len(cols), tile, 0, C.byref(ll), out.ctypes.data)
        return rc, out, ll.value, lib.nhp_last_error(ctx.h).decode()

    for kw, status in ((dict(dset=shard), _lib.ENOTIMPL), (dict(dset=ds, flags=3), _lib.ENOTIMPL), (dict(dset=ds, columns=[0, 7]), 1),
                       (dict(dset=ds, columns=[2, 2]), 1), (dict(dset=ds, tile=N + 1), 1), (dict(dset=ds, tile=-1), 1)):
        rc, out, ll, msg = information(**kw)
        assert rc == status and msg and np.all(np.isnan(out)) and np.isnan(ll), (kw, rc, msg)
    rc, out, ll, _ = information(ds, columns=[1])
    assert rc == 0 and np.all(np.isfinite(out[:D * D])) and np.all(np.isnan(out[D * D:])) and np.isfinite(ll)

    v, out = np.ones(P + 1), np.full(P + 1, np.nan)
    rc = lib.nhp_cont_hessian_vec(ctx.h, ds.h, model.h, 0, 0, v.ctypes.data, out.ctypes.data, P + 1)
    assert rc == 1 and np.all(np.isnan(out)) and b"length" in lib.nhp_last_error(ctx.h)
    rc = lib.nhp_cont_hessian_vec(ctx.h, shard.h, model.h, 0, 0, v.ctypes.data, out.ctypes.data, P)
    assert rc == _lib.ENOTIMPL and np.all(np.isnan(out))
    with pytest.raises(NotImplementedError):                            # an LGCP baseline, at the C ABI
        g = cr.CASES["G-W"]()
        gp = cr.process_of(nhp, g)
        gds = continuous.DeviceDataset(ctx, (g["times"], g["nodes"], g["T"]), g["N"], g["dt_max"])
        buf = np.full(N * D * D, np.nan)
        _lib.check(lib.nhp_cont_information(ctx.h, gds.h, gp.device_model(ctx).h, 0, None, 0, 0, 0, None, buf.ctypes.data), ctx.h)
    assert np.all(np.isnan(buf))
