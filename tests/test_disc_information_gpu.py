"""The discrete information kernels (csrc/disc_information.hip) against tests/disc_information_ref.py (long double).

Bounds, derived in disc_information_ref.block_bound / hv_bound and shown attainable by a plain float64 evaluation in
tests/test_disc_information_host.py:
    every block entry   |J - J_ref| <= (2·N·B + n_t + 48)·2⁻⁵³·J_ref     (an entry with no term is an exact zero)
    every entry of J·v  |.| <= (3·N·B + n_t + 64)·2⁻⁵³·S_hv
Every case also asks: blocks exactly symmetric, bitwise identical across two calls, ll equal to disc_loglikelihood's.

Cases (both kinds unless noted), on the inputs of tests/disc_edge_cases.py:
    one_element       N=1   T=1    B=1   D = 2, T < L
    k_below_bk        N=3   T=17   B=2   D = 7, less than one MFMA fragment; T one over a 16-bin chunk
    ragged            N=17  T=129  B=5   D = 86: automatic (one tile of 96 rows, one slab), tile_rows=32 (tiles of 32, 32, 22
                                         rows: six tile pairs) and slab_bins=48 (three slabs, the last of 33 bins)
    one_column_over   N=129 T=65   B=2   D = 259: three tiles of 96, 96, 67 rows, all columns
    two_column_tiles  N=130 T=997  B=2   D = 261, columns [0, 77, 129] only (the long-double reference of all 130 columns
                                         would take a minute)
    C2  all_zero, one_bin, half, every_bin   N=5 T=300 B=3   the chunk list empty, of one entry, about full, full
    C3  max_255, with_256, huge              N=2 T=192 B=2   weights spanning ten orders of magnitude
    sparse_runs (made here)  N=4 T=1000 B=2  events only in bins {0, 15, 16, 511, 999}: the chunk list at its first, last
                                         and adjacent chunks; also with slab_bins=256 (bin 511 closes a slab, 999 sits in
                                         the short last chunk of the last slab)

disc_standard_errors: `se` against the inverse of the reference's blocks within 64·cond·2⁻⁵³ relative, cond the 2-norm
condition number of the column's free sub-block of the reference.  fd_shape: cond = 1.2e3 to 1.4e3 (both kinds), the check
asks for 1e-11.  ragged, Fisher: cond = 2.5e7 to 2.7e7, the check asks for 1.9e-7.  ragged, OBSERVED: a column has
n_t = about 43 bins with an event and D = 86 parameters, so its block has rank <= n_t < D and cond = 1e19 or more: no
inverse exists and no tolerance means anything, so that combination is run only for `pd` being reported without an exception.

Largest error / bound on an MI355X, per case: see DESIGN.md section 3.17.
"""
import ctypes as C

import numpy as np
import pytest

import disc_edge_cases as cases
import disc_grad_ref as ref
import disc_information_ref as ir

pytestmark = pytest.mark.gpu


def process(nhp, c):
    dt, L = c["dt"], c["phi"].shape[0]
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(c["lam0"].copy(), dt),
                                             nhp.DiscreteGaussianImpulseResponse(c["theta"].copy(), L, dt),
                                             nhp.DenseWeightModel(c["W"].copy()), dt)
    assert np.array_equal(proc.impulses.basis(), c["phi"])
    return proc


SPARSE_BINS = (0, 15, 16, 511, 999)
_made = {}


def sparse_runs(orc):
    """N = 4, T = 1000, B = 2, L = 5: column 0 holds an event in each of the five bins, column 1 in the first and the last
    bin only, column 2 in the adjacent chunks' bins 15 and 16, column 3 none."""
    if "sparse_runs" not in _made:
        N, T, B, L = 4, 1000, 2, 5
        rng = np.random.default_rng(4000)
        c = cases._model(orc, rng, N, B, L, 1.0)
        data = np.zeros((N, T), dtype=np.int64)
        data[0, list(SPARSE_BINS)] = [1, 2, 1, 3, 1]
        data[1, [0, 999]] = [2, 1]
        data[2, [15, 16]] = [1, 1]
        c["data"] = data
        _made["sparse_runs"] = c
    return _made["sparse_runs"]


def case_and_reference(orc, name, kind, columns):
    if name == "sparse_runs":
        c = sparse_runs(orc)
        key = (name, kind, columns)
        if key not in _made:
            _made[key] = ir.evaluate(c, kind, columns=columns)
        return c, _made[key]
    return cases.case(orc, name), ir.reference(orc, name, kind, columns)


def held_to_the_reference(nhp, orc, name, kind, columns=None, **tiling):
    """Blocks of one kind against the reference, with the checks every case asks for; returns (info, reference, dataset)."""
    c, res = case_and_reference(orc, name, kind, columns)
    N, T = c["data"].shape
    B = c["phi"].shape[1]
    D = 1 + N * B
    proc = process(nhp, c)
    ds = nhp.convolve(proc, c["data"])
    cols = None if columns is None else list(columns)
    info = nhp.disc_observed_information(proc, convolved=ds, columns=cols, kind=kind, **tiling)
    again = nhp.disc_observed_information(proc, convolved=ds, columns=cols, kind=kind, **tiling)
    J = np.asarray(info.blocks)
    assert J.shape == (len(res.columns), D, D) and info.kind == kind and list(info.columns) == res.columns
    assert len(info.names) == D and info.names[0] == ("λ0", None, None) and info.names[1 + (B - 1) * N + (N - 1)] == ("η", N - 1, B - 1)
    ratio, bad = ir.check_blocks(J, res, N, B)
    print(f"[{name}/{kind}{'/' + str(tiling) if tiling else ''}] blocks error / bound {ratio:.3g}  (n_t {res.n_t.min()}..{res.n_t.max()})")
    assert np.all(np.isfinite(J))
    assert np.array_equal(J, J.transpose(0, 2, 1)), "blocks are not exactly symmetric"
    assert np.array_equal(J, np.asarray(again.blocks)), "blocks differ between two calls"
    assert info.ll == nhp.loglikelihood(proc, c["data"], convolved=ds) == again.ll
    assert len(bad) == 0, (name, kind, bad[:5], ratio)
    assert np.all(J[np.asarray(res.blocks, dtype=np.float64) == 0.0] == 0.0)
    return info, res, (proc, ds, c)


def product_held_to_the_reference(nhp, name, kind, res, proc, ds, c, info):
    """J·v against the reference within hv_bound, and against blocks[k] @ v_c within the sum of both bounds: a random v and
    the unit vector on λ0[0]."""
    N, T = c["data"].shape
    B = c["phi"].shape[1]
    P = N + N * N * B
    unit = np.zeros(P)
    unit[0] = 1.0
    J = np.asarray(info.blocks)
    for label, v in (("random", np.random.default_rng(11).normal(size=P)), ("unit", unit)):
        got = nhp.disc_hessian_vector_product(proc, convolved=ds, v=v, kind=kind)
        want, scale, n_t = ir.hvp(res, v, N, B)
        bound = ir.hv_bound(N, B, n_t, scale)
        err = np.abs(ref.backend().arr(got) - want).astype(np.float64)
        pos = bound > 0
        print(f"[{name}/{kind}] J·v ({label}) error / bound {float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0:.3g}")
        assert np.all(err <= bound), (name, kind, label, np.argwhere(err > bound)[:5])
        for k, col in enumerate(res.columns):
            idx = ir.block_index(N, B, col)
            both = bound[idx] + ir.block_bound(N, B, res.n_t[k], np.asarray(res.blocks[k], dtype=np.float64)) @ np.abs(v[idx])
            assert np.all(np.abs(J[k] @ v[idx] - got[idx]) <= both + (len(idx) + 2) * 2.0 ** -53 * np.abs(J[k]) @ np.abs(v[idx]))    # (+ the host product's own rounding)
        if label == "unit":
            assert np.all(got[1:N] == 0.0)                       # the information is block diagonal by child node


RUNS = [("one_element", None, {}), ("k_below_bk", None, {}), ("ragged", None, {}), ("ragged", None, {"tile_rows": 32}),
        ("ragged", None, {"slab_bins": 48}), ("one_column_over", None, {}), ("two_column_tiles", (0, 77, 129), {})]
RUNS += [(n, None, {}) for n in cases.C2 + cases.C3] + [("sparse_runs", None, {}), ("sparse_runs", None, {"slab_bins": 256})]


@pytest.mark.parametrize("kind", ir.KINDS)
@pytest.mark.parametrize("name,columns,tiling", RUNS, ids=[n + "".join(f"-{k}{v}" for k, v in t.items()) for n, _, t in RUNS])
def test_blocks_equal_the_reference(nhp, orc, name, columns, tiling, kind):
    info, res, (proc, ds, c) = held_to_the_reference(nhp, orc, name, kind, columns, **tiling)
    N = c["data"].shape[0]
    J = np.asarray(info.blocks)
    if columns is None and N <= 17 and not tiling:
        product_held_to_the_reference(nhp, name, kind, res, proc, ds, c, info)
    if name == "all_zero":
        se = nhp.disc_standard_errors(proc, convolved=ds, kind=kind)
        if kind == "observed":
            assert np.all(J == 0.0) and not se.pd.any() and np.all(np.isnan(se.se)) and not se.free.any()
        else:
            assert np.all(J[:, 0, 0] > 0.0) and np.all(J[:, 1:, :] == 0.0)       # (no event anywhere: Ŝ = 0, only the λ0 entry has terms)
    if name == "one_bin" and kind == "observed":
        assert np.all(J[[0, 1, 2, 4]] == 0.0) and np.linalg.matrix_rank(J[3]) == 1
    if name == "half":
        assert 0.4 < np.count_nonzero(c["data"]) / c["data"].size < 0.6
    if name == "every_bin":
        assert np.count_nonzero(c["data"]) == c["data"].size
    if name == "sparse_runs" and kind == "observed":
        assert np.all(J[3] == 0.0) and [int(n) for n in res.n_t] == [5, 2, 2, 0]
        assert np.count_nonzero(c["data"]) == 9 and set(np.flatnonzero(c["data"].any(axis=0))) == set(SPARSE_BINS)


@pytest.mark.parametrize("kind", ir.KINDS)
def test_a_column_subset_in_any_order_gives_the_blocks_of_the_full_call(nhp, orc, kind):
    c = cases.case(orc, "ragged")
    proc = process(nhp, c)
    ds = nhp.convolve(proc, c["data"])
    full = nhp.disc_observed_information(proc, convolved=ds, kind=kind, slab_bins=64)      # (the same tiling in both calls)
    some = nhp.disc_observed_information(proc, convolved=ds, kind=kind, slab_bins=64, columns=[16, 0, 5])
    assert list(some.columns) == [16, 0, 5] and some.ll == full.ll
    assert np.array_equal(np.asarray(some.blocks), np.asarray(full.blocks)[[16, 0, 5]])
    held_to_the_reference(nhp, orc, "ragged", kind, (16, 0, 5))


def test_device_outputs_are_device_tensors_with_the_same_values(nhp, orc):
    import torch
    c = cases.case(orc, "k_below_bk")
    N, T = c["data"].shape
    B = c["phi"].shape[1]
    proc = process(nhp, c)
    ds = nhp.convolve(proc, c["data"])
    for kind in ir.KINDS:
        host = nhp.disc_observed_information(proc, convolved=ds, kind=kind)
        dev = nhp.disc_observed_information(proc, convolved=ds, kind=kind, device=True)
        assert isinstance(dev.blocks, torch.Tensor) and dev.blocks.is_cuda and dev.blocks.dtype == torch.float64
        assert np.array_equal(dev.blocks.cpu().numpy(), np.asarray(host.blocks)) and dev.ll == host.ll
        v = np.random.default_rng(2).normal(size=N + N * N * B)
        out = nhp.disc_hessian_vector_product(proc, convolved=ds, v=torch.as_tensor(v, device=dev.blocks.device), kind=kind, device=True)
        assert isinstance(out, torch.Tensor) and out.is_cuda
        assert np.array_equal(out.cpu().numpy(), nhp.disc_hessian_vector_product(proc, convolved=ds, v=v, kind=kind))
        with pytest.raises(ValueError):
            nhp.disc_hessian_vector_product(proc, convolved=ds, v=v, kind=kind, device=True)


def test_refusals(nhp, orc):
    from nhp_amd import _lib
    c = cases.case(orc, "lgcp")
    lgcp = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteLogGaussianCoxProcess(c["grid_x"].copy(), c["lam_grid"].copy(), None, -1.0, c["dt"]),
                                             nhp.DiscreteGaussianImpulseResponse(c["theta"].copy(), c["phi"].shape[0], c["dt"]),
                                             nhp.DenseWeightModel(c["W"].copy()), c["dt"])
    N, T = c["data"].shape
    B = c["phi"].shape[1]
    P = N + N * N * B
    with pytest.raises(NotImplementedError):
        nhp.disc_observed_information(lgcp, c["data"])
    with pytest.raises(NotImplementedError):
        nhp.disc_hessian_vector_product(lgcp, c["data"], v=np.zeros(P))
    with pytest.raises(NotImplementedError):
        nhp.disc_standard_errors(lgcp, c["data"])
    # the library's own refusal: lambda0 == NULL with a grid attached is NHP_ENOTIMPL, and nothing is written
    ctx = _lib.default_context()
    ds = nhp.convolve(lgcp, c["data"])
    lgcp.baseline.attach(ds)
    _, W, th, _ = lgcp._lowered()
    out = np.full(1 + N * B, -7.0)
    ll = C.c_double(-7.0)
    col = np.zeros(1, dtype=np.int32)
    colp = col.ctypes.data_as(C.POINTER(C.c_int32))
    rc = _lib.lib().nhp_disc_information(ctx.h, ds.h, None, _lib.dptr(W), _lib.dptr(th), c["dt"], 0, colp, 1, 0, 0, C.byref(ll), out.ctypes.data)
    assert rc == _lib.ENOTIMPL and b"LGCP" in _lib.lib().nhp_last_error(ctx.h) and np.all(out == -7.0) and ll.value == -7.0
    rc = _lib.lib().nhp_disc_hessian_vec(ctx.h, ds.h, None, _lib.dptr(W), _lib.dptr(th), c["dt"], 0, out.ctypes.data, out.ctypes.data)
    assert rc == _lib.ENOTIMPL
    # a repeated or out-of-range column
    k = cases.case(orc, "k_below_bk")
    proc = process(nhp, k)
    kds = nhp.convolve(proc, k["data"])
    for bad in ([0, 0], [3], [-1]):
        with pytest.raises(ValueError):
            nhp.disc_observed_information(proc, convolved=kds, columns=bad)
    l0, W, th, _ = proc._lowered()
    blocks = np.full((2, 7, 7), -7.0)
    for bad in ([1, 1], [0, 3]):
        col = np.array(bad, dtype=np.int32)
        rc = _lib.lib().nhp_disc_information(ctx.h, kds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), k["dt"], 0,
                                             col.ctypes.data_as(C.POINTER(C.c_int32)), 2, 0, 0, C.byref(ll), blocks.ctypes.data)
        assert rc == _lib.EDOMAIN and b"repeated" in _lib.lib().nhp_last_error(ctx.h) and np.all(blocks == -7.0)
    with pytest.raises(nhp.NhpError, match="multiple of 16"):
        nhp.disc_observed_information(proc, convolved=kds, tile_rows=24)
    # a network process is not what mle! fits
    net = nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(k["lam0"].copy(), k["dt"]),
                                           nhp.DiscreteGaussianImpulseResponse(k["theta"].copy(), k["phi"].shape[0], k["dt"]),
                                           nhp.DenseWeightModel(k["W"].copy()), np.ones((3, 3)), nhp.DenseNetworkModel(3), k["dt"])
    with pytest.raises(TypeError):
        nhp.disc_observed_information(net, k["data"])
    with pytest.raises(TypeError):
        nhp.disc_standard_errors(net, k["data"])
    # the context goes on working
    assert np.all(np.isfinite(np.asarray(nhp.disc_observed_information(proc, convolved=kds).blocks)))


def reference_standard_errors(res, x, N, B, lower, upper):
    """se [P] from the inverse of the reference's blocks over the free parameters, and the largest condition number."""
    se = np.full(len(x), np.nan)
    worst = 0.0
    for k, col in enumerate(res.columns):
        idx = ir.block_index(N, B, col)
        J = np.asarray(res.blocks[k], dtype=np.float64)
        f = (x[idx] > lower) & (x[idx] < upper) & np.any(J != 0.0, axis=1)
        sub = J[np.ix_(f, f)]
        worst = max(worst, float(np.linalg.cond(sub)))
        se[idx[f]] = np.sqrt(np.diag(np.linalg.inv(sub)))
    return se, worst


@pytest.mark.parametrize("name,kind", [("fd_shape", "observed"), ("fd_shape", "fisher"), ("ragged", "fisher")])
def test_standard_errors_equal_the_inverse_of_the_reference_blocks(nhp, orc, name, kind):
    c = cases.case(orc, name)
    N, T = c["data"].shape
    B = c["phi"].shape[1]
    res = ir.reference(orc, name, kind, None)
    proc = process(nhp, c)
    x = proc.params()
    out = nhp.disc_standard_errors(proc, c["data"], kind=kind)
    assert out.pd.all() and out.se.shape == x.shape
    worst, worst_cond = 0.0, 0.0
    for k, col in enumerate(res.columns):
        idx = ir.block_index(N, B, col)
        J = np.asarray(res.blocks[k], dtype=np.float64)
        f = (x[idx] > 1e-6) & (x[idx] < 10.0) & np.any(J != 0.0, axis=1)
        assert np.array_equal(out.free[idx], f) and np.all(np.isnan(out.se[idx[~f]])) and f.sum() >= len(idx) - 2
        sub = J[np.ix_(f, f)]
        cond = float(np.linalg.cond(sub))
        want = np.sqrt(np.diag(np.linalg.inv(sub)))
        rel = np.abs(out.se[idx[f]] - want) / want
        worst, worst_cond = max(worst, float(rel.max() / (64 * cond * 2.0 ** -53))), max(worst_cond, cond)
        assert np.all(rel <= 64 * cond * 2.0 ** -53), (name, kind, col, float(rel.max()), cond)
    print(f"[{name}/{kind}] se error / (64·cond·2^-53) {worst:.3g}, largest cond {worst_cond:.3g}")
    assert worst_cond < (1e4 if name == "fd_shape" else 1e8)                   # small enough for the check to mean something
    z = 1.959963984540054
    fr = out.free
    assert np.allclose((out.upper_ci - x)[fr], z * out.se[fr], rtol=1e-12) and np.allclose((x - out.lower_ci)[fr], z * out.se[fr], rtol=1e-12)
    # se_W: the explicit quadratic form over the link's B rows of the reference's inverse
    free_links = [(p, col) for col in range(N) for p in range(N) if out.free[ir.block_index(N, B, col)].all()][:3]
    for p, col in free_links:
        cov = np.linalg.inv(np.asarray(res.blocks[col], dtype=np.float64))
        rows = 1 + np.arange(B) * N + p
        assert np.isclose(out.se_W[p, col], np.sqrt(cov[np.ix_(rows, rows)].sum()), rtol=1e-5)
    assert np.all(np.isfinite(out.se_W)) and np.all(np.isfinite(out.se_theta)) and np.all(out.se_theta >= 0.0)


def test_a_parameter_on_the_bound_is_excluded(nhp, orc):
    """fd_shape with λ0[1] set to `lower`: not free, NaN, and the rest of its column is the inverse over the others."""
    c = dict(cases.case(orc, "fd_shape"))
    c["lam0"] = c["lam0"].copy()
    c["lam0"][1] = 1e-6
    N, T = c["data"].shape
    B = c["phi"].shape[1]
    res = ir.evaluate(c, "observed")
    proc = process(nhp, c)
    x = proc.params()
    out = nhp.disc_standard_errors(proc, c["data"], lower=1e-6)
    want, cond = reference_standard_errors(res, x, N, B, 1e-6, 10.0)
    assert not out.free[1] and np.isnan(out.se[1]) and np.isnan(out.lower_ci[1]) and out.pd.all()
    assert out.free.sum() == len(x) - 1 and np.array_equal(np.isnan(out.se), np.isnan(want))
    ok = ~np.isnan(want)
    rel = np.abs(out.se[ok] - want[ok]) / want[ok]
    print(f"[fd_shape, λ0[1] on the bound] se error / (64·cond·2^-53) {float(rel.max() / (64 * cond * 2.0 ** -53)):.3g}, cond {cond:.3g}")
    assert np.all(rel <= 64 * cond * 2.0 ** -53) and cond < 1e6


def test_a_rank_deficient_observed_block_reports_pd_without_an_exception(nhp, orc):
    """ragged, observed: n_t < D in every column, so no column's block has an inverse (see the module docstring)."""
    c = cases.case(orc, "ragged")
    res = ir.reference(orc, "ragged", "observed", None)
    assert res.n_t.max() < 1 + 17 * 5
    out = nhp.disc_standard_errors(process(nhp, c), c["data"])
    assert out.pd.dtype == bool and out.pd.shape == (17,)
    assert np.all(np.isnan(out.se[~out.free]))
