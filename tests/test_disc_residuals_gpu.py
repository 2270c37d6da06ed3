"""disc_residuals / disc_goodness_of_fit on the device: nhp_disc_residuals (csrc/disc_residuals.hip).

The reference of the cell values is the numpy restatement (tests/disc_residuals_ref.py, written from include/nhp.h; held to
60-digit mpmath by tests/test_disc_residuals_host.py) evaluated at the GPU's OWN disc_intensity output, which the oracle
tests hold to 1e-12: what is compared here is the new kernels alone.

Tolerances: pit 1e-12 absolute, pearson 1e-12 relative (the project's parity tolerance of the discrete intensity); expected,
chi2, deviance and cumulative 1e-12 relative to the node's total against numpy sums of the reference planes; observed,
histogram and impossible exactly.  Shapes: T below, astride and past the 256 threads of a workgroup and the 1024 bins of a
workgroup's chunk (the residual pass and the scan share it), three chunks (scan offsets past the first), and more histogram
bins than a workgroup has threads.  Statistical bounds and seeds are those of the host file, pre-checked there."""
import ctypes as C

import numpy as np
import pytest

import disc_residuals_ref as rr
import disc_simulate_ref as dr

pytestmark = pytest.mark.gpu

TOL = 1e-12


def counts_for(N, T, seed, rate=0.4):
    return np.random.default_rng(seed).poisson(rate, (N, T)).astype(np.int64)


def compare(nhp, p, counts, seed, nbins=20, label=""):
    """disc_residuals with every plane against the restatement at the GPU's own intensity -> (result, reference)."""
    lam = nhp.intensity(p, counts)
    ref = rr.residuals(counts, lam, seed, nbins)
    got = nhp.disc_residuals(p, counts, seed=seed, nbins=nbins, pit=True, pearson=True, cumulative=True)
    N, T = counts.shape
    assert got.pit.shape == got.pearson.shape == got.cumulative.shape == (N, T) and got.histogram.shape == (N, nbins)
    fin = np.isfinite(ref["pearson"])
    e_pit = np.abs(got.pit - ref["pit"]).max()
    e_pe = (np.abs(got.pearson[fin] - ref["pearson"][fin]) / np.maximum(np.abs(ref["pearson"][fin]), 1e-300)).max() if fin.any() else 0.0
    total = np.maximum(ref["expected"], 1e-300)
    e_cum = (np.abs(got.cumulative - ref["cumulative"]).max(axis=1) / total).max()
    print(f"{label}: max |pit - ref| = {e_pit:.3g}, max rel pearson = {e_pe:.3g}, max rel cumulative = {e_cum:.3g}")
    assert np.all((got.pit >= 0.0) & (got.pit <= 1.0))
    assert e_pit <= TOL and e_pe <= TOL and e_cum <= TOL
    assert np.array_equal(got.pearson[~fin], ref["pearson"][~fin])
    for k in ("expected", "chi2", "deviance"):
        want = ref[k]
        f = np.isfinite(want)
        err = np.abs(getattr(got, k)[f] - want[f]) / np.maximum(np.abs(want[f]), 1e-300)
        print(f"{label}: max rel {k} = {err.max() if f.any() else 0.0:.3g}")
        assert np.all(err <= TOL) and np.array_equal(getattr(got, k)[~f], want[~f])
    assert got.observed.dtype == np.int64 and np.array_equal(got.observed, ref["observed"])
    assert got.histogram.dtype == np.int64 and np.array_equal(got.histogram, ref["histogram"])
    assert np.all(got.histogram.sum(axis=1) == T)
    assert got.impossible == ref["impossible"]
    return got, ref


SHAPES = [(1, 1, 1, 1, 20), (3, 257, 2, 4, 20), (5, 1025, 3, 4, 20), (64, 300, 2, 3, 300), (2, 2500, 2, 3, 7)]


@pytest.mark.parametrize("N,T,B,L,nbins", SHAPES)
def test_against_the_restatement(nhp, N, T, B, L, nbins):
    p = dr.make(nhp, N, L=L, B=B, seed=N)
    compare(nhp, p, counts_for(N, T, T), seed=N + T, nbins=nbins, label=f"N={N} T={T} B={B} L={L}")


def test_network_process_with_zeros_in_A(nhp):
    p = dr.make(nhp, 5, seed=2, network=True, dt=0.5)
    assert np.any(p.adjacency_matrix == 0.0)
    compare(nhp, p, counts_for(5, 300, 1), seed=3, label="network")


def test_lgcp_baseline(nhp):
    p = dr.make(nhp, 5, seed=4, lgcp_T=300)
    compare(nhp, p, counts_for(5, 300, 2), seed=4, label="LGCP")


def crafted(nhp):
    """Node 0: λ0 = 0 and no incoming weight (μ = 0 exactly); node 1: μ = 2500 exactly; node 2: driven by node 1, μ near 10."""
    p = dr.make(nhp, 3, L=4, B=3, seed=9)
    p.baseline = nhp.DiscreteHomogeneousProcess(np.array([0.0, 2500.0, 7.3]), 1.0)
    W = np.zeros((3, 3))
    W[1, 2] = 0.001
    p.weights = nhp.DenseWeightModel(W)
    T = 40
    counts = np.zeros((3, T), dtype=np.int64)
    counts[0, 17] = 1                                 # the impossible cell
    counts[1] = np.random.default_rng(3).poisson(2500.0, T)
    counts[1, :3] = (2400, 2500, 2600)
    lam = nhp.intensity(p, counts)                    # node 2 drives nothing: its counts may follow its own means
    counts[2] = np.floor(lam[:, 2]).astype(np.int64) + (np.arange(T) % 2)      # s = ⌊μ⌋ and ⌊μ⌋ + 1: both tails
    counts[2, 30:34] = (15, 16, 17, 30)               # the Stirling error's table / series switch, and a far count
    return p, counts


def test_crafted_cells(nhp):
    p, counts = crafted(nhp)
    got, ref = compare(nhp, p, counts, seed=11, label="crafted")
    lam = nhp.intensity(p, counts)
    assert np.all(lam[:, 0] == 0.0) and np.all(lam[:, 1] == 2500.0)
    assert got.impossible == 1 and got.pit[0, 17] == 1.0 and np.isposinf(got.pearson[0, 17]) and np.isposinf(got.chi2[0])
    v = rr.uniforms(3, counts.shape[1], 11)
    quiet = np.arange(counts.shape[1]) != 17
    assert np.array_equal(got.pit[0, quiet], v[quiet, 0]) and np.all(got.pearson[0, quiet] == 0.0)      # μ = 0, s = 0: pit = v
    assert got.deviance[0] == 0.0 and got.expected[0] == 0.0 and got.observed[0] == 1
    assert np.array_equal(got.pearson[1, :3], np.array([-2.0, 0.0, 2.0]))
    s2, m2 = counts[2, :30].astype(float), lam[:30, 2]
    assert np.all((s2 <= m2) == (np.arange(30) % 2 == 0))


def test_determinism_and_seed(nhp):
    p = dr.make(nhp, 5, seed=5)
    counts = counts_for(5, 1025, 8)
    kw = dict(pit=True, pearson=True, cumulative=True)
    a, b, c = (nhp.disc_residuals(p, counts, seed=s, **kw) for s in (7, 7, 8))
    for k in ("pit", "pearson", "cumulative", "expected", "observed", "chi2", "deviance", "histogram"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
        if k not in ("pit", "histogram"):
            assert np.array_equal(getattr(a, k), getattr(c, k)), k
    assert not np.array_equal(a.pit, c.pit) and a.impossible == b.impossible == c.impossible == 0
    # an absent plane changes nothing else
    d = nhp.disc_residuals(p, counts, seed=7, pit=False)
    assert d.pit is None and d.pearson is None and d.cumulative is None
    for k in ("expected", "observed", "chi2", "deviance", "histogram"):
        assert np.array_equal(getattr(a, k), getattr(d, k)), k


def test_device_results_equal_host_results(nhp):
    import torch
    p = dr.make(nhp, 5, seed=5)
    counts = counts_for(5, 1025, 8)
    kw = dict(seed=7, nbins=33, pit=True, pearson=True, cumulative=True)
    h, d = nhp.disc_residuals(p, counts, **kw), nhp.disc_residuals(p, counts, device=True, **kw)
    for k in ("pit", "pearson", "cumulative", "expected", "observed", "chi2", "deviance", "histogram"):
        x = getattr(d, k)
        assert isinstance(x, torch.Tensor) and x.is_cuda and tuple(x.shape) == getattr(h, k).shape
        assert np.array_equal(x.cpu().numpy(), getattr(h, k)), k
    assert d.impossible == h.impossible
    g_h, g_d = nhp.disc_goodness_of_fit(p, residuals=h), nhp.disc_goodness_of_fit(p, residuals=d)
    assert g_h.statistic == pytest.approx(g_d.statistic, abs=1e-15) and np.allclose(g_h.node_statistic, g_d.node_statistic, atol=1e-15)
    assert g_h.histogram_pvalue == g_d.histogram_pvalue and np.array_equal(g_h.dispersion, g_d.dispersion)


@pytest.mark.parametrize("on_device", [False, True])
def test_planes_not_requested_are_not_written(nhp, on_device):
    """A direct ABI call with pit alone, its plane the first third of a buffer filled with a sentinel: the rest stays."""
    import torch
    from nhp_amd import _lib
    from nhp_amd.discrete import convolve
    ctx = nhp.default_context()
    p = dr.make(nhp, 3, seed=1)
    counts = counts_for(3, 257, 4)
    N, T, nbins = 3, 257, 20
    ds = convolve(p, counts, ctx)
    l0, W, th, A = p._lowered()
    SENT = -12345.5
    if on_device:
        dev = torch.device("cuda", ctx.device)
        planes = torch.full((3, N * T), SENT, dtype=torch.float64, device=dev)
        ex, chi, dv = (torch.full((N + 1,), SENT, dtype=torch.float64, device=dev) for _ in range(3))
        ob = torch.full((N + 1,), -7, dtype=torch.int64, device=dev)
        hist = torch.full((N * nbins + 1,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ptr = lambda x: x.data_ptr()
        host = lambda x: x.cpu().numpy()
    else:
        planes = np.full((3, N * T), SENT)
        ex, chi, dv = (np.full(N + 1, SENT) for _ in range(3))
        ob, hist = np.full(N + 1, -7, dtype=np.int64), np.full(N * nbins + 1, -7, dtype=np.int64)
        ptr = lambda x: x.ctypes.data
        host = np.asarray
    imp = C.c_int64(-1)
    _lib.check(_lib.lib().nhp_disc_residuals(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A), p.dt, 5, nbins,
                                             1 if on_device else 0, ptr(planes), None, None, ptr(ex), ptr(ob), ptr(chi), ptr(dv),
                                             ptr(hist), C.byref(imp), None), ctx.h)
    pl = host(planes)
    want = nhp.disc_residuals(p, counts, seed=5, nbins=nbins)
    assert np.array_equal(pl[0].reshape(N, T), want.pit) and np.all(pl[1:] == SENT)
    assert np.array_equal(host(ex)[:N], want.expected) and host(ex)[N] == SENT and host(chi)[N] == SENT and host(dv)[N] == SENT
    assert np.array_equal(host(ob)[:N], want.observed) and host(ob)[N] == -7
    assert np.array_equal(host(hist)[:-1].reshape(N, nbins), want.histogram) and host(hist)[-1] == -7 and imp.value == 0


def test_errors_leave_the_context_usable(nhp):
    from nhp_amd import DomainError
    ctx = nhp.default_context()
    p = dr.make(nhp, 3, seed=1)
    counts = counts_for(3, 40, 4)
    good = nhp.disc_residuals(p, counts, seed=1, ctx=ctx)

    def still_works():
        again = nhp.disc_residuals(p, counts, seed=1, ctx=ctx)
        assert np.array_equal(again.pit, good.pit) and np.array_equal(again.histogram, good.histogram)

    huge = dr.make(nhp, 3, seed=1)
    huge.baseline = nhp.DiscreteHomogeneousProcess(np.array([0.1, 2.0 ** 20 + 1.0, 0.1]), 1.0)
    with pytest.raises(NotImplementedError):
        nhp.disc_residuals(huge, counts, ctx=ctx)
    still_works()
    big_count = counts.copy()
    big_count[2, 5] = 2 ** 20 + 1
    quiet = dr.make(nhp, 3, seed=1, scale=0.0)
    with pytest.raises(NotImplementedError):
        nhp.disc_residuals(quiet, big_count, ctx=ctx)
    still_works()
    for bad in (-0.5, np.nan, np.inf):
        q = dr.make(nhp, 3, seed=1)
        q.baseline.λ = np.array([0.1, bad, 0.1])
        with pytest.raises(DomainError):
            nhp.disc_residuals(q, counts, ctx=ctx)
        still_works()
    with pytest.raises(ValueError):
        nhp.disc_residuals(p, counts, nbins=0, ctx=ctx)
    still_works()
    cont = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.ones(2)), nhp.ExponentialImpulseResponse(np.ones((2, 2))),
                                               nhp.DenseWeightModel(np.full((2, 2), 0.1)))
    with pytest.raises(TypeError):
        nhp.disc_residuals(cont, counts[:2], ctx=ctx)
    still_works()


@pytest.fixture(scope="module")
def stat_data(nhp):
    p = rr.stat_process(nhp)
    return p, nhp.disc_rand(p, rr.STAT_T, rr.STAT_DATA_SEED)


def test_true_model_passes(nhp, stat_data):
    p, counts = stat_data
    g = nhp.disc_goodness_of_fit(p, counts, seed=rr.STAT_SEED)
    print(f"true model: {g}; node p {g.node_pvalue}; dispersion {g.dispersion}; expected {g.expected} observed {g.observed}")
    assert g.pvalue > rr.KS_TRUE_MIN and g.histogram_pvalue > rr.KS_TRUE_MIN
    assert np.all(np.abs(g.dispersion - 1.0) <= rr.DISPERSION_TOL)
    assert g.impossible == 0 and np.array_equal(g.observed, counts.sum(axis=1))
    # the product's statistics against the host file's own
    r = nhp.disc_residuals(p, counts, seed=rr.STAT_SEED)
    d, pv = rr.ks_uniform(r.pit)
    assert g.statistic == pytest.approx(d, abs=1e-15) and g.pvalue == pytest.approx(pv, rel=1e-9)
    assert g.histogram_pvalue == pytest.approx(rr.histogram_pvalue(r.histogram), rel=1e-12)


def test_wrong_model_fails(nhp, stat_data):
    p, counts = stat_data
    g = nhp.disc_goodness_of_fit(rr.wrong(p), counts, seed=rr.STAT_SEED, device=True)
    print(f"weights x 1.5: {g}; dispersion {g.dispersion}")
    assert g.pvalue < rr.KS_WRONG_MAX and g.histogram_pvalue < rr.KS_WRONG_MAX
