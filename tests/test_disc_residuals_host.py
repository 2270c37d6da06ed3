"""disc_residuals / disc_goodness_of_fit without a GPU: the export and the argument errors raised before any device work, the
numpy restatement of nhp_disc_residuals (tests/disc_residuals_ref.py) against 60-digit mpmath on the grid of cells, the naive
log-gamma pmf failing the same bound (so the restatement cannot be quietly swapped for it), and the statistical checks of
tests/test_disc_residuals_gpu.py run on the restatement with the same seeds: a correct implementation passes them."""
import numpy as np
import pytest

import disc_residuals_ref as rr
import disc_simulate_ref as dr

# 1e-14 absolute: four times the 2.4e-15 the restatement was measured at on this grid against mpmath
EXACT_TOL = 1e-14


def test_exports_and_errors_before_any_device_work(nhp):
    from nhp_amd import _lib
    assert callable(nhp.disc_residuals) and callable(nhp.disc_goodness_of_fit)
    assert hasattr(_lib.lib(), "nhp_disc_residuals")
    assert "uniform" in nhp.disc_residuals.__doc__ and nhp.DiscreteResiduals.__doc__ and nhp.DiscreteFitTest.__doc__
    p = dr.make(nhp, 3)
    data = np.zeros((3, 10), dtype=np.int64)
    cont = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.ones(2)), nhp.ExponentialImpulseResponse(np.ones((2, 2))),
                                               nhp.DenseWeightModel(np.full((2, 2), 0.1)))
    for fn in (nhp.disc_residuals, nhp.disc_goodness_of_fit):
        with pytest.raises(TypeError):
            fn(cont, data[:2])
    for nbins in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError):
            nhp.disc_residuals(p, data, nbins=nbins)


@pytest.fixture(scope="module")
def grid_errors():
    """max |restatement - exact| over the grid, per uniform; every pit inside [0, 1]."""
    import mpmath as mp
    cells = rr.grid()
    assert len(cells) == 109
    s, mu = np.array([c[0] for c in cells], float), np.array([c[1] for c in cells])
    worst, steps = {}, []
    for v in rr.GRID_V:
        p = rr.pit_cells(s, mu, np.full(len(cells), v), steps=steps)
        assert np.all((p >= 0.0) & (p <= 1.0))
        worst[v] = max(abs(float(mp.mpf(float(pi)) - rr.exact(si, mi, v))) for (si, mi), pi in zip(cells, p))
    return worst, max(int(x.max()) for x in steps)


def test_restatement_against_mpmath(grid_errors):
    worst, steps = grid_errors
    print(f"restatement against mpmath: max abs error per v {worst}, most loop steps of a cell {steps}")
    assert max(worst.values()) <= EXACT_TOL
    assert steps < 10000                              # 8 487 at μ = 2^20 eight sigma out: the 2^20 cap bounds the loops


def test_naive_log_gamma_pmf_misses_the_bound():
    import mpmath as mp
    mu = 2.0 ** 20
    naive = lambda s, m: (np.array([rr.naive_pmf(a, b) for a, b in zip(s, m)]), None)
    errs = []
    for z in (0, 1, -1):
        s = float(int(mu + z * 1024.0))
        p = rr.pit_cells(np.array([s]), np.array([mu]), np.array([0.37]), pmf_fn=naive)[0]
        errs.append(abs(float(mp.mpf(float(p)) - rr.exact(s, mu, 0.37))))
    print(f"naive pmf at mu = 2^20: abs errors {errs}")
    assert max(errs) > EXACT_TOL * 1000               # 2.4e-10 measured


def test_edge_cells_of_the_restatement():
    counts = np.array([[0, 1, 0]], dtype=np.int64)
    lam = np.array([[0.0], [0.0], [1e-300]])
    v = np.array([[0.25], [0.5], [0.75]])
    r = rr.residuals(counts, lam, 0, nbins=4, v=v)
    assert r["pit"][0].tolist() == [0.25, 1.0, 0.75] and r["impossible"] == 1
    assert r["pearson"][0, 0] == 0.0 and np.isposinf(r["pearson"][0, 1]) and np.isposinf(r["chi2"][0])
    assert r["deviance"][0] == 2e-300 and r["histogram"][0].tolist() == [0, 1, 0, 2] and r["observed"][0] == 1


@pytest.fixture(scope="module")
def stat_data(nhp):
    p = rr.stat_process(nhp)
    counts, _ = dr.simulate(p, rr.STAT_T, rr.STAT_DATA_SEED)
    return p, counts


def test_true_model_passes(nhp, stat_data):
    p, counts = stat_data
    r = rr.residuals(counts, dr.intensity(p, counts), rr.STAT_SEED)
    d, pv = rr.ks_uniform(r["pit"])
    disp = r["chi2"] / rr.STAT_T
    hp = rr.histogram_pvalue(r["histogram"])
    print(f"true model: KS D = {d:.5f}, p = {pv:.3f}; histogram p = {hp:.3f}; dispersion {disp}")
    assert pv > rr.KS_TRUE_MIN and hp > rr.KS_TRUE_MIN
    assert np.all(np.abs(disp - 1.0) <= rr.DISPERSION_TOL)
    assert r["impossible"] == 0 and np.array_equal(r["observed"], counts.sum(axis=1))


def test_wrong_model_fails(nhp, stat_data):
    p, counts = stat_data
    r = rr.residuals(counts, dr.intensity(rr.wrong(p), counts), rr.STAT_SEED)
    d, pv = rr.ks_uniform(r["pit"])
    hp = rr.histogram_pvalue(r["histogram"])
    print(f"weights x 1.5: KS D = {d:.5f}, p = {pv:.3g}; histogram p = {hp:.3g}")
    assert pv < rr.KS_WRONG_MAX and hp < rr.KS_WRONG_MAX
