"""disc_forecast(process, data, horizon) without a GPU: the export, the argument errors raised before any device work, the
literal three-part sampler against the exact mean recursion (and against the two wrong laws the GPU tests must be able to
tell apart: no carry-over, carry-over one bin late), and every statistical check of tests/test_disc_forecast_gpu.py run on
the numpy restatement of the documented Philox scheme with the same models and seeds -- an ensemble that reproduces the
restatement bit for bit therefore passes them.

Statistics held to |z| <= 5 in this file: 40 (literal sampler) + 40 (restatement, cell means) + 5 (iid cells) + 8 (single
link) + 100 (martingale sums) = 193: fewer than 10^3."""
import re

import numpy as np
import pytest

import disc_forecast_ref as fr
import disc_simulate_ref as dr


def test_the_symbol_and_the_python_entry_exist(nhp):
    from nhp_amd import _lib
    assert callable(nhp.disc_forecast)
    assert hasattr(_lib.lib(), "nhp_disc_forecast")
    assert "conditional" in nhp.disc_forecast.__doc__ and nhp.DiscreteForecast.__doc__


def test_argument_errors_come_before_any_device_work(nhp):
    cont = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.ones(2)), nhp.ExponentialImpulseResponse(np.ones((2, 2))),
                                               nhp.DenseWeightModel(0.1 * np.ones((2, 2))))
    data = fr.history(3, 12, 1)
    with pytest.raises(TypeError, match="discrete"):
        nhp.disc_forecast(cont, data[:2], 5)
    p = dr.make(nhp, 3)
    for h in (0, -5, 2.5, "3"):
        with pytest.raises(ValueError, match="horizon"):
            nhp.disc_forecast(p, data, h)
    for s in (0, -1, 1.5):
        with pytest.raises(ValueError, match="nsamples"):
            nhp.disc_forecast(p, data, 5, nsamples=s)
    for cap in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="max_events"):
            nhp.disc_forecast(p, data, 5, max_events=cap)
    with pytest.raises(ValueError, match="rows"):
        nhp.disc_forecast(p, fr.history(4, 12, 1), 5)
    with pytest.raises(ValueError, match="rows"):
        nhp.disc_forecast(p, data[0], 5)
    with pytest.raises(TypeError, match="integer"):
        nhp.disc_forecast(p, data.astype(float), 5)
    for col in (-2, 0):                               # in the tail, and before it: the whole host matrix is checked
        bad = data.copy()
        bad[1, col] = -1
        with pytest.raises(nhp.DomainError, match="non-negative"):
            nhp.disc_forecast(p, bad, 5)
    q = dr.make(nhp, 3, lgcp_T=20)
    with pytest.raises(ValueError, match=re.escape("Sample duration does not match process duration.")):
        nhp.disc_forecast(q, data, 9)                 # T0 + H = 21 > 20
    ds = nhp.DiscreteDataset.__new__(nhp.DiscreteDataset)           # no device behind it: the refusal comes first
    with pytest.raises(TypeError, match="matrix"):
        nhp.disc_forecast(p, ds, 5)
    with pytest.raises(TypeError):                                  # forecast() itself keeps refusing discrete processes
        nhp.forecast(p, data, 5)


def test_literal_sampler_follows_the_recursion_and_not_the_wrong_laws(nhp):
    m = fr.MEAN_CASE
    p, data = fr.mean_case(nhp)
    base, W, theta, A, phi, dt = fr.lower(p, m["T0"], m["H"])
    h = fr.link_lag_mass(W, theta, A, phi, dt)
    rho = np.max(np.abs(np.linalg.eigvals(h.sum(axis=2))))
    carry = fr.carry_exact(data, h, m["H"])
    mu = fr.mean_recursion(base, carry, h)
    assert 0.5 < rho < 0.9 and np.all(carry[h.shape[2]:] == 0.0) and carry[0].min() > 0
    print(f"spectral radius {rho:.2f}; share of carry-over in the first bin {carry[0] / mu[0]}")
    paths = fr.literal_sample(data, base, h, m["S"], np.random.default_rng(m["numpy_seed"]))
    z = fr.cell_z(paths, mu)
    late = np.vstack([np.zeros((1, carry.shape[1])), carry[:-1]])
    z_none = fr.cell_z(paths, fr.mean_recursion(base, np.zeros_like(carry), h))
    z_late = fr.cell_z(paths, fr.mean_recursion(base, late, h))
    print(f"max |z|: the law {np.abs(z).max():.1f}, no carry-over {np.abs(z_none).max():.1f}, carry-over one bin late "
          f"{np.abs(z_late).max():.1f}")
    assert z.size == 40 and np.all(np.abs(z) <= 5.0)
    assert np.abs(z_none).max() > 10.0 and np.abs(z_late).max() > 10.0


def test_boundary_state_of_the_restatement(nhp):
    """The documented operation order gives carry and the cell means of the definition to rounding; carry is exactly 0 beyond L."""
    for name, (kw, T0, rate, H, seed) in fr.RESTATE_CASES.items():
        p = dr.make(nhp, **kw)
        data = fr.history(kw["N"], T0, seed, rate)
        cm, carry, (W, theta, A, phi, dt) = fr.boundary(p, data, H)
        h = fr.link_lag_mass(W, theta, A, phi, dt)
        assert np.allclose(carry, fr.carry_exact(data, h, H), rtol=1e-12, atol=0.0), name
        assert np.all(carry[phi.shape[0]:] == 0.0) and carry[0].max() > 0


@pytest.mark.parametrize("name", list(fr.RESTATE_CASES))
def test_restatement_is_deterministic_and_keeps_children_inside_their_replica(nhp, name):
    kw, T0, rate, H, seed = fr.RESTATE_CASES[name]
    p = dr.make(nhp, **kw)
    data = fr.history(kw["N"], T0, seed, rate)
    info = {}
    paths, carry = fr.restate(p, data, H, fr.RESTATE_S, seed, info)
    assert paths.shape == (fr.RESTATE_S, kw["N"], H) and paths.sum() > 0 and len(info["per_generation"]) >= 1
    assert ("ptrs" in info["branches"]) == ("PTRS" in name) and (info["cell_means"].max() > 10.0) == ("PTRS" in name)
    again, _ = fr.restate(p, data, H, fr.RESTATE_S, seed)
    other, _ = fr.restate(p, data, H, fr.RESTATE_S, seed + 1)
    assert np.array_equal(paths, again) and not np.array_equal(paths, other)
    longer = np.hstack([fr.history(kw["N"], 7, 99), data])         # bins before the last L change nothing
    if T0 >= p.nlags() and "LGCP" not in name:                     # (an LGCP's means move with T0)
        assert np.array_equal(fr.restate(p, longer, H, fr.RESTATE_S, seed)[0], paths)


def test_the_chunk_case_spans_several_chunks(nhp):
    p, data, H, S, seed, cap = fr.chunk_case(nhp)
    info = {}
    paths, carry = fr.restate(p, data, H, S, seed, info)
    print(f"cells {info['cells']}, slots per generation {info['per_generation']}, events {paths.sum()}")
    assert info["cells"] > 4096 and info["per_generation"][0] > 4096 and paths.sum() < cap <= 4096
    assert len(info["per_generation"]) >= 2 and carry.max() > 0


def test_restatement_ensemble_mean_against_the_recursion(nhp):
    m = fr.MEAN_CASE
    p, data = fr.mean_case(nhp)
    base, W, theta, A, phi, dt = fr.lower(p, m["T0"], m["H"])
    h = fr.link_lag_mass(W, theta, A, phi, dt)
    mu = fr.mean_recursion(base, fr.carry_exact(data, h, m["H"]), h)
    paths, _ = fr.restate(p, data, m["H"], m["S"], m["seed"])
    z = fr.cell_z(paths, mu)
    print(f"ensemble mean per cell: max |z| = {np.abs(z).max():.2f} over {z.size} cells")
    assert z.size == 40 and np.all(np.abs(z) <= 5.0)


def test_known_laws_on_the_restatement(nhp):
    k = fr.IID
    paths, carry = fr.restate(fr.iid_process(nhp), fr.history(k["N"], 5, 2), k["H"], k["S"], k["seed"])
    assert not carry.any()
    z, chi2, zv = fr.iid_checks(paths, k["mean"])
    print(f"iid cells: z of the node totals {z}, of the variance {zv:.2f}")
    assert np.all(np.abs(z) <= 5.0) and chi2 and abs(zv) <= 5.0
    k = fr.LINK
    p, data = fr.link_process(nhp)
    paths, carry = fr.restate(p, data, k["H"], k["S"], k["seed"])
    zm, zv, on = fr.link_checks(paths, carry)
    print(f"single link: carry {carry[:, 2]}, z of the means {zm}, of the variances {zv}")
    assert on.sum() == k["L"] and not paths[:, :2].any() and not paths[:, 2][:, ~on].any()
    assert np.all(np.abs(zm) <= 5.0) and np.all(np.abs(zv) <= 5.0)


def test_martingale_checks_on_the_restatement(nhp):
    p, data = fr.mean_case(nhp)
    m, k = fr.MEAN_CASE, fr.MARTINGALE
    paths, _ = fr.restate(p, data, m["H"], k["S"], k["seed"])
    full, mask = fr.chain(data, paths)
    assert mask.sum() == k["S"] * m["H"] and data.shape[1] >= p.nlags()
    fr.assert_martingale(p.nlags(), full, mask, dr.intensity(p, full), dr.intensity(p, full, dr.shifted_basis(p)))
