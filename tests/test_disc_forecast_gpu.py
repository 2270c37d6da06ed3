"""disc_forecast(process, data, horizon) on the device: nhp_disc_forecast (csrc/disc_forecast.hip).

Contract of the outputs and determinism, the exact numpy restatement of the documented counter scheme
(tests/disc_forecast_ref.py, written from include/nhp.h), carry and the exact mean against numpy, the ensemble mean against
the mean recursion, two known laws, consistency with the library's own intensity across the boundary T0 (normalised
martingale sums over the forecast bins), the failure paths, the degenerate sizes, the round trip into loglikelihood and the
example.

Statistical bounds are |z| <= 5 with fixed seeds: 40 (cell means) + 5 (iid cells) + 8 (single link) + 100 (martingale sums) =
153 statistics, fewer than 10^3; the two-sided normal tail at 5 is 5.7e-7, and every seed is pre-checked on the restatement
by tests/test_disc_forecast_host.py."""
import copy
import importlib.util
import os

import numpy as np
import pytest

import disc_forecast_ref as fr
import disc_simulate_ref as dr

pytestmark = pytest.mark.gpu


def case(nhp, name):
    kw, T0, rate, H, seed = fr.RESTATE_CASES[name]
    return dr.make(nhp, **kw), fr.history(kw["N"], T0, seed, rate), H, seed


def same(a, b):
    return (np.array_equal(a.totals, b.totals) and np.array_equal(a.cell_sum, b.cell_sum) and np.array_equal(a.carry, b.carry)
            and np.array_equal(a.expected, b.expected) and a.events == b.events and a.generations == b.generations)


# ---- 1. contract and determinism ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,network", [(3, False), (5, True)])
def test_output_contract_and_determinism(nhp, N, network):
    import torch
    ctx = nhp.default_context()
    p = dr.make(nhp, N, seed=N, network=network)
    L, H, S = p.nlags(), 6, 50
    data = fr.history(N, 12, N)
    f = nhp.disc_forecast(p, data, H, nsamples=S, seed=7, return_paths=True)
    assert f.totals.shape == (S, N) and f.paths.shape == (S, N, H)
    assert f.mean.shape == f.expected.shape == f.carry.shape == f.cell_sum.shape == (N, H)
    assert f.totals.dtype == f.paths.dtype == f.cell_sum.dtype == np.int64
    assert f.mean.dtype == f.expected.dtype == f.carry.dtype == np.float64
    assert f.paths.min() >= 0 and f.events > 100 and f.generations >= 2
    assert np.array_equal(f.totals, f.paths.sum(axis=2)) and np.array_equal(f.cell_sum, f.paths.sum(axis=0))
    assert f.events == f.paths.sum() and np.array_equal(f.mean, f.cell_sum / S)
    # a repeated call, without the paths, another max_events: the same bits
    for other in (nhp.disc_forecast(p, data, H, nsamples=S, seed=7, return_paths=True),
                  nhp.disc_forecast(p, data, H, nsamples=S, seed=7),
                  nhp.disc_forecast(p, data, H, nsamples=S, seed=7, max_events=2 * f.events),
                  nhp.disc_forecast(p, data, H, nsamples=S, seed=7, max_events=20 * f.events),
                  nhp.disc_forecast(p, data[:, -L:], H, nsamples=S, seed=7)):
        assert same(f, other)
    assert nhp.disc_forecast(p, data, H, nsamples=S, seed=7).paths is None
    # device outputs, and a device-tensor history
    dev_data = torch.from_numpy(data).to(torch.device("cuda", ctx.device))
    for d in (nhp.disc_forecast(p, data, H, nsamples=S, seed=7, return_paths=True, device=True),
              nhp.disc_forecast(p, dev_data, H, nsamples=S, seed=7, return_paths=True, device=True)):
        for x, dtype, shape in ((d.totals, torch.int64, (S, N)), (d.paths, torch.int64, (S, N, H)), (d.cell_sum, torch.int64, (N, H)),
                                (d.mean, torch.float64, (N, H)), (d.expected, torch.float64, (N, H)), (d.carry, torch.float64, (N, H))):
            assert x.dtype == dtype and tuple(x.shape) == shape and x.device.type == "cuda" and x.device.index == ctx.device
        assert np.array_equal(d.paths.cpu().numpy(), f.paths) and np.array_equal(d.totals.cpu().numpy(), f.totals)
        assert np.array_equal(d.cell_sum.cpu().numpy(), f.cell_sum) and np.array_equal(d.carry.cpu().numpy(), f.carry)
        assert np.array_equal(d.expected.cpu().numpy(), f.expected) and np.array_equal(d.mean.cpu().numpy(), f.mean)
        assert d.events == f.events
    h = nhp.disc_forecast(p, dev_data, H, nsamples=S, seed=7, return_paths=True)
    assert same(f, h) and np.array_equal(h.paths, f.paths)
    assert not np.array_equal(nhp.disc_forecast(p, data, H, nsamples=S, seed=8).totals, f.totals)


# ---- 2. the exact restatement; 3. carry and the exact mean ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(fr.RESTATE_CASES))
def test_restatement_reproduces_the_ensemble_exactly(nhp, name):
    p, data, H, seed = case(nhp, name)
    f = nhp.disc_forecast(p, data, H, nsamples=fr.RESTATE_S, seed=seed, return_paths=True)
    want, carry = fr.restate(p, data, H, fr.RESTATE_S, seed)
    assert want.sum() > 0
    assert np.array_equal(f.carry, carry.T)
    assert np.array_equal(f.paths, want)


def test_several_chunks_of_cells_and_of_child_slots(nhp):
    p, data, H, S, seed, cap = fr.chunk_case(nhp)
    info = {}
    want, _ = fr.restate(p, data, H, S, seed, info)
    assert info["cells"] > 4096 and info["per_generation"][0] > 4096 and want.sum() < cap <= 4096 and len(info["per_generation"]) >= 2
    f = nhp.disc_forecast(p, data, H, nsamples=S, seed=seed, return_paths=True, max_events=cap)
    assert np.array_equal(f.paths, want) and f.events == want.sum()
    g = nhp.disc_forecast(p, data, H, nsamples=S, seed=seed, return_paths=True)
    assert np.array_equal(g.paths, want)


@pytest.mark.parametrize("name", list(fr.RESTATE_CASES))
def test_carry_and_expected_against_numpy(nhp, name):
    """All terms are non-negative, so either summation order is within (terms·depth)·2^-53 of the sum: H·(N·B + L + 2)·2^-52 <
    1e-13 at these shapes; the bound is 1e-12 relative."""
    p, data, H, seed = case(nhp, name)
    f = nhp.disc_forecast(p, data, H, nsamples=2, seed=seed)
    base, W, theta, A, phi, dt = fr.lower(p, data.shape[1], H)
    h = fr.link_lag_mass(W, theta, A, phi, dt)
    carry = fr.carry_exact(data, h, H)
    mu = fr.mean_recursion(base, carry, h)
    print(f"{name}: max relative error of carry {np.abs(f.carry.T - carry)[carry > 0].max() / carry[carry > 0].min():.2e}, of "
          f"expected {np.abs(f.expected.T / mu - 1).max():.2e}")
    assert np.allclose(f.carry.T, carry, rtol=1e-12, atol=0.0)
    assert np.allclose(f.expected.T, mu, rtol=1e-12, atol=0.0)
    assert np.all(f.carry[:, phi.shape[0]:] == 0.0) and f.carry[:, 0].max() > 0
    quiet = nhp.disc_forecast(p, np.zeros_like(data), H, nsamples=2, seed=seed)
    assert np.all(quiet.carry == 0.0)
    assert np.allclose(quiet.expected.T, fr.mean_recursion(base, np.zeros_like(carry), h), rtol=1e-12, atol=0.0)


# ---- 4. the ensemble mean ---------------------------------------------------------------------------------------------------------

def test_ensemble_mean_against_the_exact_recursion(nhp):
    m = fr.MEAN_CASE
    p, data = fr.mean_case(nhp)
    f = nhp.disc_forecast(p, data, m["H"], nsamples=m["S"], seed=m["seed"], return_paths=True)
    base, W, theta, A, phi, dt = fr.lower(p, m["T0"], m["H"])
    h = fr.link_lag_mass(W, theta, A, phi, dt)
    mu = fr.mean_recursion(base, fr.carry_exact(data, h, m["H"]), h)
    z = fr.cell_z(f.paths, mu)
    z_lib = fr.cell_z(f.paths, f.expected.T)
    print(f"ensemble mean per cell: max |z| = {np.abs(z).max():.2f} over {z.size} cells (against the library's expected: "
          f"{np.abs(z_lib).max():.2f})")
    assert z.size == 40 and np.all(np.abs(z) <= 5.0)
    assert np.allclose(f.mean, f.paths.mean(axis=0))


# ---- 5. known laws ----------------------------------------------------------------------------------------------------------------

def test_without_weights_the_cells_are_iid_poisson(nhp):
    k = fr.IID
    f = nhp.disc_forecast(fr.iid_process(nhp), fr.history(k["N"], 5, 2), k["H"], nsamples=k["S"], seed=k["seed"], return_paths=True)
    assert not f.carry.any() and f.generations == 1 and np.all(f.expected == k["mean"])
    z, chi2, zv = fr.iid_checks(f.paths, k["mean"])
    print(f"iid cells: z of the node totals {z}, of the variance {zv:.2f}")
    assert np.all(np.abs(z) <= 5.0) and chi2 and abs(zv) <= 5.0


def test_a_single_link_without_baseline_gives_poisson_carry(nhp):
    k = fr.LINK
    p, data = fr.link_process(nhp)
    f = nhp.disc_forecast(p, data, k["H"], nsamples=k["S"], seed=k["seed"], return_paths=True)
    zm, zv, on = fr.link_checks(f.paths, f.carry.T)
    print(f"single link: carry {f.carry[2]}, z of the means {zm}, of the variances {zv}")
    assert on.sum() == k["L"] and not f.paths[:, :2].any() and not f.paths[:, 2][:, ~on].any()
    assert np.all(np.abs(zm) <= 5.0) and np.all(np.abs(zv) <= 5.0)
    assert np.array_equal(f.expected, f.carry)


# ---- 6. consistency with the library's own intensity --------------------------------------------------------------------------------

def test_martingale_sums_against_disc_intensity_across_the_boundary(nhp):
    p, data = fr.mean_case(nhp)
    m, k = fr.MEAN_CASE, fr.MARTINGALE
    f = nhp.disc_forecast(p, data, m["H"], nsamples=k["S"], seed=k["seed"], return_paths=True)
    full, mask = fr.chain(data, f.paths)
    lam = nhp.intensity(p, full)
    late = copy.deepcopy(p)
    shifted = dr.shifted_basis(p)
    late.impulses.basis = lambda: shifted
    fr.assert_martingale(p.nlags(), full, mask, lam, nhp.intensity(late, full))


# ---- 7. failure paths ---------------------------------------------------------------------------------------------------------------

def test_explosion_is_an_error_and_the_context_survives(nhp):
    wild = dr.make(nhp, 3, seed=2, scale=3.0)
    data = fr.history(3, 12, 1)
    with pytest.raises(RuntimeError, match="exploded"):
        nhp.disc_forecast(wild, data, 40, nsamples=50, seed=1, max_events=20000)
    with pytest.raises(RuntimeError, match="exploded"):                      # the cells alone pass the cap
        nhp.disc_forecast(wild, data, 40, nsamples=50, seed=1, max_events=10)
    p, data, H, seed = case(nhp, "standard, H = 6 > L = 4")
    f = nhp.disc_forecast(p, data, H, nsamples=fr.RESTATE_S, seed=seed, return_paths=True)
    assert np.array_equal(f.paths, fr.restate(p, data, H, fr.RESTATE_S, seed)[0])


def test_parameters_and_counts_no_process_has(nhp):
    import torch
    data = fr.history(3, 12, 1)
    p = dr.make(nhp, 3, seed=2)
    p.weights.W = p.weights.W.copy()
    p.weights.W[1, 2] = -0.1
    with pytest.raises(nhp.DomainError):
        nhp.disc_forecast(p, data, 5, nsamples=4)
    p = dr.make(nhp, 3, seed=2)
    p.impulses.θ[0, 1, 0] = np.nan
    with pytest.raises(nhp.DomainError):
        nhp.disc_forecast(p, data, 5, nsamples=4)
    p = dr.make(nhp, 3, seed=2)
    p.baseline.λ[2] = np.inf
    with pytest.raises(nhp.DomainError):
        nhp.disc_forecast(p, data, 5, nsamples=4)
    p = dr.make(nhp, 3, seed=2)
    bad = torch.from_numpy(data).to(torch.device("cuda", nhp.default_context().device))
    bad[1, -2] = -1
    with pytest.raises(nhp.DomainError, match="non-negative"):
        nhp.disc_forecast(p, bad, 5, nsamples=4)
    huge = data.copy()
    huge[0, -1] = 10 ** 9                             # a cell mean above 2^20
    with pytest.raises(nhp.DomainError):
        nhp.disc_forecast(p, huge, 5, nsamples=4)
    assert nhp.disc_forecast(p, data, 5, nsamples=4).totals.shape == (4, 3)


# ---- 8. degenerate sizes ------------------------------------------------------------------------------------------------------------

def test_degenerate_sizes(nhp):
    one = dr.make(nhp, 1, seed=2, rate=2.0, scale=0.4)
    data = np.array([[3, 1, 4]], dtype=np.int64)
    f = nhp.disc_forecast(one, data, 1, nsamples=1, seed=1, return_paths=True)
    want, carry = fr.restate(one, data, 1, 1, 1)
    assert f.paths.shape == (1, 1, 1) and np.array_equal(f.paths, want) and f.totals[0, 0] == want.sum() and f.carry[0, 0] == carry[0, 0] > 0
    assert f.expected[0, 0] == dr.lower(one, 1)[0][0, 0] + f.carry[0, 0]            # expected = base + carry in the first bin
    quiet = dr.make(nhp, 3, seed=2, rate=0.0)
    f = nhp.disc_forecast(quiet, np.zeros((3, 7), dtype=np.int64), 5, nsamples=6, seed=1, return_paths=True)
    assert f.events == 0 and f.generations == 0 and not f.paths.any() and not f.totals.any() and not f.cell_sum.any()
    assert not f.carry.any() and not f.expected.any()
    f = nhp.disc_forecast(quiet, np.zeros((3, 7), dtype=np.int64), 5, nsamples=6, seed=1, max_events=0)
    assert f.events == 0 and not f.totals.any()


# ---- 9. round trip; 10. the example ---------------------------------------------------------------------------------------------------

def test_a_path_appended_to_the_data_is_data(nhp):
    p, data, H, seed = case(nhp, "network, H = 3 < L = 4")
    f = nhp.disc_forecast(p, data, H, nsamples=4, seed=seed, return_paths=True)
    full = np.hstack([data, f.paths[1]])
    assert full.shape == (data.shape[0], data.shape[1] + H)
    assert np.isfinite(nhp.loglikelihood(p, full))
    lam = nhp.intensity(p, full)                      # the first forecast bin's conditional mean is base + carry
    assert np.allclose(lam[data.shape[1]], fr.boundary(p, data, H)[0][0], rtol=1e-12)


def test_the_example_runs(nhp):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples",
                        "discrete_gaussian_standard_hawkes_forecast.py")
    import sys
    sys.path.insert(0, os.path.dirname(path))
    try:
        spec = importlib.util.spec_from_file_location("example_disc_forecast", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        truth, f, cold = mod.main(duration=300, horizon=5, nsamples=200, seed=0)
    finally:
        sys.path.remove(os.path.dirname(path))
    assert truth.shape == (3, 5) and f.mean.shape == f.expected.shape == (3, 5) and f.paths.shape == (200, 3, 5)
    assert np.all(np.isfinite(f.mean)) and np.all(np.isfinite(f.expected)) and np.all(f.expected > 0)
    assert not cold.carry.any() and np.all(cold.expected <= f.expected)          # carry >= 0: forgetting the history never adds
