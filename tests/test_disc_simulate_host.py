"""disc_rand(process, steps) without a GPU: the export, the argument errors raised before any device work, the numpy
restatement of nhp_disc_simulate (tests/disc_simulate_ref.py) as a sample of the stated law, and the statistical checks of
tests/test_disc_simulate_gpu.py run on the restatement's samples with the same models and seeds -- a sampler that
reproduces the restatement bit for bit therefore passes them."""
import re

import numpy as np
import pytest

import disc_simulate_ref as dr


def test_the_symbol_and_the_python_entry_exist(nhp):
    from nhp_amd import _lib
    assert hasattr(_lib.lib(), "nhp_disc_simulate")
    assert callable(nhp.disc_rand)
    assert "disc_rand" in nhp.rand.__doc__ and "rand(process, steps)" in nhp.disc_rand.__doc__


def test_argument_errors_come_before_any_device_work(nhp):
    cont = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.ones(2)), nhp.ExponentialImpulseResponse(np.ones((2, 2))),
                                               nhp.DenseWeightModel(0.1 * np.ones((2, 2))))
    with pytest.raises(TypeError, match="discrete"):
        nhp.disc_rand(cont, 100)
    p = dr.make(nhp, 3)
    for steps in (0, -5, 2.5):
        with pytest.raises(ValueError, match="steps"):
            nhp.disc_rand(p, steps)
    for cap in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="max_events"):
            nhp.disc_rand(p, 100, max_events=cap)
    q = dr.make(nhp, 3, lgcp_T=200)
    with pytest.raises(ValueError, match=re.escape("Sample duration does not match process duration.")):
        nhp.disc_rand(q, 201)
    with pytest.raises(NotImplementedError, match="continuous"):      # the device switch of rand() stays what it was
        nhp.rand(p, 100, seed=0, device=True)


def test_restatement_without_weights_returns_its_immigrants(nhp):
    p = dr.make(nhp, 4, scale=0.0)
    info = {}
    s, bg = dr.simulate(p, dr.T_SMALL, 2, info)
    assert s.shape == bg.shape == (4, dr.T_SMALL) and s.dtype == np.int64
    assert np.array_equal(s, bg) and s.sum() > 200 and info["slots"] == 0


@pytest.mark.parametrize("name", list(dr.RESTATE_CASES))
def test_restatement_counts_are_immigrants_plus_kept_children(nhp, name):
    kw, T, seed = dr.RESTATE_CASES[name]
    p = dr.make(nhp, **kw)
    info = {}
    s, bg = dr.simulate(p, T, seed, info)
    assert np.all(s - bg >= 0) and bg.sum() > 0
    assert s.sum() - bg.sum() == info["kept"] > 0 and info["slots"] >= info["kept"]
    assert ("ptrs" in info["branches"]) == ("PTRS" in name) and "inversion" in info["branches"]
    if "zero column" in name:
        assert np.array_equal(s[1], bg[1])            # nothing reaches a node whose column of A is empty
    again, _ = dr.simulate(p, T, seed)
    other, _ = dr.simulate(p, T, seed + 1)
    assert np.array_equal(s, again) and not np.array_equal(s, other)


def test_restatement_mean_children_per_link(nhp):
    """Children of node p on node c per event of p, over a long run, against G[p, c] (the run is cut short of the last L bins'
    losses: they are below 1e-3 of the total here)."""
    p = dr.make(nhp, 3, seed=9, scale=0.6, rate=0.5)
    T = 20000
    s, bg = dr.simulate(p, T, 1)
    G = dr.link_mass(p)
    want = (s.sum(axis=1)[:, None] * G).sum(axis=0)                     # expected children per child node given the parents
    got = (s - bg).sum(axis=1)
    z = (got - want) / np.sqrt(want)
    print("children per node", got, "expected", want, "z", z)
    assert np.all(np.abs(z) <= 5.0)


@pytest.mark.parametrize("mean", dr.IMMIGRANT_MEANS)
def test_immigrant_checks_on_the_restatement(nhp, mean):
    s, bg = dr.simulate(dr.immigrant_process(nhp, mean), dr.IMMIGRANT_T, dr.IMMIGRANT_SEED)
    assert np.array_equal(s, bg)
    z, chi2 = dr.immigrant_checks(s, mean)
    print(f"mean {mean}: z of the node totals {z}")
    assert np.all(np.abs(z) <= 5.0) and chi2


@pytest.mark.parametrize("name", list(dr.MARTINGALE_CASES))
def test_martingale_checks_on_the_restatement(nhp, name):
    p = dr.make(nhp, **dr.MARTINGALE_CASES[name])
    s, _ = dr.simulate(p, dr.MARTINGALE_T, dr.MARTINGALE_SEED)
    assert s.sum(axis=1).min() > 1000
    dr.assert_martingale(p, s, dr.intensity(p, s), dr.intensity(p, s, dr.shifted_basis(p)))


def test_restatement_agrees_with_the_host_simulator(nhp):
    kw, T, S = dr.AGREEMENT
    p = dr.make(nhp, **kw)
    dr.assert_agreement([dr.simulate(p, T, seed)[0] for seed in range(S)], [nhp.rand(p, T, seed=1000 + seed) for seed in range(S)])
