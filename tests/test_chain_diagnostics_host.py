"""The numpy restatement of the streaming convergence diagnostics (tests/chain_diagnostics_ref.py, from include/nhp.h)
against known answers, chains.potential_scale_reduction against a direct computation, and the argument checks of mcmc_ that
come before any device work.  No GPU."""
import numpy as np
import pytest
from scipy.signal import lfilter

import chain_diagnostics_ref as ref

SEEDS = range(20)          # one column per seed: the planes are per entry, so 20 chains cost one pass


def normal_columns(n):
    return np.stack([np.random.default_rng(s).normal(size=n) for s in SEEDS], axis=1)


def test_iid_normal_has_ess_near_n_and_rhat_near_one():
    n = 10_000
    d = ref.diagnose(normal_columns(n), 100)
    assert d["a"] == 100 and not d["undefined"].any()
    ratio = d["ess"] / n
    print("iid ESS/n", ratio.min(), ratio.max(), "R-hat max", d["rhat"].max())
    assert np.all((ratio >= 0.6) & (ratio <= 1.5))
    assert np.all(d["rhat"] < 1.01)
    # MCSE is the batch-means standard error of the mean: ≈ 1/√n here
    assert np.all(np.abs(d["mcse"] * np.sqrt(n) - 1.0) < 0.3)


def test_ar1_ess_matches_theory():
    """AR(1) with φ = 0.9: ESS/n -> (1 − φ)/(1 + φ) = 0.0526."""
    n, phi = 40_000, 0.9
    x = lfilter([1.0], [1.0, -phi], normal_columns(n), axis=0)
    d = ref.diagnose(x, 200)
    ratio = d["ess"] / n
    print("AR(1) ESS/n", ratio.min(), ratio.max())
    assert np.all((ratio >= 0.035) & (ratio <= 0.08))


def test_shifted_second_half_gives_rhat_sqrt3():
    """Halves N(0, 1) and N(2, 1): W = 1, (m1 − m2)²/(2W) = 2, R-hat -> √3."""
    n = 10_000
    x = normal_columns(n)
    x[n // 2:] += 2.0
    d = ref.diagnose(x, 100)
    print("shifted R-hat", d["rhat"].min(), d["rhat"].max())
    assert np.all((d["rhat"] >= 1.6) & (d["rhat"] <= 1.85))


def test_nan_rules_and_undefined_entries():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(23, 4))
    x[:, 2] = 0.625                                           # a constant column
    d = ref.diagnose(x, 4)                                    # a = 5, partial last batch, n odd: two snapshots
    assert d["a"] == 5 and list(d["undefined"]) == [False, False, True, False]
    assert np.isnan(d["ess"][2]) and np.isnan(d["rhat"][2]) and d["mcse"][2] == 0.0
    assert np.all(np.isfinite(np.delete(d["ess"], 2))) and np.all(np.isfinite(np.delete(d["rhat"], 2)))
    # the middle step of an odd n is dropped: the halves are steps 0..10 and 12..22
    h = 11
    m1, m2 = x[:h].mean(axis=0), x[12:].mean(axis=0)
    W = (x[:h].var(axis=0, ddof=1) + x[12:].var(axis=0, ddof=1)) / 2
    with np.errstate(invalid="ignore"):                       # (the constant column: 0/0)
        want = np.sqrt((h - 1) / h + (m1 - m2) ** 2 / (2 * W))
        # batch means by hand: five batches of four, the last three steps never folded in
        bm = x[:20].reshape(5, 4, 4).mean(axis=1)
        sbm = 4 * bm.var(axis=0, ddof=1)
        ess = 23 * x.var(axis=0, ddof=1) / sbm
    assert np.allclose(np.delete(d["rhat"], 2), np.delete(want, 2), rtol=1e-10)
    assert np.allclose(np.delete(d["mcse"], 2), np.delete(np.sqrt(sbm / 23), 2), rtol=1e-10)
    assert np.allclose(np.delete(d["ess"], 2), np.delete(ess, 2), rtol=1e-10)
    # a < 2: ESS and MCSE are NaN, R-hat is not
    d7 = ref.diagnose(x[:7], 4)
    assert d7["a"] == 1 and np.all(np.isnan(d7["ess"])) and np.all(np.isnan(d7["mcse"]))
    assert np.all(np.isfinite(np.delete(d7["rhat"], 2)))
    # n != n_planned: R-hat is NaN, ESS is not
    dp = ref.diagnose(x[:20], 4, n_planned=23)
    assert np.all(np.isnan(dp["rhat"])) and np.all(np.isfinite(np.delete(dp["ess"], 2)))
    # h < 2: no split
    assert np.all(np.isnan(ref.diagnose(x[:3], 1)["rhat"]))
    s = ref.summarize(d, 1e9, 0.0)
    assert s["entries"] == 4 and s["undefined"] == 1 and s["ess_below"] == 3 and s["rhat_above"] == 3
    assert s["min_ess_index"] == int(np.nanargmin(d["ess"])) and s["max_mcse"] == np.nanmax(np.delete(d["mcse"], 2))
    empty = ref.summarize(d, 100.0, 1.01, slice(2, 3))
    assert empty["undefined"] == 1 and empty["min_ess_index"] == -1 and np.isnan(empty["min_ess"]) and np.isnan(empty["max_mcse"])


def test_summary_ties_go_to_the_lower_index():
    x = np.random.default_rng(5).normal(size=(40, 1)).repeat(3, axis=1)
    s = ref.summarize(ref.diagnose(x, 5), 100.0, 1.01)
    assert s["min_ess_index"] == 0 and s["max_rhat_index"] == 0


def test_potential_scale_reduction_against_stacked_samples(nhp):
    from nhp_amd import chains
    rng = np.random.default_rng(11)
    n, m, P = 200, 4, 7
    x = rng.normal(size=(m, n, P)) + rng.normal(scale=0.3, size=(m, 1, P))
    x[..., 5] = 1.0                                           # never moved in any chain: NaN
    summaries = {k: chains.summarize_chain(list(x[k])) for k in range(m)}
    got = chains.potential_scale_reduction(summaries)
    W = x.var(axis=1, ddof=1).mean(axis=0)
    Bn = x.mean(axis=1).var(axis=0, ddof=1)
    with np.errstate(invalid="ignore"):
        want = np.sqrt((n - 1) / n + Bn / W)
    keep = np.arange(P) != 5
    assert np.isnan(got[5]) and np.allclose(got[keep], want[keep], rtol=1e-9)
    assert np.all(got[keep] > 1.0)
    assert np.array_equal(chains.potential_scale_reduction(list(summaries.values())), got, equal_nan=True)
    with pytest.raises(ValueError):
        chains.potential_scale_reduction({0: summaries[0]})
    with pytest.raises(ValueError):
        chains.potential_scale_reduction([summaries[0], chains.summarize_chain(list(x[1][:50]))])


def test_diagnostics_arguments_are_checked_before_any_device_work(nhp, monkeypatch):
    from nhp_amd import _lib
    from helpers import random_case

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "default_context", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    c = random_case(3, 50, 10.0, "exponential", 1.0, nhp=nhp)
    with pytest.raises(ValueError, match="moments"):
        nhp.mcmc_(c["proc"], c["data"], nsteps=4, diagnostics=True, moments=False)
    with pytest.raises(ValueError):
        nhp.mcmc_(c["proc"], c["data"], nsteps=4, diagnostics="all", moments=True)
    with pytest.raises(ValueError):
        nhp.mcmc_(c["proc"], c["data"], nsteps=4, diagnostics=True, moments=True, batch_len=0)
