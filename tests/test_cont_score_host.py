"""Host-side checks of the continuous chain scorer (no GPU): the numpy restatement against the long-double / 50-digit
reference -- the yardstick the GPU tests hold the device to --, the cells' sum against the exact log-likelihood from
tests/compensator_ref.py, four planted mistakes, compare_scores on two continuous scores, and the argument checks of mcmc_
and score_samples (which must refuse before any library call)."""
import math

import numpy as np
import pytest

import compensator_ref as cref
import cont_score_ref as ref


@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_numpy_restatement_against_reference(kind, network):
    """The streaming fp64 algorithm is the definition to rounding: every quantity within the continuous routes' parity floor,
    1e-11·max(1, Σ|ℓ|), every cell within 1e-11·max(1, Σ|log λ| + ΔΛ) of its own."""
    case = ref.small_case(kind, network)
    r = ref.score_mp(case)
    got = ref.score_numpy(case)
    err = ref.errors(got, r)
    tol = ref.tolerances({k: 0.0 for k in err}, r)
    print(f"{kind} network={network} yardstick: " + ", ".join(f"{k}={v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        if k == "pointwise":
            assert np.all(ref.pointwise_errors(got, r) <= tol[k])
        else:
            assert v <= tol[k], (k, v, tol[k])
    assert got["summary"]["n"] == 7 and got["summary"]["cells"] == 8 * 3


@pytest.mark.parametrize("kind,dt_max", [("exponential", 0.5), ("exponential", math.inf), ("logitnormal", 0.5)])
def test_cells_add_up_to_the_exact_loglikelihood(kind, dt_max):
    """Over edges covering [0, T], Σ_k ℓ_{k,c} = Σ log λ_c − Λ_c(T) with Λ_c(T) from tests/compensator_ref.py (written from the
    compensator's definition, one fsum over every event): the exact log-likelihood, block by block."""
    case = ref.make_case(3, 40, [0.0, 0.7, 0.9, 3.0, 6.0, 8.0], 2, kind, True, seed=11, T=8.0, dt_max=dt_max)
    for draw in case["draws"]:
        kw = dict(theta=draw["theta"]) if kind == "exponential" else dict(mu=draw["mu"], tau=draw["tau"])
        model = cref.Model(draw["lam0"], draw["W"], dt_max, A=draw["A"], **kw)
        total = np.array([model.Lambda(c, case["T"], case["times"], case["nodes"] - 1) for c in range(3)])
        sumlog, abslog, dlam = ref.cell_parts(case, draw, np.float64)
        got = (sumlog - dlam).sum(axis=0)
        want = sumlog.sum(axis=0) - total
        bound = 1e-11 * np.maximum(1.0, abslog.sum(axis=0) + total)
        assert np.all(np.abs(got - want) <= bound), (got, want)
        assert np.all(np.abs(dlam.sum(axis=0) - total) <= bound)


def mutant_case():
    """Events on edges, events whose window straddles the next edge, events before the block that still reach into it."""
    T, dt = 8.0, 1.0
    edges = [1.0, 2.0, 2.5, 4.0, 7.0]
    extra = [(2.0, 1), (2.5, 2), (4.0, 3), (1.75, 1), (2.25, 2), (3.5, 3)]
    case = ref.make_case(3, 60, edges, 1, "exponential", False, 21, T=T, dt_max=dt, extra_times=extra)
    return case


@pytest.mark.parametrize("mutate", ref.MUTANTS)
def test_planted_mistakes_exceed_the_bound(mutate):
    """Each of the four mistakes moves some cell by orders of magnitude more than the cell's bound 1e-11·max(1, Σ|log λ| + ΔΛ)."""
    case = mutant_case()
    draw = case["draws"][0]
    if mutate == "one_minus_exp":            # tiny θ, large W: terms of 1e-3 made of 1 − e^{−x} at x ≈ 1e-13, where 1 − exp keeps three digits
        draw = dict(draw, theta=np.full((3, 3), 2.0 ** -42), W=np.full((3, 3), 2.0 ** 32))
    good, scale = ref.cells(case, draw, np.longdouble)
    clean = ref.cells(case, draw, np.float64)[0]
    bad = ref.cells(case, draw, np.float64, mutate)[0]
    bound = 1e-11 * np.maximum(1.0, np.asarray(scale, dtype=np.float64))
    err_clean = np.abs(np.asarray(clean - good, dtype=np.float64))
    err_bad = np.abs(np.asarray(bad - good, dtype=np.float64))
    print(f"{mutate}: clean {np.max(err_clean / bound):.2e} of the bound, planted {np.max(err_bad / bound):.2e}")
    assert np.all(err_clean <= bound)
    assert np.max(err_bad / bound) >= 100.0


def test_compare_scores_on_continuous_scores(nhp):
    rng = np.random.default_rng(0)
    pa, pb = rng.normal(size=(4, 3)), rng.normal(size=(4, 3))
    edges = [0.0, 1.0, 2.0, 3.0, 4.0]

    def make(pw, e):
        return nhp.ContinuousScore([3, pw.size, 0.0, 0.0, pw.sum(), -2 * pw.sum(), 0.0, 0.0, 0.0, 0.0], np.zeros((3, pw.shape[1])), pw, e)
    a, b = make(pa, edges), make(pb, edges)
    assert a.bins == tuple(edges) and a.n == 3 and a.cells == 12
    cmp = nhp.compare_scores(a, b)
    d = (pa - pb).ravel()
    assert cmp.elpd_diff == pytest.approx(d.sum()) and cmp.se_diff == pytest.approx(math.sqrt(12 * np.var(d, ddof=1)))
    with pytest.raises(ValueError, match="different bins"):
        nhp.compare_scores(a, make(pb, [0.0, 1.0, 2.0, 3.0, 4.5]))


def a_process(nhp, N=2, lgcp=False):
    base = nhp.LogGaussianCoxProcess([0.0, 1.0, 2.0], [np.ones(3)] * N) if lgcp else nhp.HomogeneousProcess(np.ones(N))
    return nhp.ContinuousStandardHawkesProcess(base, nhp.ExponentialImpulseResponse(np.ones((N, N))), nhp.DenseWeightModel(np.full((N, N), 0.1)))


DATA = (np.array([0.5, 1.0]), np.array([1, 2]), 2.0)


@pytest.mark.parametrize("kwargs,exc,match", [
    (dict(waic=2, score_every=0), ValueError, "score_every"),
    (dict(waic=2, score_every=1.5), ValueError, "score_every"),
    (dict(waic=2, burn=-1), ValueError, "burn"),
    (dict(waic=0), ValueError, "number of blocks"),
    (dict(waic=True), ValueError, "number of blocks"),
    (dict(waic=[0.0]), ValueError, "at least two"),
    (dict(waic=[0.0, 1.0, 1.0]), ValueError, "increase strictly"),
    (dict(waic=[0.0, math.nan]), ValueError, "finite"),
    (dict(waic=[-0.5, 1.0]), ValueError, "inside"),
    (dict(waic=[0.0, 2.5]), ValueError, "inside"),
    (dict(heldout=DATA), ValueError, "heldout must be"),
    (dict(heldout=(DATA, [1.0, 0.5])), ValueError, "increase strictly"),
    (dict(heldout=((np.array([0.5]), np.array([3]), 2.0), 2)), ValueError, "nodes"),
    (dict(heldout=([DATA, DATA], 2)), NotImplementedError, "several trials"),
])
def test_mcmc_argument_checks_precede_the_library(nhp, monkeypatch, kwargs, exc, match):
    from nhp_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched before the arguments were checked"))
    monkeypatch.setattr(_lib, "default_context", lambda: pytest.fail("a context was made before the arguments were checked"))
    with pytest.raises(exc, match=match):
        nhp.mcmc_(a_process(nhp), DATA, nsteps=2, **kwargs)


def test_mcmc_refuses_what_scoring_is_not_built_for(nhp, monkeypatch):
    from nhp_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched before the arguments were checked"))
    monkeypatch.setattr(_lib, "default_context", lambda: pytest.fail("a context was made before the arguments were checked"))
    with pytest.raises(NotImplementedError, match="homogeneous baseline"):
        nhp.mcmc_(a_process(nhp, lgcp=True), DATA, nsteps=2, waic=2)
    with pytest.raises(NotImplementedError, match="several trials"):
        nhp.mcmc_(a_process(nhp), [DATA, DATA], nsteps=2, waic=2)
    shard = object.__new__(nhp.ShardedDataset)
    with pytest.raises(NotImplementedError, match="ShardedDataset"):
        nhp.mcmc_(a_process(nhp), shard, nsteps=2, waic=2)


def test_score_samples_argument_checks(nhp, monkeypatch):
    from nhp_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched before the arguments were checked"))
    monkeypatch.setattr(_lib, "default_context", lambda: pytest.fail("a context was made before the arguments were checked"))
    proc = a_process(nhp)
    x = proc.params()
    for kw, match in [(dict(every=0), "every"), (dict(burn=-1), "burn"), (dict(burn=1), "no draws left")]:
        with pytest.raises(ValueError, match=match):
            nhp.score_samples(proc, [x], DATA, 2, **kw)
    with pytest.raises(ValueError, match="inside"):
        nhp.score_samples(proc, [x], DATA, [0.0, 3.0])
    with pytest.raises(NotImplementedError, match="homogeneous baseline"):
        nhp.score_samples(a_process(nhp, lgcp=True), [x], DATA, 2)
