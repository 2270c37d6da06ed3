"""Host-side checks of the chain scorer (no GPU): the numpy restatement against the 50-digit one -- the yardstick the GPU tests
hold the device to --, compare_scores, the argument checks of disc_mcmc_ and disc_score_samples (which must refuse before any
library call), and the new symbols in the built library."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import disc_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 5, 1, 2, None), (3, 37, 2, 4, None), (17, 129, 5, 9, (5, 128)), (6, 1000, 8, 5, (999, 1000))]


@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("N,T,B,L,bins", SHAPES)
def test_numpy_restatement_against_mpmath(N, T, B, L, bins, network):
    """The streaming fp64 algorithm (logaddexp, Welford, loggamma restored at the end) is the definition to rounding: on every
    quantity within 1e-12 of Σ|ℓ| (per cell: of that cell's own |ℓ_i|), the project's parity bound, for S = 1, 2 and 7 draws;
    where S = 1 leaves a quantity undefined both say NaN."""
    case = ref.make_case(N, T, B, L, bins, 7, network, seed=N + T, rate=0.5)
    mpr = ref.score_mp(case, (1, 2, 7))
    for S in (1, 2, 7):
        got = ref.score_numpy(dict(case, draws=case["draws"][:S]))
        err = ref.errors(got, mpr[S])
        floor_sum = 1e-12 * mpr[S]["sum_abs_ell"]
        print(f"N={N} T={T} network={network} S={S} yardstick: " + ", ".join(f"{k}={v:.2e}" for k, v in err.items()))
        for k, v in err.items():
            if S == 1 and k in ("p_waic", "elpd_waic", "waic", "se_elpd", "joint_sd", "pointwise"):
                assert math.isnan(v), (k, v)
            elif k == "se_elpd" and got["summary"]["cells"] == 1:
                assert math.isnan(v)
            elif k == "pointwise":                              # each cell against 1e-12 of its own |ℓ_i|
                cell_floor = ref.tolerances({"pointwise": 0.0}, mpr[S])["pointwise"]
                assert np.all(ref.pointwise_errors(got, mpr[S]) <= cell_floor), (k, v)
            elif k == "per_node" and S == 1:
                assert v <= floor_sum                           # lppd's row alone is defined
            else:
                assert v <= floor_sum, (k, v, floor_sum)
        assert got["summary"]["n"] == S and got["summary"]["cells"] == mpr[S]["summary"]["cells"]


def test_reference_invariants_hold_in_exact_arithmetic():
    """Jensen: lppd_i >= mean_s ℓ_i and the joint score above the mean of the totals; p_i >= 0 -- in the 50-digit reference,
    so the GPU test's invariants test the device and not the definitions."""
    case = ref.make_case(3, 37, 2, 4, None, 7, True, seed=5)
    r = ref.score_mp(case)[7]
    assert all(a >= b for a, b in zip(r["lppd_i"].reshape(-1), r["mean"].reshape(-1)))
    assert all(x >= 0 for x in (r["lppd_i"] - r["pointwise"]).reshape(-1))
    assert r["summary"]["joint_lpd"] >= r["summary"]["joint_mean"]


# ---- compare_scores ---------------------------------------------------------------------------------------------------------
def make_score(nhp, pw, bins):
    R, N = pw.shape
    summary = [3, R * N, 0.0, 0.0, pw.sum(), -2 * pw.sum(), 0.0, 0.0, 0.0, 0.0]
    return nhp.DiscreteScore(summary, np.zeros((3, N)), pw, bins)


def test_compare_scores_arithmetic_and_refusals(nhp):
    rng = np.random.default_rng(0)
    a, b = rng.normal(-1.0, 0.3, (11, 4)), rng.normal(-1.1, 0.3, (11, 4))
    sa, sb = make_score(nhp, a, (5, 16)), make_score(nhp, b, (5, 16))
    assert sa.n == 3 and sa.cells == 44 and sa.bins == (5, 16) and sa.elpd_waic == a.sum()
    c = nhp.compare_scores(sa, sb)
    d = (a - b).ravel()
    assert c.cells == 44 and c.elpd_diff == d.sum()
    assert c.se_diff == pytest.approx(math.sqrt(44 * d.var(ddof=1)), rel=1e-15)
    back = nhp.compare_scores(sb, sa)
    assert back.elpd_diff == -c.elpd_diff and back.se_diff == pytest.approx(c.se_diff, rel=1e-15)
    assert nhp.compare_scores(sa, sa).elpd_diff == 0.0 and nhp.compare_scores(sa, sa).se_diff == 0.0
    with pytest.raises(ValueError, match="different cells"):
        nhp.compare_scores(sa, make_score(nhp, a[:10], (5, 15)))
    with pytest.raises(ValueError, match="different bins"):
        nhp.compare_scores(sa, make_score(nhp, b, (6, 17)))
    with pytest.raises(ValueError, match="pointwise"):
        nhp.compare_scores(sa, nhp.DiscreteScore([3, 44] + [0.0] * 8, np.zeros((3, 4)), None, (5, 16)))


# ---- argument checks: before any library call ------------------------------------------------------------------------------
def make_process(nhp, N=3, B=2, L=4, network=False):
    th = np.full((N, N, B), 1.0 / B)
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(th, L, 1.0), nhp.DenseWeightModel(np.full((N, N), 0.1)), 1.0)
    if network:
        proc = nhp.DiscreteNetworkHawkesProcess(proc.baseline, proc.impulses, proc.weights, np.ones((N, N)), nhp.BernoulliNetworkModel(0.5, N), 1.0)
    return proc


@pytest.fixture
def no_library(nhp, monkeypatch):
    """Any reach for the library or a context fails the test."""
    from nhp_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "default_context", refuse)


def test_mcmc_refuses_bad_scoring_arguments_before_the_library(nhp, no_library):
    proc, data = make_process(nhp), np.zeros((3, 40), dtype=np.int64)
    bad = [dict(waic=True, score_every=0), dict(waic=True, score_every=1.5), dict(waic=True, burn=-1),
           dict(heldout=np.zeros((4, 40), dtype=np.int64)), dict(heldout=(data, (10, 41))), dict(heldout=(data, (10, 10))),
           dict(heldout=(data, (-1, 5))), dict(heldout=(data, 7)), dict(heldout=(data, (1, 2), 3)), dict(heldout=np.zeros(40))]
    for kw in bad:
        for route in (dict(), dict(keep_samples=False), dict(moments=True)):
            with pytest.raises(ValueError):
                nhp.mcmc_(proc, data, nsteps=2, **kw, **route)
    lgcp = make_process(nhp)
    lgcp.baseline = object.__new__(nhp.DiscreteLogGaussianCoxProcess)
    with pytest.raises(NotImplementedError, match="DiscreteLogGaussianCoxProcess"):
        nhp.mcmc_(lgcp, data, nsteps=2, waic=True)
    with pytest.raises(NotImplementedError, match="DiscreteLogGaussianCoxProcess"):
        nhp.mcmc_(lgcp, data, nsteps=2, heldout=(data, (30, 40)))


@pytest.mark.parametrize("network", [False, True])
def test_score_samples_refuses_bad_arguments_before_the_library(nhp, no_library, network):
    proc, data = make_process(nhp, network=network), np.zeros((3, 40), dtype=np.int64)
    x = proc.params()
    bad = [dict(samples=[x], every=0), dict(samples=[x], burn=-1), dict(samples=[x], burn=1), dict(samples=[]),
           dict(samples=[x], bins=(0, 41)), dict(samples=[x], bins=(3, 3)), dict(samples=[x[:-1]]), dict(samples=[x, np.append(x, 1.0)]),
           dict(samples=[x], data=np.zeros((2, 40), dtype=np.int64))]
    for kw in bad:
        kw = dict(dict(data=data), **kw)
        with pytest.raises(ValueError):
            nhp.disc_score_samples(proc, **kw)
    lgcp = make_process(nhp)
    lgcp.baseline = object.__new__(nhp.DiscreteLogGaussianCoxProcess)
    with pytest.raises(NotImplementedError, match="DiscreteLogGaussianCoxProcess"):
        nhp.disc_score_samples(lgcp, [x], data)


def test_a_standard_sample_is_scored_as_the_product_it_holds(nhp):
    """params(process) of a standard process holds η = W∘θ; the scorer takes (W, θ) = (1, η), whose bump table entry is the
    chain's W·θ bit for bit -- params!'s split multiplies back to a neighbour often enough to matter."""
    from nhp_amd import discrete
    rng = np.random.default_rng(3)
    proc = make_process(nhp, N=4, B=3)
    proc.weights.W = rng.uniform(0.01, 0.9, (4, 4))
    proc.impulses.θ = rng.dirichlet(np.ones(3), (4, 4))
    l0, W, th, A = discrete._sample_arrays(proc, proc.params())
    eta = (proc.weights.W[:, :, None] * proc.impulses.θ).ravel(order="F")
    assert A is None and np.array_equal(l0, proc.baseline.λ) and np.array_equal(np.tile(W, 3) * th, eta)
    net = make_process(nhp, network=True)
    l0, W, th, A = discrete._sample_arrays(net, net.params())
    assert np.array_equal(W, net.weights.W.ravel(order="F")) and np.array_equal(A, np.ones(9)) and th.size == 18 and l0.size == 3


def test_the_built_library_exports_the_scorer(nhp):
    from nhp_amd import _lib
    lib = _lib.lib()
    for name in ("nhp_disc_score_create", "nhp_disc_score_destroy", "nhp_disc_score_reset", "nhp_disc_score_accumulate",
                 "nhp_disc_score_fetch", "nhp_disc_score_fetch_planes", "nhp_disc_model_attach_score"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    lib.nhp_abi_version.restype = C.c_int32
    assert lib.nhp_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "nhp.h")).read()
    assert "nhp_disc_score_fetch" in header and "nhp_disc_model_attach_score" in header
