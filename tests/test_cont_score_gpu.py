"""The continuous chain scorer on the device (csrc/cont_score.hip) against the long-double / 50-digit reference of
tests/cont_score_ref.py.  The bound is DESIGN 3.24's rule with the continuous routes' tolerance as its floor: the device may
differ from the reference by 16 times the numpy restatement's error, and not less than 1e-11·max(1, Σ_i|ℓ_i|) for the sums and
1e-11·max(1, Σ|log λ_m| + ΔΛ) of the cell for a cell; every cell is held to its own bound."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cont_score_ref as ref

pytestmark = pytest.mark.gpu


def process_of(nhp, case, draw):
    N = len(draw["lam0"])
    if case["kind"] == "exponential":
        imp = nhp.ExponentialImpulseResponse(draw["theta"], Δtmax=case["dt_max"])
    else:
        imp = nhp.LogitNormalImpulseResponse(draw["mu"], draw["tau"], case["dt_max"])
    base, w = nhp.HomogeneousProcess(draw["lam0"]), nhp.DenseWeightModel(draw["W"])
    if draw["A"] is None:
        return nhp.ContinuousStandardHawkesProcess(base, imp, w)
    return nhp.ContinuousNetworkHawkesProcess(base, imp, w, draw["A"], nhp.BernoulliNetworkModel(0.5, N))


def data_of(case):
    return (case["times"], case["nodes"], case["T"])


def device_score(nhp, case, draws=None, planes=False):
    """The scripted draws through score_samples' own path: each set into a device model, accumulated, fetched."""
    from nhp_amd import _lib, inference as inf
    ctx = _lib.default_context()
    draws = case["draws"] if draws is None else draws
    proc = process_of(nhp, case, draws[0])
    ds = nhp.device_dataset(proc, data_of(case), ctx)
    scorer, model = inf._DeviceScore(ctx, ds, case["edges"]), None
    try:
        for d in draws:
            model = inf._set_score_model(model, ctx, proc, process_of(nhp, case, d).params())
            scorer.accumulate(model)
        s = scorer.fetch(pointwise=True)
        out = dict(summary={k: getattr(s, k) for k in ref.FIELDS}, per_node=s.per_node, pointwise=s.pointwise, score=s)
        if planes:
            out["planes"] = scorer.fetch_planes()
        return out
    finally:
        scorer.close()


def check_against_reference(nhp, case, label):
    r = ref.score_mp(case)
    yard = ref.errors(ref.score_numpy(case), r)
    got = device_score(nhp, case)
    err = ref.errors(got, r)
    tol = ref.tolerances(yard, r)
    cell_err = ref.pointwise_errors(got, r)
    print(f"{label}: " + ", ".join(f"{k}={err[k]:.2e}/{np.max(tol[k]) if k == 'pointwise' else tol[k]:.2e}" for k in err))
    assert np.all(cell_err <= tol["pointwise"]), (label, float(np.nanmax(cell_err / tol["pointwise"])))
    for k, v in err.items():
        if k != "pointwise" and math.isnan(tol[k]):               # undefined in the reference (se_elpd of one cell): NaN on the device too
            assert math.isnan(v), (label, k, v)
        elif k != "pointwise":
            assert v <= tol[k], (label, k, v, tol[k])
    return got, r


@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_small_case_with_every_edge(nhp, kind, network):
    """N = 3, M ≈ 40: events exactly on an edge and exactly Δtmax before one, an empty block, blocks narrower and wider than
    Δtmax, b_0 > 0 with history before it, b_K < T."""
    check_against_reference(nhp, ref.small_case(kind, network), f"N=3 {kind} network={network}")


@pytest.mark.parametrize("M,K", [(0, 2), (1, 2), (5, 1)])
@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_node(nhp, kind, M, K):
    case = ref.make_case(1, M, np.linspace(0.0, 4.0, K + 1), 7, kind, False, seed=M + K, T=4.0, dt_max=1.0)
    check_against_reference(nhp, case, f"N=1 M={M} K={K} {kind}")


@pytest.mark.parametrize("N,kind,network", [(70, "exponential", True), (70, "logitnormal", False), (300, "exponential", True)])
def test_across_a_wave_and_a_column_tile(nhp, N, kind, network):
    """M ≈ 1500, K = 20: more columns than one wave and than one 256-column tile; a node without events and an all-zero
    column of A.  (The logit-normal case keeps Δtmax short: its reference takes Φ from mpmath for every straddling pair.)"""
    M, T = 1500, 30.0
    dt = T / M * (0.5 if kind == "logitnormal" else 8.0)
    case = ref.make_case(N, M, np.linspace(0.0, T, 21), 7, kind, network, seed=N, T=T, dt_max=dt, silent_node=N // 2, zero_column=3)
    check_against_reference(nhp, case, f"N={N} {kind} network={network}")


def test_more_blocks_than_one_workgroup(nhp):
    case = ref.make_case(5, 400, np.linspace(0.0, 40.0, 258), 7, "exponential", True, seed=9, T=40.0, dt_max=0.5)
    check_against_reference(nhp, case, "N=5 K=257")


def test_infinite_window(nhp):
    case = ref.make_case(4, 300, np.linspace(0.0, 30.0, 8), 7, "exponential", False, seed=4, T=30.0, dt_max=math.inf)
    check_against_reference(nhp, case, "N=4 Δtmax=inf")


def test_lse_plane_holds_the_larger_value_bit_for_bit(nhp):
    """Two draws whose λ on a busy cell differ by 1e6: the smaller term of the log-sum-exp is below half an ulp."""
    case = ref.make_case(2, 200, [0.0, 10.0], 1, "exponential", False, seed=2, T=10.0, dt_max=0.5)
    d0 = case["draws"][0]
    d1 = dict(d0, lam0=d0["lam0"] * 1e6, W=d0["W"] * 1e6)
    one = device_score(nhp, case, [d0], planes=True)["planes"][0]
    two = device_score(nhp, case, [d0, d1], planes=True)["planes"][0]
    big = device_score(nhp, case, [d1], planes=True)["planes"][0]
    assert np.array_equal(two, np.maximum(one, big)) and not np.array_equal(one, big)


def test_one_draw_has_no_variance(nhp):
    case = ref.small_case("exponential", True)
    got = device_score(nhp, case, case["draws"][:1])
    s = got["summary"]
    assert s["n"] == 1 and all(math.isnan(s[k]) for k in ("p_waic", "elpd_waic", "waic", "se_elpd", "joint_sd"))
    assert math.isfinite(s["lppd"]) and s["joint_lpd"] == s["joint_mean"] and np.all(np.isnan(got["pointwise"]))


def test_one_draw_over_the_whole_recording_is_the_exact_loglikelihood(nhp):
    """Edges covering [0, T]: joint_mean = Σ log λ − Σ_c Λ_c(T), from the library's own total_intensity and compensator."""
    for kind in ("exponential", "logitnormal"):
        case = ref.make_case(6, 800, np.linspace(0.0, 20.0, 12), 1, kind, True, seed=6, T=20.0, dt_max=0.25)
        proc = process_of(nhp, case, case["draws"][0])
        lam = nhp.total_intensity(proc, data_of(case))
        total = nhp.compensator(proc, data_of(case)).total
        want = math.fsum(np.log(lam)) - math.fsum(total)
        got = device_score(nhp, case)["summary"]["joint_mean"]
        scale = math.fsum(np.abs(np.log(lam))) + math.fsum(total)
        assert abs(got - want) <= 1e-11 * max(1.0, scale), (kind, got, want)


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------------
def test_refusals_at_the_c_abi(nhp):
    from nhp_amd import _lib, inference as inf
    lib, ctx = _lib.lib(), _lib.default_context()
    case = ref.small_case("exponential", False)
    proc = process_of(nhp, case, case["draws"][0])
    ds = nhp.device_dataset(proc, data_of(case), ctx)
    model = proc.device_model(ctx)

    def create(edges, dsh=ds.h):
        h, e = C.c_void_p(), _lib.f64(edges)
        rc = lib.nhp_cont_score_create(ctx.h, dsh, _lib.dptr(e), len(e), C.byref(h))
        if rc == 0:
            lib.nhp_cont_score_destroy(h)
        return rc
    EINVAL, ENOTIMPL = _lib.EINVAL, _lib.ENOTIMPL
    assert create([0.0, 1.0]) == 0
    for edges in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.0, math.nan], [0.0, math.inf], [-1.0, 1.0], [0.0, 8.5]):
        assert create(edges) == EINVAL, edges
    assert create([0.0, 1.0], None) == EINVAL
    e = _lib.f64([0.0, 1.0])
    assert lib.nhp_cont_score_create(ctx.h, ds.h, _lib.dptr(e), 2, None) == EINVAL
    # several trials, a column shard
    trials = nhp.device_dataset(proc, [data_of(case), data_of(case)], ctx)
    assert create([0.0, 1.0], trials.h) == ENOTIMPL and "trials" in lib.nhp_last_error(ctx.h).decode()
    shard = nhp.DeviceDataset(ctx, data_of(case), 3, case["dt_max"], columns=(0, 2))
    assert create([0.0, 1.0], shard.h) == ENOTIMPL and "column shard" in lib.nhp_last_error(ctx.h).decode()
    # fetch before accumulate, null handles, a third scorer, another Δtmax, an LGCP baseline
    scorers = [inf._DeviceScore(ctx, ds, [0.0, 4.0, 8.0]) for _ in range(3)]
    try:
        s, p = np.empty(10), np.empty(9)
        assert lib.nhp_cont_score_fetch(ctx.h, scorers[0].h, _lib.dptr(s), _lib.dptr(p), None) == EINVAL
        assert "nothing accumulated" in lib.nhp_last_error(ctx.h).decode()
        assert lib.nhp_cont_score_fetch_planes(ctx.h, scorers[0].h, None, None, None) == EINVAL
        assert lib.nhp_cont_score_accumulate(ctx.h, None, model.h) == EINVAL
        assert lib.nhp_cont_score_accumulate(ctx.h, scorers[0].h, None) == EINVAL
        assert lib.nhp_cont_score_reset(ctx.h, None) == EINVAL
        assert lib.nhp_cont_model_attach_score(ctx.h, None, scorers[0].h, 1) == EINVAL
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorers[0].h, 0) == EINVAL
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorers[0].h, 1) == 0
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorers[0].h, 2) == 0          # the same scorer again: its slot
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorers[1].h, 1) == 0
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorers[2].h, 1) == EINVAL
        assert "at most two" in lib.nhp_last_error(ctx.h).decode()
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, None, 1) == 0
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorers[2].h, 1) == 0
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, None, 1) == 0
        other = process_of(nhp, dict(case, dt_max=0.25), case["draws"][0]).device_model(ctx)
        assert lib.nhp_cont_score_accumulate(ctx.h, scorers[0].h, other.h) == EINVAL
        four = ref.make_case(4, 5, [0.0, 1.0], 1, "exponential", False, 1, T=8.0, dt_max=0.5)
        assert lib.nhp_cont_score_accumulate(ctx.h, scorers[0].h, process_of(nhp, four, four["draws"][0]).device_model(ctx).h) == _lib.ESHAPE
        d0 = case["draws"][0]
        lg = nhp.ContinuousStandardHawkesProcess(nhp.LogGaussianCoxProcess([0.0, 4.0, 8.0], [np.ones(3)] * 3),
                                                 nhp.ExponentialImpulseResponse(d0["theta"], Δtmax=0.5), nhp.DenseWeightModel(d0["W"]))
        assert lib.nhp_cont_score_accumulate(ctx.h, scorers[0].h, lg.device_model(ctx).h) == ENOTIMPL
        assert "LGCP" in lib.nhp_last_error(ctx.h).decode()
    finally:
        for s in scorers:
            s.close()


# ---- chains ------------------------------------------------------------------------------------------------------------------
def chain_process(nhp, N, network, seed=0):
    rng = np.random.default_rng(seed)
    base, imp = nhp.HomogeneousProcess(rng.uniform(0.5, 1.5, N)), nhp.ExponentialImpulseResponse(rng.uniform(2.0, 6.0, (N, N)), Δtmax=0.5)
    w = nhp.DenseWeightModel(rng.uniform(0.05, 0.3, (N, N)) / N)
    if network:
        return nhp.ContinuousNetworkHawkesProcess(base, imp, w, np.ones((N, N)), nhp.BernoulliNetworkModel(0.5, N))
    return nhp.ContinuousStandardHawkesProcess(base, imp, w)


@functools.lru_cache(maxsize=None)
def chain_data(N=6, M=800):
    rng = np.random.default_rng(77)
    T = M / (1.2 * N)
    return np.sort(rng.uniform(0.0, T, M)), rng.integers(1, N + 1, M), T


def bits(score):
    return np.concatenate([[getattr(score, k) for k in ref.FIELDS], score.per_node.ravel(), score.pointwise.ravel()]).tobytes()


@pytest.mark.parametrize("network", [False, True])
def test_routes_and_repeats_give_the_same_bits(nhp, network):
    """N = 6, M ≈ 800, 30 steps: the resident chain in one call and twice, the step-by-step device route, and score_samples on
    the kept samples of the same chain."""
    data, K, kw = chain_data(), 7, dict(nsteps=30, seed=5, burn=4, score_every=2, pointwise=True)
    resident = [nhp.mcmc_(chain_process(nhp, 6, network), data, keep_samples=False, waic=K, **kw).waic for _ in range(2)]
    stepwise = nhp.mcmc_(chain_process(nhp, 6, network), data, keep_samples=True, waic=K, **kw)
    again = nhp.score_samples(chain_process(nhp, 6, network), stepwise.samples, data, K, burn=4, every=2, pointwise=True)
    assert resident[0].n == 13 and resident[0].cells == K * 6
    assert bits(resident[0]) == bits(resident[1]) == bits(stepwise.waic) == bits(again)
    cmp = nhp.compare_scores(resident[0], again)
    assert cmp.elpd_diff == 0.0 and cmp.cells == K * 6


def test_resident_chain_cut_into_three_calls(nhp):
    """verbose cuts the resident chain at the log points: the scorers' kept count persists across the calls."""
    data, kw = chain_data(), dict(nsteps=30, seed=5, burn=4, score_every=3, pointwise=True, keep_samples=False, waic=5)
    one = nhp.mcmc_(chain_process(nhp, 6, True), data, **kw).waic
    three = nhp.mcmc_(chain_process(nhp, 6, True), data, verbose=True, log_freq=10, **kw).waic
    assert one.n == 9 and bits(one) == bits(three)


def test_invariants_on_a_real_chain(nhp):
    from nhp_amd import _lib, inference as inf
    ctx, data = _lib.default_context(), chain_data()
    proc = chain_process(nhp, 6, True)
    res = nhp.mcmc_(proc, data, nsteps=25, seed=1, keep_samples=True, heldout=(data, [10.0, 40.0, 41.0, 100.0]), pointwise=True)
    s = res.heldout
    assert s.n == 25 and s.cells == 18 and s.bins == (10.0, 40.0, 41.0, 100.0)
    assert np.allclose(s.per_node.sum(axis=1), [s.lppd, s.p_waic, s.elpd_waic], rtol=1e-13, atol=0)
    assert s.joint_lpd >= s.joint_mean and s.waic == -2.0 * s.elpd_waic
    ds = nhp.device_dataset(proc, data, ctx)
    scorer, model = inf._DeviceScore(ctx, ds, [10.0, 40.0, 41.0, 100.0]), None
    try:
        for x in res.samples:
            model = inf._set_score_model(model, ctx, proc, x)
            scorer.accumulate(model)
        lse, mean, m2 = scorer.fetch_planes()
    finally:
        scorer.close()
    assert np.all(m2 >= 0.0)
    assert np.all(lse - math.log(25) >= mean - 4 * np.spacing(np.abs(mean)))


def test_chain_without_the_new_arguments_is_untouched(nhp):
    """res.mean of a short resident chain: before any scorer was attached to the cached model, and after one was."""
    data, kw = chain_data(), dict(nsteps=12, seed=3, keep_samples=False, moments=True, burn=2)
    proc = chain_process(nhp, 6, True)
    start = proc.params()

    def run(**extra):
        proc.network.ρ = 0.5
        _set(proc, start)
        return nhp.mcmc_(proc, data, **kw, **extra)
    before = run().mean
    scored = run(waic=4)
    after = run().mean
    assert scored.waic.n == 10 and np.array_equal(scored.mean, before) and np.array_equal(after, before)


def _set(proc, x):
    N = proc.ndims()
    NN = N * N
    k = len(proc.network.params())
    proc.baseline.λ = x[k:k + N].copy()
    proc.weights.params_(x[k + N:k + N + NN])
    proc.impulses.params_(x[k + N + NN:k + N + 2 * NN])
    proc.adjacency_matrix = x[k + N + 2 * NN:].reshape((N, N), order="F").copy()


# ---- the remaining routes, network models and refusals ---------------------------------------------------------------------------
def test_host_draw_route_scores_what_score_samples_scores(nhp):
    """device_draws=False: every scored step's params(process) -- the network's own leading parameters included -- is set into
    a device model kept for scoring; the kept samples scored afterwards give the same bits."""
    data, kw = chain_data(), dict(nsteps=12, seed=8, burn=3, score_every=2, pointwise=True)
    for network in (False, True):
        res = nhp.mcmc_(chain_process(nhp, 6, network), data, keep_samples=True, device_draws=False, waic=5,
                        heldout=(data, [60.0, 80.0, 111.0]), **kw)
        again = nhp.score_samples(chain_process(nhp, 6, network), res.samples, data, 5, burn=3, every=2, pointwise=True)
        held = nhp.score_samples(chain_process(nhp, 6, network), res.samples, data, [60.0, 80.0, 111.0], burn=3, every=2, pointwise=True)
        assert res.waic.n == 5 and bits(res.waic) == bits(again) and bits(res.heldout) == bits(held)
        assert nhp.compare_scores(res.waic, again).elpd_diff == 0.0


def family_process(nhp, which, N=6):
    rng = np.random.default_rng(1)
    base, w = nhp.HomogeneousProcess(rng.uniform(0.5, 1.5, N)), nhp.DenseWeightModel(rng.uniform(0.05, 0.3, (N, N)) / N)
    if which == "logitnormal":
        return nhp.ContinuousStandardHawkesProcess(base, nhp.LogitNormalImpulseResponse(np.zeros((N, N)), np.ones((N, N)), 0.5), w)
    imp = nhp.ExponentialImpulseResponse(rng.uniform(2.0, 6.0, (N, N)), Δtmax=0.5)
    net = {"dense": lambda: nhp.DenseNetworkModel(N), "block": lambda: nhp.StochasticBlockNetworkModel(N, 2),
           "latent": lambda: nhp.LatentDistanceNetworkModel(N, 2)}[which]()
    return nhp.ContinuousNetworkHawkesProcess(base, imp, w, np.ones((N, N)), net)


@pytest.mark.parametrize("which", ["dense", "block", "latent", "logitnormal"])
def test_other_network_models_and_the_logit_normal_family(nhp, which):
    """A dense, a block and a latent distance network chain and a logit-normal chain, scorers attached: the resident chain
    twice gives the same bits, and the step-by-step chain's score is that of score_samples on its kept samples."""
    data, kw = chain_data(), dict(nsteps=14, seed=2, burn=4, score_every=2, pointwise=True, waic=6)
    resident = [nhp.mcmc_(family_process(nhp, which), data, keep_samples=False, **kw).waic for _ in range(2)]
    stepwise = nhp.mcmc_(family_process(nhp, which), data, keep_samples=True, **kw)
    again = nhp.score_samples(family_process(nhp, which), stepwise.samples, data, 6, burn=4, every=2, pointwise=True)
    assert resident[0].n == 5 and resident[0].cells == 36 and np.all(np.isfinite(resident[0].pointwise))
    assert bits(resident[0]) == bits(resident[1]) and bits(stepwise.waic) == bits(again)
    assert resident[0].joint_lpd >= resident[0].joint_mean and resident[0].p_waic >= 0


def test_mcmc_run_refuses_a_column_shard_with_a_scorer_attached(nhp):
    from nhp_amd import _lib, inference as inf
    lib, ctx = _lib.lib(), _lib.default_context()
    case = ref.small_case("exponential", False)
    proc = process_of(nhp, case, case["draws"][0])
    ds = nhp.device_dataset(proc, data_of(case), ctx)
    shard = nhp.DeviceDataset(ctx, data_of(case), 3, case["dt_max"], columns=(0, 2))
    model, pri = proc.device_model(ctx), inf._priors(proc)
    scorer = inf._DeviceScore(ctx, ds, [0.0, 4.0, 8.0])
    try:
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, scorer.h, 1) == 0
        assert lib.nhp_cont_mcmc_run(ctx.h, None, shard.h, model.h, C.byref(pri), 0.0, 0.0, 1, 0, 2, -1) == _lib.ENOTIMPL
        assert "column shard" in lib.nhp_last_error(ctx.h).decode()
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, None, 1) == 0
        assert lib.nhp_cont_mcmc_run(ctx.h, None, shard.h, model.h, C.byref(pri), 0.0, 0.0, 1, 0, 2, -1) == 0
    finally:
        lib.nhp_cont_model_attach_score(ctx.h, model.h, None, 1)
        scorer.close()


def test_lds_column_budget_and_out_of_memory(nhp):
    """N = 10 300 exponential columns are past the per-event intensity's 160 KiB of LDS: attach and accumulate are
    NHP_ENOTIMPL.  On the same dataset 2·10⁶ blocks ask for 494 GB of planes, more than the device has: NHP_ENOMEM, and a
    scorer made right after works."""
    from nhp_amd import _lib, continuous
    lib, ctx = _lib.lib(), _lib.default_context()
    N, T = 10_300, 8.0
    ds = nhp.DeviceDataset(ctx, (np.array([1.0, 2.0, 2.25]), np.array([1, N, 7]), T), N, 0.5)
    table, l0 = np.full(N * N, 1e-4), np.ones(N)
    d = _lib.ModelDesc()
    d.n_nodes, d.baseline_kind, d.grid_n, d.impulse_kind, d.dt_max = N, _lib.BASELINE_HOMOGENEOUS, 0, _lib.IMPULSE_EXPONENTIAL, 0.5
    d.lambda0, d.theta, d.W = _lib.dptr(l0), _lib.dptr(table), _lib.dptr(table)
    model = continuous.DeviceModel(ctx, d)

    def create(edges):
        h, e = C.c_void_p(), _lib.f64(edges)
        return lib.nhp_cont_score_create(ctx.h, ds.h, _lib.dptr(e), len(e), C.byref(h)), h
    rc, h = create([0.0, 4.0, T])
    assert rc == 0
    try:
        assert lib.nhp_cont_score_accumulate(ctx.h, h, model.h) == _lib.ENOTIMPL
        assert "LDS column budget" in lib.nhp_last_error(ctx.h).decode()
        assert lib.nhp_cont_model_attach_score(ctx.h, model.h, h, 1) == _lib.ENOTIMPL
    finally:
        lib.nhp_cont_score_destroy(h)
    rc, h = create(np.linspace(0.0, T, 2_000_001))
    assert rc == _lib.ENOMEM and not h.value and "out of device memory" in lib.nhp_last_error(ctx.h).decode()
    rc, h = create([0.0, T])
    assert rc == 0
    lib.nhp_cont_score_destroy(h)
