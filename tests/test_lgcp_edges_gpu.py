"""The Gibbs update of a log Gaussian Cox baseline on the GPU against tests/lgcp_ref.py: the candidate log-likelihoods
(nhp_cont_lgcp_loglik, nhp_disc_lgcp_loglik) inside the ref's derived rounding bound at the grid's edges, the hand-over of the
parent sampler's attribution, the refusals, the other copies of the piecewise-linear interpolator on a grid with events on its
knots, the lock-step elliptical-slice loops against the serial restatement, their invariance, and one mcmc_ step.

A run prints the largest error / bound per case, the Kolmogorov-Smirnov p-values and the decision margins.
tests/test_lgcp_edges_host.py shows that the invariance harness rejects three mutants."""
import contextlib
import os

import numpy as np
import pytest

import lgcp_ref as ref

pytestmark = pytest.mark.gpu

ENV = ("NHP_SAMPLER", "NHP_CHUNK", "NHP_SORT", "NHP_SLICES", "NHP_SAMPLER_SLICES", "NHP_SAMPLER_EXPO_SLICES", "NHP_SAMPLER_CFG")


@contextlib.contextmanager
def environment(**env):
    """The route switches cleared, `env` set (None: left unset), everything put back afterwards."""
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    try:
        yield
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def dataset(nhp, case, chunk=None, sort=None, columns=None):
    with environment(NHP_CHUNK=chunk, NHP_SORT=sort):
        return nhp.continuous.DeviceDataset(nhp.default_context(), (case["times"], case["nodes"], case["T"]), case["N"], case["dt_max"],
                                            columns=columns)


def baseline_of(nhp, case):
    return nhp.LogGaussianCoxProcess(case["grid_x"].copy(), [row.copy() for row in case["lam"]], None, 0.0)


# --------------------------------------------------------------------------------------- candidate log-likelihood, continuous
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_continuous_candidate_loglikelihood_inside_the_bound(nhp, name):
    case, res = ref.prepared(name)
    base, ds = baseline_of(nhp, case), dataset(nhp, case)
    got = base.candidate_loglikelihood(ds, case["Y"], parentnodes=case["parentnodes"])
    r, bad = ref.ratio(got, res)
    print(f"continuous {name}: largest error/bound {r:.3g} (n up to {int(res.n.max())}, G = {len(case['grid_x'])})")
    assert len(bad) == 0, (name, r, got, np.asarray(res.ll, dtype=np.float64))
    # a node without baseline events: the trapezoids alone, which the kernel adds in grid order
    pn = case.get("parentnodes_none")
    if pn is not None:
        got = base.candidate_loglikelihood(ds, case["Y"], parentnodes=pn)
    for c in range(case["N"]):
        if pn is not None or res.n[c] == 0:
            assert got[c] == 0.0 - ref.sequential_trapezoid(case["grid_x"], case["lam"][c]), (name, c)
    assert pn is not None or (res.n == 0).sum() >= 1


# ------------------------------------------------------------------------------------------------------ the knots process
def knots_model(nhp, orc, kind="exponential", network=False, scale=1.0, seed=31, own_curves=False):
    """A process on the knots case whose baseline is the case's curves (own_curves: curves of its own), with weights small
    enough that the baseline takes a good part of the events; returns (process, oracle model)."""
    case = ref.prepared("knots")[0]
    rng = np.random.default_rng(seed)
    N = case["N"]
    W = rng.uniform(0.0, 0.1, (N, N)) * scale
    theta = rng.uniform(1.0, 5.0, (N, N))
    mu, tau = rng.normal(0.0, 1.0, (N, N)), rng.uniform(0.5, 2.0, (N, N))
    A = (rng.uniform(size=(N, N)) < 0.6).astype(np.float64) if network else None
    lam = np.exp(rng.normal(0.0, 0.6, case["lam"].shape)) if own_curves else case["lam"]
    base = nhp.LogGaussianCoxProcess(case["grid_x"].copy(), [row.copy() for row in lam], None, 0.0)
    if kind == "exponential":
        imp = nhp.ExponentialImpulseResponse(theta, 1.0, 1.0, case["dt_max"])
        om = orc.ContModel(lam, W, theta=theta, dt_max=case["dt_max"], A=A, grid_x=case["grid_x"])
    else:
        imp = nhp.LogitNormalImpulseResponse(mu, tau, case["dt_max"])
        om = orc.ContModel(lam, W, mu=mu, tau=tau, dt_max=case["dt_max"], A=A, grid_x=case["grid_x"])
    if network:
        proc = nhp.ContinuousNetworkHawkesProcess(base, imp, nhp.DenseWeightModel(W), A, nhp.BernoulliNetworkModel(0.5, N))
    else:
        proc = nhp.ContinuousStandardHawkesProcess(base, imp, nhp.DenseWeightModel(W))
    return proc, om


def routed_dataset(nhp, case, route, sort=None):
    """The dataset of a sampler route: "1" / "8" (the lane-per-child and the 8-lane kernel on the default layout) or "slices"
    (items of 256, which keep their child slices: tests/slices_ref.py says so for this case)."""
    ds = dataset(nhp, case, chunk="256" if route == "slices" else None, sort=sort)
    assert (ds.scalars()["sl_rows"] > 0) == (route == "slices")
    return ds


def sampler_env(route):
    return {} if route == "slices" else {"NHP_SAMPLER": route}


# ------------------------------------------------------------------------------------------------- attribution hand-over
@pytest.mark.parametrize("sort", ["0", "1", None])
@pytest.mark.parametrize("route", ["1", "8", "slices"])
def test_the_samplers_attribution_reaches_the_candidate_loglikelihood(nhp, orc, route, sort):
    case = ref.prepared("knots")[0]
    proc, _ = knots_model(nhp, orc)
    ds = routed_dataset(nhp, case, route, sort)
    Y = case["Y"]

    def want(pn):
        return ref.cont_candidate_ll(case["times"], case["nodes"], pn, case["N"], case["grid_x"], case["lam"])

    def inside(got, pn):
        r, bad = ref.ratio(got, want(pn))
        assert len(bad) == 0, (route, sort, r)

    with environment(**sampler_env(route)):
        _, pn1 = nhp.resample_parents(proc, ds, seed=9, step=2)
        inside(proc.baseline.candidate_loglikelihood(ds, Y), pn1)
        _, pn2 = nhp.resample_parents(proc, ds, seed=10, step=2)
        assert not np.array_equal(pn1 == 0, pn2 == 0) and 0.2 < np.mean(pn2 == 0) < 0.9
        got2 = proc.baseline.candidate_loglikelihood(ds, Y)
        inside(got2, pn2)                                              # the second sweep's attribution, not the first's
        assert np.max(np.abs(got2 - np.asarray(want(pn1).ll, dtype=np.float64))) > 1e-3
    inside(proc.baseline.candidate_loglikelihood(ds, Y, parentnodes=case["parentnodes"]), case["parentnodes"])
    inside(proc.baseline.candidate_loglikelihood(ds, Y), case["parentnodes"])      # an explicit vector replaces it for later calls


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(nhp, orc):
    from nhp_amd import _lib
    case, res = ref.prepared("knots")
    N, gx, lam, M = case["N"], case["grid_x"], case["lam"], len(case["times"])
    ctx = nhp.default_context()
    ds = dataset(nhp, case)
    base = baseline_of(nhp, case)
    first = base.candidate_loglikelihood(ds, case["Y"], parentnodes=case["parentnodes"])
    SENTINEL = -12345.5

    def call(ds_, pn, x, lam_):
        out = np.full(N, SENTINEL)
        x, lam_ = _lib.f64(x), _lib.f64(np.asarray(lam_).ravel())
        pn = None if pn is None else np.ascontiguousarray(pn, dtype=np.int64)
        rc = _lib.lib().nhp_cont_lgcp_loglik(ctx.h, ds_.h, _lib.iptr(pn), _lib.dptr(x), len(x), _lib.dptr(lam_), _lib.dptr(out))
        return rc, out

    wide = np.linspace(0.0, case["T"], 4097)
    swapped = gx.copy()
    swapped[2], swapped[3] = gx[3], gx[2]
    repeated = gx.copy()
    repeated[3] = repeated[2]
    bad_hi, bad_lo = case["parentnodes"].copy(), case["parentnodes"].copy()
    bad_hi[M // 2], bad_lo[M - 1] = N + 1, -1
    trials = nhp.continuous.DeviceDataset(ctx, [(case["times"], case["nodes"], case["T"])] * 2, N, case["dt_max"])
    assert trials.ntrials == 2
    refusals = [
        ("G = 1", ds, None, gx[:1], lam[:, :1], _lib.ESHAPE),
        ("G = 4097", ds, None, wide, np.ones((N, 4097)), _lib.ESHAPE),
        ("grid goes back", ds, None, swapped, lam, _lib.EDOMAIN),
        ("grid point repeated", ds, None, repeated, lam, _lib.EDOMAIN),
        ("grid starts after 0", ds, None, np.concatenate([[0.25], gx[1:]]), lam, _lib.EDOMAIN),
        ("event beyond the grid", ds, None, np.concatenate([gx[:-1], [gx[-1] - 0.125]]), lam, _lib.EDOMAIN),
        ("parent node N + 1", ds, bad_hi, gx, lam, _lib.EDOMAIN),
        ("parent node -1", ds, bad_lo, gx, lam, _lib.EDOMAIN),
        ("no attribution yet", dataset(nhp, case), None, gx, lam, _lib.EINVAL),
        ("column shard", dataset(nhp, case, columns=(0, 2)), case["parentnodes"], gx, lam, _lib.ENOTIMPL),
        ("several trials", trials, None, gx, lam, _lib.ENOTIMPL),
    ]
    for what, ds_, pn, x, lam_, status in refusals:
        rc, out = call(ds_, pn, x, lam_)
        assert rc == status and rc != _lib.OK, (what, rc, status)
        assert np.all(out == SENTINEL), what
        rc, out = call(ds, None, gx, lam)                                  # the earlier attribution is still there
        assert rc == _lib.OK and np.array_equal(out, first), what
    # the Python surface raises what the statuses stand for
    with pytest.raises(nhp.DomainError):
        nhp.LogGaussianCoxProcess(gx * 0.5, list(lam)).candidate_loglikelihood(ds, case["Y"])
    with pytest.raises(nhp.NhpError):
        base.candidate_loglikelihood(dataset(nhp, case), case["Y"])


# ----------------------------------------------------------------------------------------- candidate log-likelihood, discrete
def disc_process(nhp, d, W):
    N = d["N"]
    L, B = 3, 2
    th = np.full((N, N, B), 0.5)
    base = nhp.DiscreteLogGaussianCoxProcess(d["grid_x"].copy(), d["lam"].copy(), None, d["m"], d["dt"])
    return nhp.DiscreteStandardHawkesProcess(base, nhp.DiscreteGaussianImpulseResponse(th, L, d["dt"]), nhp.DenseWeightModel(W), d["dt"])


@pytest.mark.parametrize("name", sorted(ref.DISC_CASES))
def test_discrete_candidate_loglikelihood_inside_the_bound(nhp, orc, name):
    d = ref.disc_case(name)
    N, T = d["N"], d["T"]
    cand = np.exp(d["m"] + d["Y"])
    # W = 0: every count is a baseline count, whatever the sampler draws
    proc = disc_process(nhp, d, np.zeros((N, N)))
    ds = nhp.convolve(proc, d["data"])
    counts = nhp.resample_parent_counts(proc, convolved=ds, seed=3, step=1)
    assert np.array_equal(counts[:, 0], d["data"].sum(axis=1)) and counts[:, 1:].sum() == 0
    res = ref.disc_candidate_ll(d["data"].T, d["grid_x"], cand, d["dt"])
    r0, bad = ref.ratio(proc.baseline.candidate_loglikelihood(ds, d["Y"]), res)
    assert len(bad) == 0, (name, r0)
    # W > 0: the baseline counts of the oracle's sampler, which the device sampler equals
    rng = np.random.default_rng(5)
    proc = disc_process(nhp, d, rng.uniform(0.0, 0.6, (N, N)) / N)
    ds, conv = nhp.convolve(proc, d["data"], fetch=True)
    b = proc.baseline
    base_tn = orc.disc_lgcp_intensity(b.x, b.λ, b.dt, np.arange(1, T + 1, dtype=np.float64))
    got_counts = nhp.resample_parent_counts(proc, convolved=ds, seed=4, step=2)
    wc, wb = orc.disc_resample_parents_b(d["data"], conv, base_tn, proc.weights.W, proc.impulses.θ, proc.dt, seed=4, step=2)
    assert np.array_equal(got_counts, wc)
    res = ref.disc_candidate_ll(wb, d["grid_x"], cand, d["dt"])
    r1, bad = ref.ratio(b.candidate_loglikelihood(ds, d["Y"]), res)
    print(f"discrete {name}: largest error/bound {r0:.3g} (W = 0), {r1:.3g} (W > 0); baseline share {wb.sum() / max(1, d['data'].sum()):.2f}")
    assert len(bad) == 0, (name, r1)


# ------------------------------------------------------------------- the interpolator copies that have not met a knot
def knot_uniforms(M):
    u = np.random.default_rng(17).uniform(size=M)
    u[::97] = 0.0
    u[5::89] = np.nextafter(1.0, 0.0)
    return u


@pytest.mark.parametrize("route", ["1", "8", "slices"])
@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_samplers_on_knots_give_the_oracle_indices(nhp, orc, kind, network, route):
    case = ref.prepared("knots")[0]
    proc, om = knots_model(nhp, orc, kind, network)
    ds = routed_dataset(nhp, case, route)
    u = knot_uniforms(len(case["times"]))
    wp, wpn = orc.resample_parents(om, case["times"], case["nodes"], u, flags=orc.MATH_DET)
    assert np.mean(wpn == 0) >= 0.2                                    # the baseline's weight decides a good part of the draws
    with environment(**sampler_env(route)):
        p, pn = nhp.resample_parents(proc, ds, u=u)
    assert np.array_equal(p, wp) and np.array_equal(pn, wpn)


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_loglikelihood_and_intensity_on_knots(nhp, orc, kind, network, sliced):
    case = ref.prepared("knots")[0]
    proc, om = knots_model(nhp, orc, kind, network)
    ds = routed_dataset(nhp, case, "slices" if sliced else "1")
    t, n, T = case["times"], case["nodes"], case["T"]
    want = orc.loglik(om, t, n, T, recursive=False)
    assert abs(nhp.loglikelihood(proc, ds, recursive=False) - want) < 1e-11 * abs(want)
    if kind == "exponential":
        want = orc.loglik(om, t, n, T, recursive=True)
        assert abs(nhp.loglikelihood(proc, ds, recursive=True) - want) < 1e-11 * abs(want)
    lam = nhp.total_intensity(proc, ds)
    assert np.max(np.abs(lam - orc.total_intensity(om, t, n)) / lam) < 1e-12


@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_batched_loglikelihoods_on_knots(nhp, orc, kind, network):
    """Six models of one kind on the default dataset through nhp_cont_loglik_batch: compatible models (same kinds, grid length
    and mask presence) at a mean window below 96 on a dataset without child slices go four, then two, at a time through
    k_windowed_batch, whose baseline is baseline_at_p.  Every model has its own curves, weights, impulse parameters and
    mask, so a value computed from another model's curve or grid pointer is a different number; each is held to the oracle.
    (A pair of such models given to nhp_cont_loglik_enqueue is not paired -- a shared pass needs a homogeneous baseline -- and
    runs the synchronous route that test_loglikelihood_and_intensity_on_knots covers.)"""
    from test_enqueue_pairs_gpu import batch_ll, device_model
    case = ref.prepared("knots")[0]
    ctx = nhp.default_context()
    t, n, T = case["times"], case["nodes"], case["T"]
    ds = routed_dataset(nhp, case, "1")
    assert ds.pairs / len(t) <= 96.0
    procs = [knots_model(nhp, orc, kind, network, seed=100 + q, own_curves=True) for q in range(6)]
    models = [device_model(nhp, ctx, p) for p, _ in procs]
    got = batch_ll(nhp, ctx, ds, models)
    want = np.array([orc.loglik(om, t, n, T, recursive=False) for _, om in procs])
    assert len(set(want)) == 6
    assert np.all(np.abs(got - want) < 1e-11 * np.abs(want)), (got, want)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_most_likely_parents_on_knots(nhp, orc, kind):
    import cascades_ref as cf
    import compensator_ref as cr
    case = ref.prepared("knots")[0]
    proc, _ = knots_model(nhp, orc, kind, network=True, scale=5.0)      # weights at which parents and baseline compete
    want = cf.map_parents_ref(cr.Model.of(proc), case["times"], case["nodes"])
    assert float(want.gap[1:].min()) >= 1e-9 and 0.2 <= np.mean(want.parents == 0) <= 0.8
    par, pno, prob = nhp.map_parents(proc, (case["times"], case["nodes"], case["T"]))
    assert np.array_equal(par, want.parents) and np.array_equal(pno, want.parentnodes)
    assert np.max(np.abs(prob - want.prob)) <= 1e-11


# ------------------------------------------------------------------------------------------------ lock step equals serial
def test_continuous_lock_step_equals_the_serial_loop(nhp):
    """Seed ref.LOCK_SEED_CONT: rounds 4, 5, 2, 1, 3, 1 over the six nodes, both bracket ends moved, smallest |ll_new - level| of
    any decision 26.6 against a likelihood bound of 2.4e-11."""
    case = ref.lockstep_cont_case()
    N, G = case["N"], len(case["grid_x"])
    base = nhp.LogGaussianCoxProcess(case["grid_x"].copy(), [r.copy() for r in case["lam"]], case["Sigma"].copy(), case["m"])
    ds = nhp.continuous.DeviceDataset(nhp.default_context(), (case["times"], case["nodes"], case["T"]), N, case["dt_max"])
    # one attempt is not enough for this seed: the error is raised and the curves stay
    before = [v.copy() for v in base.λ]
    with pytest.raises(RuntimeError):
        base.resample_(ds, ref.ScriptedRng(ref.LOCK_SEED_CONT), parentnodes=case["parentnodes"], max_attempts=1)
    assert all(np.array_equal(a, b) for a, b in zip(before, base.λ))
    rng = ref.ScriptedRng(ref.LOCK_SEED_CONT)
    new = np.vstack(base.resample_(ds, rng))
    res, bound = ref.serial_update(case, rng.record, "rows")
    cond = ref.lockstep_conditions(res, bound)
    print("continuous lock step:", cond)
    assert cond["clear"] and cond["first"] and cond["long"] and cond["both"], cond
    assert len(rng.record) == 2 + max(cond["rounds"])                  # one normal array, log u, one uniform array per round
    want = np.exp(case["m"] + np.vstack([r.y for r in res]))
    np.testing.assert_allclose(new, want, rtol=1e-14, atol=0.0)
    # What holds resample_ itself to the serial loop is the new λ above and the length of the record.  θ and the rounds it
    # does not return: the replay below is this file's copy of the lock-step loop, so it checks the decisions the GPU
    # likelihood takes on the recorded draws, not resample_'s bookkeeping.
    theta, rounds = replay_lock_step(lambda Y: base.candidate_loglikelihood(ds, Y), np.log(case["lam"]) - case["m"],
                                     np.linalg.cholesky(case["Sigma"]), rng.record, "rows")
    assert np.array_equal(theta, [r.theta for r in res]) and np.array_equal(rounds, cond["rounds"])


def replay_lock_step(loglik, Y, L, record, layout):
    """The accepted θ and the rounds of every node when the recorded draws meet the likelihood `loglik` (all nodes per call)
    in lock step.  A copy of the loop written here, not resample_: it shows which decisions that likelihood takes."""
    rows = layout == "rows"
    ax = (lambda v: v[:, None]) if rows else (lambda v: v[None, :])
    Z = record[0][1]
    V = Z @ L.T if rows else L @ Z
    unis = [a for k, a in record[1:]]
    level = loglik(Y) + np.log(unis[0])
    theta = 2 * np.pi * unis[1]
    tmin, tmax = theta - 2 * np.pi, theta.copy()
    N = len(theta)
    rounds, done = np.ones(N, dtype=np.int64), np.zeros(N, dtype=bool)
    r = 1
    while True:
        done = done | (~done & (loglik(Y * ax(np.cos(theta)) + V * ax(np.sin(theta))) >= level))
        if done.all():
            return theta, rounds
        r += 1
        todo = ~done
        neg = theta < 0.0
        tmin, tmax = np.where(todo & neg, theta, tmin), np.where(todo & ~neg, theta, tmax)
        theta = np.where(todo, tmin + (tmax - tmin) * unis[r], theta)
        rounds[todo] += 1


def test_discrete_lock_step_equals_the_serial_loop(nhp):
    """Seed ref.LOCK_SEED_DISC: rounds 11, 4, 1, 3, 2, 1, both bracket ends moved, smallest |ll_new - level| 2.14 against a
    likelihood bound of 1.1e-10."""
    case = ref.lockstep_disc_case()
    N, T = case["N"], case["T"]
    d = dict(case, lam=case["lam"])
    proc = disc_process(nhp, d, np.zeros((N, N)))
    proc.baseline.Σ = case["Sigma"].copy()
    base = proc.baseline
    ds = nhp.convolve(proc, case["data"])
    nhp.resample_parent_counts(proc, convolved=ds, seed=1, step=0)          # W = 0: the baseline counts are the data
    before = base.λ.copy()
    with pytest.raises(RuntimeError):
        base.resample_(ds, ref.ScriptedRng(ref.LOCK_SEED_DISC), max_attempts=1)
    assert np.array_equal(before, base.λ)
    rng = ref.ScriptedRng(ref.LOCK_SEED_DISC)
    Y0 = np.log(base.λ) - base.m
    new = base.resample_(ds, rng)
    res, bound = ref.serial_update(case, rng.record, "cols")
    cond = ref.lockstep_conditions(res, bound)
    print("discrete lock step:", cond)
    assert cond["clear"] and cond["first"] and cond["long"] and cond["both"], cond
    assert len(rng.record) == 2 + max(cond["rounds"])
    want = np.exp(case["m"] + np.column_stack([r.y for r in res]))
    np.testing.assert_allclose(new, want, rtol=1e-14, atol=0.0)
    theta, rounds = replay_lock_step(lambda Y: base.candidate_loglikelihood(ds, Y), Y0, np.linalg.cholesky(case["Sigma"]), rng.record, "cols")
    assert np.array_equal(theta, [r.theta for r in res]) and np.array_equal(rounds, cond["rounds"])


# -------------------------------------------------------------------------------------------------- invariance on the GPU
SIGMA2 = np.array([[1.0, 0.6], [0.6, 1.0]])
M2 = float(np.log(1.5))


def test_continuous_update_leaves_the_posterior_invariant(nhp):
    """256 nodes on the grid [0, 4]: 128 without baseline events, 128 that share the event times 0.5, 1.0, 3.5; one lock-step
    update per sweep through resample_, every node one replica of its group's chain."""
    N, X, events = 256, 4.0, (0.5, 1.0, 3.5)
    times = np.repeat(events, 128)
    nodes = np.tile(np.arange(129, 257, dtype=np.int64), 3)
    rng = np.random.default_rng(41)
    Y = rng.standard_normal((N, 2)) @ np.linalg.cholesky(SIGMA2).T
    base = nhp.LogGaussianCoxProcess(np.array([0.0, X]), list(np.exp(M2 + Y)), SIGMA2.copy(), M2)
    ds = nhp.continuous.DeviceDataset(nhp.default_context(), (times, nodes, X), N, 1.0)
    base.candidate_loglikelihood(ds, Y, parentnodes=np.zeros(len(times), dtype=np.int64))      # every event a baseline event

    def sweep(_):
        base.resample_(ds, rng)
        return np.log(np.vstack(base.λ)) - M2

    groups = {"no events": (slice(0, 128), ref.two_point_cont_loglik(X, M2, ())),
              "three events": (slice(128, 256), ref.two_point_cont_loglik(X, M2, events))}
    _invariance(sweep, Y, groups, "continuous")


def _invariance(sweep, Y, groups, what):
    """ref.invariance_pvalues for several groups of replicas that one sweep advances together."""
    from scipy import stats
    kept = []
    for s in range(ref.BURN + ref.KEPT_SWEEPS):
        Y = sweep(Y)
        if s >= ref.BURN and (s - ref.BURN) % ref.THIN == ref.THIN - 1:
            kept.append(Y.copy())
    assert len(kept) == ref.KEPT_SWEEPS // ref.THIN
    for name, (rows, ll) in groups.items():
        cdfs = ref.posterior_cdfs(ll, SIGMA2)
        K = np.concatenate([k[rows] for k in kept])
        p = tuple(float(stats.kstest(cdfs[k](K[:, k]), "uniform").pvalue) for k in (0, 1))
        print(f"invariance, {what}, {name}: {len(K)} draws, KS p-values {p[0]:.3g}, {p[1]:.3g}")
        assert min(p) > ref.P_MIN, (what, name, p)


def test_discrete_update_leaves_the_posterior_invariant(nhp):
    """128 identical rows of T = 8 bins on the grid [0, 8], W = 0."""
    N, T, counts = 128, 8, (3, 0, 1, 2, 0, 4, 1, 2)
    data = np.tile(np.array(counts, dtype=np.int64), (N, 1))
    rng = np.random.default_rng(42)
    Y = (rng.standard_normal((N, 2)) @ np.linalg.cholesky(SIGMA2).T)
    d = dict(N=N, grid_x=np.array([0.0, float(T)]), lam=np.exp(M2 + Y.T), m=M2, dt=1.0)
    proc = disc_process(nhp, d, np.zeros((N, N)))
    proc.baseline.Σ = SIGMA2.copy()
    base = proc.baseline
    ds = nhp.convolve(proc, data)
    nhp.resample_parent_counts(proc, convolved=ds, seed=1, step=0)

    def sweep(_):
        return (np.log(base.resample_(ds, rng)) - M2).T

    _invariance(sweep, Y, {"eight bins": (slice(0, N), ref.two_point_disc_loglik(float(T), M2, counts, 1.0))}, "discrete")


# ---------------------------------------------------------------------------------------------------------- one mcmc_ step
def test_one_mcmc_step_is_parents_baseline_weights_impulses(nhp, orc):
    """mcmc_ with an LGCP baseline against the composition inference.py documents, by hand on a copy with the same seed: an
    update that read the attribution of an earlier sweep (or none) would give another curve."""
    case = ref.lockstep_cont_case()
    N = case["N"]

    def process():
        base = nhp.LogGaussianCoxProcess(case["grid_x"].copy(), [r.copy() for r in case["lam"]], case["Sigma"].copy(), case["m"])
        return nhp.ContinuousStandardHawkesProcess(base, nhp.ExponentialImpulseResponse(np.full((N, N), 2.0), 1.0, 1.0, case["dt_max"]),
                                                   nhp.DenseWeightModel(np.full((N, N), 0.05)))

    data = (case["times"], case["nodes"], case["T"])
    seed = 6
    a = process()
    ds = nhp.continuous.DeviceDataset(nhp.default_context(), data, N, case["dt_max"])
    nhp.resample_parents(a, ds, seed=99, step=7)                           # a stale attribution for the step to replace
    res = nhp.mcmc_(a, ds, nsteps=1, seed=seed)
    b = process()
    ds2 = nhp.continuous.DeviceDataset(nhp.default_context(), data, N, case["dt_max"])
    rng = np.random.default_rng(seed)
    _, pn, st = nhp.resample_parents(b, ds2, seed=seed, step=0, with_stats=True)
    assert 0.05 < np.mean(pn == 0) < 0.95
    b.baseline.resample_(ds2, rng, parentnodes=pn)
    b.weights.resample_(st["Mn"], st["Mnm"], rng)
    b.impulses.resample_(st["Mnm"], st["Xnm"], rng)
    assert np.array_equal(res.samples[0], b.params()) and np.array_equal(a.params(), b.params())
