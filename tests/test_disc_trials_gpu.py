"""Independent trials on the GPU (nhp_disc_dataset_set_trials): the convolution stops at every trial's first bin, bit for bit
the trials convolved alone, on both kernels; and every consumer of Ŝ, given a list of trials, computes what its reference
computes from the stacked counts and the stacked per-trial Ŝ (tests/disc_trials_ref.py), to the tolerance the existing test
of the same quantity holds it to.  tests/test_disc_trials_host.py shows that each convolution case can see a leak."""
import copy
import math

import numpy as np
import pytest

import disc_grad_ref as gr
import disc_information_ref as ir
import disc_residuals_ref as rr
import disc_score_ref as sc
import disc_svi_ref as sr
import disc_trials_ref as tr

pytestmark = pytest.mark.gpu

ROUTES = ("by rule", "dense")


def route(monkeypatch, which):
    if which == "dense":
        monkeypatch.setenv("NHP_CONV_DENSE", "1")
    else:
        monkeypatch.delenv("NHP_CONV_DENSE", raising=False)


# ---- the convolution ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ROUTES)
@pytest.mark.parametrize("name", list(tr.CONV_CASES))
def test_convolution_equals_the_trials_convolved_alone(nhp, orc, monkeypatch, name, which):
    """Ŝ bit for bit, from a list, a tuple and a dataset cut by offsets; Σ_t Ŝ within the rounding of two orders of
    summation (2(T − 1)·2⁻⁵³ relative: the terms are non-negative), and bit for bit with a basis whose sums are exact."""
    from nhp_amd import _lib
    route(monkeypatch, which)
    N, lengths, B, L, *_ = tr.CONV_CASES[name]
    proc, trials = tr.conv_case(nhp, name)
    stacked, off = tr.stack(trials)
    T = stacked.shape[1]
    phi = proc.impulses.basis()
    want = tr.convolve(orc, trials, phi)
    ds, conv = nhp.convolve(proc, trials, fetch=True)
    assert conv.shape == (T, N, B) and ds.ntrials == len(trials) and np.array_equal(ds.trial_offsets, off)
    assert [ds.trial_bins(r) for r in range(len(trials))] == list(zip(off[:-1].tolist(), off[1:].tolist()))
    assert ds.trial_bins(-1) == (int(off[-2]), T)
    assert np.array_equal(conv, want)
    _, conv_t = nhp.convolve(proc, tuple(trials), fetch=True)
    assert np.array_equal(conv_t, want)
    cut = nhp.DiscreteDataset(nhp.default_context(), stacked, trial_offsets=off)
    _, conv_c = nhp.convolve(proc, cut, fetch=True)
    assert np.array_equal(conv_c, want)
    got_sum, want_sum = ds.convsum(), tr.convsum(want)
    assert got_sum.shape == (N, B)
    assert np.all(np.abs(got_sum - want_sum) <= 2.0 * (T - 1) * 2.0 ** -53 * want_sum)
    sparse = which != "dense" and L <= 64 and np.count_nonzero(stacked) < 0.125 * stacked.size      # nhp_disc_convolve's rule
    assert np.array_equal(got_sum, tr.convsum_device_order(want, sparse))        # the kernels' own order of summation
    assert np.array_equal(cut.convsum(), got_sum)                                # the same bits from another run
    if len(trials) == 1:                                   # R = 1: the plain dataset's bits, Ŝ and column sums
        plain, conv_p = nhp.convolve(proc, stacked, fetch=True)
        assert np.array_equal(conv, conv_p) and np.array_equal(conv, orc.disc_convolve(stacked, phi))
        assert np.array_equal(got_sum, plain.convsum())
    # exact sums: every order of summation gives the same bits
    dy = tr.dyadic_basis(L, B)
    out = np.empty(T * N * B)
    ctx = nhp.default_context()
    _lib.check(_lib.lib().nhp_disc_convolve(ctx.h, cut.h, _lib.dptr(np.asfortranarray(dy).ravel(order="K")), L, B, _lib.dptr(out)), ctx.h)
    cut.B = B
    want_dy = tr.convolve(orc, trials, dy)
    assert np.array_equal(out.reshape((T, N, B), order="F"), want_dy)
    assert np.array_equal(cut.convsum(), want_dy.sum(axis=0))


def test_set_trials_drops_the_convolution_and_checks_its_offsets(nhp, orc):
    proc, trials = tr.conv_case(nhp, "pair_straddles")
    stacked, off = tr.stack(trials)
    T = stacked.shape[1]
    phi = proc.impulses.basis()
    ds, conv = nhp.convolve(proc, stacked, fetch=True)                 # one recording: the naive concatenation
    assert ds.ntrials == 1 and np.array_equal(conv, tr.convolve_naive(orc, trials, phi))
    ds.set_trials(off)
    assert ds.B == 0 and ds.ntrials == len(trials)
    with pytest.raises(Exception, match="convolve"):                   # Ŝ is gone
        nhp.discrete.disc_intensity(proc, convolved=ds)
    with pytest.raises(Exception, match="convolve"):
        ds.convsum()
    _, conv = nhp.convolve(proc, ds, fetch=True)
    assert np.array_equal(conv, tr.convolve(orc, trials, phi))
    for bad, entry in (([1, T], r"offsets\[0\]"), ([0, 5, 5, T], r"offsets\[2\]"), ([0, 7, 3, T], r"offsets\[2\]"),
                       ([0, 5, T - 1], r"offsets\[2\]"), ([0, T + 1], r"offsets\[1\]"), ([0, 0, T], r"offsets\[1\]")):
        with pytest.raises(nhp.NhpError, match="status 1.*" + entry):  # NHP_EINVAL, naming the entry
            ds.set_trials(bad)
        assert np.array_equal(ds.trial_offsets, off) and ds.B == proc.impulses.nbasis()      # a refused call changes nothing
    with pytest.raises(Exception):
        nhp.DiscreteDataset(nhp.default_context(), stacked, trial_offsets=[0, 3, 3, T])
    with pytest.raises(ValueError):
        nhp.DiscreteDataset(nhp.default_context(), trials, trial_offsets=off)
    ds.set_trials([0, T])                                              # R = 1: as if never cut
    assert ds.ntrials == 1 and ds.B == 0
    _, conv = nhp.convolve(proc, ds, fetch=True)
    assert np.array_equal(conv, orc.disc_convolve(stacked, phi))


def lgcp_like(nhp, proc, T):
    x = np.linspace(0.0, float(T), 5)
    base = nhp.DiscreteLogGaussianCoxProcess(x, np.full((5, proc.ndims()), 0.3), None, -1.0, proc.dt)
    return nhp.DiscreteStandardHawkesProcess(base, proc.impulses, proc.weights, proc.dt)


def test_the_library_refuses_what_convolves_across_time(nhp):
    """The guards of the C entry points, reached past the package's own: an LGCP baseline and the streamed SVI window."""
    proc, trials = tr.conv_case(nhp, "word_edges")
    stacked, off = tr.stack(trials)
    T = stacked.shape[1]
    ds = nhp.convolve(proc, trials)
    with pytest.raises(NotImplementedError, match="trials"):
        lgcp_like(nhp, proc, T).baseline.attach(ds)
    for call in (lambda d: nhp.svi_(proc, d, nsteps=1, batch_bins=64, streamed=True),
                 lambda d: nhp.loglikelihood(lgcp_like(nhp, proc, T), d), lambda d: nhp.disc_forecast(proc, d, 4, nsamples=2)):
        with pytest.raises(NotImplementedError, match="trial"):
            call(trials)
    with pytest.raises(NotImplementedError, match="trials"):
        nhp.svi_(proc, ds, nsteps=1, batch_bins=64, streamed=True)
    ds.trial_offsets = np.array([0, T], dtype=np.int64)                # the package now takes it for one recording; the library knows
    with pytest.raises(NotImplementedError, match="trials"):
        nhp.svi_(proc, ds, nsteps=1, batch_bins=64, streamed=True)
    import disc_netvb_ref as nr
    import disc_sbmvb_ref as br
    n = proc.ndims()
    Bn, Ln = proc.impulses.nbasis(), proc.nlags()
    netproc = nr.put(nr.make_process(nhp, n, Bn, Ln, nr.PARITY_PRIORS, nr.PARITY_NET, seed=n), nr.random_start(n, Bn))
    blkproc = br.put(br.make_process(nhp, n, Bn, Ln, 2), nr.random_start(n, Bn), br.random_blocks(n, 2))
    for p in (netproc, blkproc):                                       # nhp_disc_netsvi_run, nhp_disc_sbmsvi_run
        with pytest.raises(NotImplementedError, match="trials"):
            nhp.svi_(p, ds, nsteps=1, batch_bins=64, streamed=True)
    plain = nhp.DiscreteDataset(nhp.default_context(), stacked)
    lgcp_like(nhp, proc, T).baseline.attach(plain)
    with pytest.raises(NotImplementedError, match="LGCP"):
        plain.set_trials(off)


# ---- the consumers --------------------------------------------------------------------------------------------------------------
LENGTHS = [37, 64, 129, 50]
N, B, L = 4, 3, 6
_shared = {}


def shared(nhp, orc, network=False):
    """One trial dataset for all the consumers, its stacked counts and its reference Ŝ, computed once and left unchanged."""
    if network not in _shared:
        proc, trials, lam0, W, th, A = tr.make_trials(nhp, N, LENGTHS, B, L, seed=5, rate=0.1, network=network)
        stacked, off = tr.stack(trials)
        conv = tr.convolve(orc, trials, orc.disc_basis(L, B, 1.0))
        for a in (stacked, off, conv, lam0, W, th, *trials):
            a.setflags(write=False)
        _shared[network] = dict(proc=proc, trials=trials, stacked=stacked, off=off, conv=conv, lam0=lam0, W=W, th=th, A=A)
    c = dict(_shared[network])
    c["proc"] = copy.deepcopy(c["proc"])
    return c


@pytest.mark.parametrize("network", [False, True])
def test_intensity_and_loglikelihood(nhp, orc, network):
    c = shared(nhp, orc, network)
    proc, trials = c["proc"], c["trials"]
    want = orc.disc_intensity(c["conv"], c["lam0"], c["W"], c["th"], dt=1.0, A=c["A"])
    got = nhp.intensity(proc, trials)
    assert got.shape == (sum(LENGTHS), N)
    assert np.max(np.abs(got - want) / want) < 1e-12
    naive = orc.disc_intensity(tr.convolve_naive(orc, trials, orc.disc_basis(L, B, 1.0)), c["lam0"], c["W"], c["th"], dt=1.0, A=c["A"])
    assert np.max(np.abs(got - naive) / naive) > 1e-6                  # not the concatenation's intensity
    wll = orc.disc_loglik(c["stacked"], want)
    ll = nhp.loglikelihood(proc, trials)
    ds = nhp.convolve(proc, trials)
    assert abs(ll - wll) < 1e-11 * abs(wll) and ll == nhp.loglikelihood(proc, trials, convolved=ds) == nhp.loglikelihood(proc, ds)
    alone = sum(nhp.loglikelihood(proc, x) for x in trials)            # the unchanged single-trial route, trial by trial
    assert abs(ll - alone) < 1e-11 * abs(alone)


def test_gradient(nhp, orc):
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    r = tr.grad_reference(trials, proc.impulses.basis(), c["W"], c["th"], 1.0, c["lam0"])
    assert np.allclose(np.asarray(r.conv, dtype=np.float64), c["conv"], rtol=1e-14, atol=0.0)      # the reference's own Ŝ, trial by trial
    ll, g = nhp.loglikelihood_gradient(proc, trials)
    T = sum(LENGTHS)
    bound = gr.gradient_bound(N, T, B, r.scale)
    err = np.abs(g - r.grad)
    print(f"gradient error / bound {float(np.max(err / bound)):.3g}; ll rel {abs(ll - float(r.ll)) / abs(float(r.ll)):.3g}")
    assert abs(ll - float(r.ll)) < 1e-11 * abs(float(r.ll))
    assert g.shape == r.grad.shape and np.all(err <= bound)


def test_vb_step(nhp, orc):
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    rng = np.random.default_rng(5)
    proc.baseline.αv, proc.baseline.βv = rng.uniform(0.5, 3, N), rng.uniform(0.5, 3, N)
    proc.weights.κv, proc.weights.νv = rng.uniform(0.5, 3, (N, N)), rng.uniform(0.5, 3, (N, N))
    proc.impulses.γv = rng.uniform(0.5, 3, (N, N, B))
    want = orc.disc_vb_step(c["stacked"], c["conv"], 1.0, proc.baseline.α0, proc.baseline.β0, proc.weights.κ, proc.weights.ν,
                            proc.impulses.γ, proc.baseline.αv, proc.baseline.βv, proc.weights.κv, proc.weights.νv, proc.impulses.γv)
    nhp.update_(proc, trials, None)
    for g, w in zip((proc.baseline.αv, proc.baseline.βv, proc.weights.κv, proc.weights.νv, proc.impulses.γv), want):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)
    p2 = shared(nhp, orc)["proc"]
    res = nhp.vb_(p2, trials, max_steps=3)
    assert res.step == 3 and np.all(p2.weights.νv == 1.0 + c["stacked"].sum(axis=1)[:, None])
    assert np.all(p2.baseline.βv == 1.0 + sum(LENGTHS) * 1.0)          # the exposure: all stacked bins


def test_parent_counts(nhp, orc):
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    want = orc.disc_resample_parents(c["stacked"], c["conv"], c["lam0"], c["W"], c["th"], 1.0, seed=11, step=4)
    got = nhp.resample_parent_counts(proc, trials, seed=11, step=4)
    assert got.shape == (N, 1 + N * B) and np.array_equal(got.sum(axis=1), c["stacked"].sum(axis=1))
    assert np.array_equal(got, want)


def test_adjacency_sweep(nhp, orc):
    c = shared(nhp, orc, network=True)
    proc, trials = c["proc"], c["trials"]
    proc.weights.W = c["W"] * N * 1.5                                  # links that matter
    u = np.random.default_rng(7).uniform(size=(N, N))
    A0 = proc.adjacency_matrix.copy()
    want = orc.disc_resample_adjacency(c["stacked"], c["conv"], c["lam0"], proc.weights.W, c["th"], A0, proc.network.ρ, u, 1.0)
    links = nhp.disc_resample_adjacency_matrix_(proc, trials, u=u)
    assert np.array_equal(proc.adjacency_matrix, want) and links == want.sum()
    assert not np.array_equal(want, A0)


@pytest.mark.parametrize("kind", ir.KINDS)
def test_information_blocks(nhp, orc, kind):
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    res = tr.information_reference(trials, proc.impulses.basis(), c["W"], c["th"], 1.0, c["lam0"], kind)
    info = nhp.disc_observed_information(proc, trials, kind=kind)
    J = np.asarray(info.blocks)
    ratio, bad = ir.check_blocks(J, res, N, B)
    print(f"[{kind}] blocks error / bound {ratio:.3g}")
    assert J.shape == (N, 1 + N * B, 1 + N * B) and len(bad) == 0
    assert info.ll == nhp.loglikelihood(proc, trials)
    se = nhp.disc_standard_errors(proc, trials, kind=kind)
    assert se.se.shape == (N + N * N * B,)
    v = np.random.default_rng(3).standard_normal(N + N * N * B)
    hv = nhp.disc_hessian_vector_product(proc, trials, v=v, kind=kind)
    # J·v against blocks[c] @ v_c: two fp64 evaluations of one sum, each inside its bound of disc_information_ref
    # ((3·N·B + n_t + 64) and (2·N·B + n_t + 48) roundings, n_t <= ΣT_r) of Σ|J||v|
    for col in range(N):
        idx = ir.block_index(N, B, col)
        S_hv = np.abs(J[col]) @ np.abs(v[idx])
        assert np.all(np.abs(hv[idx] - J[col] @ v[idx]) <= (5 * N * B + 2 * sum(LENGTHS) + 112) * 2.0 ** -53 * S_hv), col


def test_residuals(nhp, orc):
    c = shared(nhp, orc)
    proc, trials, counts = c["proc"], c["trials"], c["stacked"]
    T = counts.shape[1]
    lam = nhp.intensity(proc, trials)
    ref = rr.residuals(counts, lam, 9, 20)
    got = nhp.disc_residuals(proc, trials, seed=9, nbins=20, pit=True, pearson=True, cumulative=True)
    assert got.pit.shape == got.pearson.shape == got.cumulative.shape == (N, T) and got.bins == T
    fin = np.isfinite(ref["pearson"])
    e_pit = np.abs(got.pit - ref["pit"]).max()
    e_pe = (np.abs(got.pearson[fin] - ref["pearson"][fin]) / np.maximum(np.abs(ref["pearson"][fin]), 1e-300)).max()
    e_cum = (np.abs(got.cumulative - ref["cumulative"]).max(axis=1) / np.maximum(ref["expected"], 1e-300)).max()
    print(f"max |pit - ref| = {e_pit:.3g}, max rel pearson = {e_pe:.3g}, max rel cumulative = {e_cum:.3g}")
    assert e_pit <= 1e-12 and e_pe <= 1e-12 and e_cum <= 1e-12       # the compensator runs on over the stacked bins
    for k in ("expected", "chi2", "deviance"):
        assert np.all(np.abs(getattr(got, k) - ref[k]) <= 1e-12 * np.abs(ref[k])), k
    assert np.array_equal(got.observed, ref["observed"]) and np.array_equal(got.histogram, ref["histogram"])
    fit = nhp.disc_goodness_of_fit(proc, trials, seed=9)
    assert 0.0 <= fit.pvalue <= 1.0 and fit.impossible == ref["impossible"]


def test_a_scored_draw(nhp, orc):
    """disc_score_samples on the last trial's bins of the trial list against the 50-digit reference of that trial alone (its
    rows of Ŝ are the trial's own), within disc_score_ref.tolerances."""
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    rng = np.random.default_rng(17)
    xs, draws = [], []
    for _ in range(3):
        l0 = rng.uniform(0.05, 0.4, N)
        eta = (rng.uniform(0.0, 0.8, (N, N)) / N)[:, :, None] * rng.dirichlet(np.ones(B), (N, N))
        xs.append(np.concatenate([l0, eta.ravel(order="F")]))
        draws.append((l0, np.ones((N, N)), eta, None))
    ds = nhp.convolve(proc, trials)
    bins = ds.trial_bins(-1)
    assert bins == (sum(LENGTHS[:-1]), sum(LENGTHS))
    s = nhp.disc_score_samples(proc, xs, trials, bins=bins, pointwise=True)
    assert s.n == 3 and s.cells == LENGTHS[-1] * N and s.bins == bins
    case = dict(data=np.array(trials[-1]), phi=proc.impulses.basis(), dt=1.0, bins=(0, LENGTHS[-1]), draws=draws)
    mpr = sc.score_mp(case)[3]
    got = dict(summary={k: getattr(s, k) for k in sc.FIELDS}, per_node=s.per_node, pointwise=s.pointwise)
    yard = sc.errors(sc.score_numpy(case), mpr)
    err, tol = sc.errors(got, mpr), sc.tolerances(yard, mpr)
    for k in err:
        print(f"{k}: device {err[k]:.3e}  numpy {yard[k]:.3e}")
        if np.ndim(tol[k]) == 0 and math.isnan(tol[k]):
            assert math.isnan(err[k]), k
        elif k == "pointwise":
            assert np.all(sc.pointwise_errors(got, mpr) <= tol[k])
        else:
            assert err[k] <= tol[k], (k, err[k], tol[k])
    same_score(nhp.disc_score_samples(proc, xs, ds, bins=bins, pointwise=True), s)


def same_score(a, b):
    for k in sc.FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), (k, getattr(a, k), getattr(b, k))
    assert np.array_equal(a.per_node, b.per_node, equal_nan=True) and a.bins == b.bins
    assert (a.pointwise is None) == (b.pointwise is None)
    if a.pointwise is not None:
        assert np.array_equal(a.pointwise, b.pointwise, equal_nan=True)


# ---- the fits ---------------------------------------------------------------------------------------------------------------------
def test_device_mle_on_trials(nhp):
    rng = np.random.default_rng(3)
    Nm, Bm, Lm, R, Tr = 2, 2, 4, 8, 1000
    true = np.array([0.2, 0.6])
    trials = [rng.poisson(true[:, None] * np.ones((Nm, Tr))).astype(np.int64) for _ in range(R)]

    def fresh():
        return nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.ones(Nm), 1.0),
                                                 nhp.DiscreteGaussianImpulseResponse(np.full((Nm, Nm, Bm), 1.0 / Bm), Lm, 1.0),
                                                 nhp.DenseWeightModel(np.full((Nm, Nm), 0.1)), 1.0)
    x0 = np.concatenate([np.full(Nm, 0.5), np.full(Nm * Nm * Bm, 0.03)])
    p0 = fresh()
    nhp.discrete.disc_params_(p0, x0)
    ll0 = nhp.loglikelihood(p0, trials)
    proc = fresh()
    res = nhp.mle_(proc, trials, guess=x0, optimizer="device", f_abstol=1e-9)
    assert res.status == "success"
    x = res.maximizer
    ll, g = nhp.loglikelihood_gradient(proc, trials)
    assert abs(nhp.loglikelihood(proc, trials) - res.maximum) < 1e-9 * abs(res.maximum) and abs(ll - res.maximum) < 1e-9 * abs(ll)
    assert res.maximum >= ll0
    pg = np.where(((x <= 1e-6) & (g < 0)) | ((x >= 10.0) & (g > 0)), 0.0, g)
    print(f"start {ll0:.6f} -> maximum {res.maximum:.6f}; projected gradient {np.max(np.abs(pg)):.3g} (bound {5e-2 * abs(ll) ** 0.5:.3g})")
    assert np.max(np.abs(pg)) < 5e-2 * abs(ll) ** 0.5
    host = fresh()
    hres = nhp.mle_(host, trials, guess=x0, f_abstol=1e-9)              # the host optimizer takes the list as well
    assert abs(hres.maximum - nhp.loglikelihood(host, trials)) < 1e-9 * abs(hres.maximum)
    assert res.maximum >= hres.maximum - 1e-3 * abs(hres.maximum) ** 0.5


def test_chain_routes_agree_on_trials(nhp, orc):
    """The resident routes reproduce the default route's chain on a trial list, sample for sample and bit for bit; the
    held-out score of the last trial and the WAIC of the others are those of disc_score_samples on the same samples."""
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    default, stepwise, resident = copy.deepcopy(proc), copy.deepcopy(proc), copy.deepcopy(proc)
    want = nhp.mcmc_(default, trials, nsteps=6, seed=4)
    got = nhp.mcmc_(stepwise, trials, nsteps=6, seed=4, keep_samples=True, moments=True)
    assert got.steps == 6 and len(got.samples) == 6
    for k in range(6):
        assert np.array_equal(got.samples[k], want.samples[k]), k
    assert not np.array_equal(want.samples[0], want.samples[5])
    last = nhp.mcmc_(resident, trials, nsteps=6, seed=4, keep_samples=False)
    assert np.array_equal(last.samples[0], want.samples[5])
    for p in (stepwise, resident):
        assert np.array_equal(p.baseline.λ, default.baseline.λ) and np.array_equal(p.weights.W, default.weights.W)
        assert np.array_equal(p.impulses.θ, default.impulses.θ)
    # not the chain of the concatenation
    naive = nhp.mcmc_(copy.deepcopy(proc), c["stacked"], nsteps=6, seed=4)
    assert not np.array_equal(naive.samples[5], want.samples[5])
    # scoring: fit on all trials but the last, hold out the last
    fit, R = trials[:-1], len(trials)
    bins = nhp.convolve(proc, trials).trial_bins(R - 1)
    kw = dict(nsteps=8, burn=2, seed=6, waic=True, heldout=(trials, bins), pointwise=True)
    runs = [nhp.mcmc_(copy.deepcopy(proc), fit, **kw), nhp.mcmc_(copy.deepcopy(proc), fit, keep_samples=True, moments=True, **kw)]
    one = nhp.mcmc_(copy.deepcopy(proc), fit, keep_samples=False, **kw)
    for res in runs:
        assert res.heldout.n == 6 and res.heldout.bins == bins and res.waic.bins == (0, sum(LENGTHS[:-1]))
        same_score(nhp.disc_score_samples(proc, res.samples, trials, bins=bins, burn=2, pointwise=True), res.heldout)
        same_score(nhp.disc_score_samples(proc, res.samples, fit, burn=2, pointwise=True), res.waic)
        same_score(res.heldout, one.heldout)
        same_score(res.waic, one.waic)


def split_network_sample(x, n, b):
    nn = n * n
    rho, l0, W, th, A = np.split(x, [1, 1 + n, 1 + n + nn, 1 + n + nn + nn * b])
    return float(rho[0]), l0, W.reshape((n, n), order="F"), th.reshape((n, n, b), order="F"), A.reshape((n, n), order="F")


def test_network_chain_on_trials(nhp, orc):
    """tests/test_disc_chain_gpu.py's test_chain_identity_network_process on a trial list: five resident steps; step k replayed
    on the host from sample k − 1 (with its ρ) through nhp_disc_gibbs_step and the adjacency sweep's own entry on a trial
    dataset: λ0, W, θ, A equal bit for bit; ρ_k the bits nhp_cont_network_rho leaves for (α, β, ΣA_k, N², seed, k).  The
    chain that keeps no samples ends in the same state, and none of it is the concatenation's chain."""
    from helpers import random_case
    from nhp_amd import _lib
    seed = 9
    c = shared(nhp, orc, network=True)
    proc, trials = c["proc"], c["trials"]
    proc.weights.W = c["W"] * N * 1.5                                  # links that matter
    host, resident, naive = copy.deepcopy(proc), copy.deepcopy(proc), copy.deepcopy(proc)
    start = (proc.network.ρ, proc.baseline.λ.copy(), proc.weights.W.copy(), proc.impulses.θ.copy(), proc.adjacency_matrix.copy())
    res = nhp.mcmc_(proc, trials, nsteps=5, seed=seed, keep_samples=True, moments=True)
    assert len(res.samples) == 5
    ctx = nhp.default_context()
    ds = nhp.convolve(host, trials)
    assert ds.ntrials == len(trials)
    lib = _lib.lib()
    cm = random_case(N, 50, 10.0, "exponential", 1.0, network=True, seed=1, nhp=nhp)["proc"].device_model(ctx)   # for the ρ draw
    prev, flipped = start, 0
    b, w, imp = host.baseline, host.weights, host.impulses
    for k in range(5):
        rho, l0, W, th, A = prev
        host.network.ρ, host.adjacency_matrix = rho, A.copy()
        fl0, fW, fth, fA = _lib.f64(l0).copy(), _lib.colmajor(W).copy(), _lib.colmajor(th).copy(), _lib.colmajor(A).copy()
        _lib.check(lib.nhp_disc_gibbs_step(ctx.h, ds.h, _lib.dptr(fl0), _lib.dptr(fW), _lib.dptr(fth), _lib.dptr(fA), host.dt,
                                           b.α0, b.β0, w.κ, w.ν, imp.γ, seed, k), ctx.h)
        b.λ, w.W, imp.θ = fl0, fW.reshape((N, N), order="F"), fth.reshape((N, N, B), order="F")
        links = nhp.disc_resample_adjacency_matrix_(host, convolved=ds, seed=seed, step=k, ctx=ctx)
        got = split_network_sample(res.samples[k], N, B)
        assert np.array_equal(got[1], b.λ), k
        assert np.array_equal(got[2], w.W), k
        assert np.array_equal(got[3], imp.θ), k
        assert np.array_equal(got[4], host.adjacency_matrix), k
        assert links == got[4].sum()
        flipped += not np.array_equal(got[4], A)
        _lib.check(lib.nhp_cont_model_set_rho(ctx.h, cm.h, 0.5), ctx.h)
        _lib.check(lib.nhp_cont_network_rho(ctx.h, cm.h, host.network.α, host.network.β, float(links), float(N * N), seed, k), ctx.h)
        r3 = np.empty(3)
        _lib.check(lib.nhp_cont_model_get_rho(ctx.h, cm.h, _lib.dptr(r3)), ctx.h)
        assert got[0] == r3[0], (k, got[0], r3[0])
        prev = got
    assert flipped >= 1, "vacuous: A never changed"
    assert proc.network.ρ == prev[0] and np.array_equal(proc.adjacency_matrix, prev[4])
    last = nhp.mcmc_(resident, trials, nsteps=5, seed=seed, keep_samples=False)
    assert np.array_equal(last.samples[0], res.samples[4]) and np.array_equal(resident.adjacency_matrix, proc.adjacency_matrix)
    other = nhp.mcmc_(naive, c["stacked"], nsteps=5, seed=seed, keep_samples=True, moments=True)
    assert not np.array_equal(other.samples[4], res.samples[4])
    rd = nhp.mcmc_(copy.deepcopy(host), trials, nsteps=3, seed=seed)   # the default route takes the list as well
    assert rd.steps == 3 and np.all(np.isfinite(rd.samples[2]))


def test_resident_svi_on_trials(nhp, orc):
    c = shared(nhp, orc)
    proc, trials = c["proc"], c["trials"]
    priors = (1.0, 1.0, 1.0, 1.0, 1.0)
    T, Tb = sum(LENGTHS), 64
    nb = sr.n_blocks(T, Tb)
    blocks = np.array([0, nb - 1, 1, nb - 1, 0, 0], dtype=np.int32)
    rng = np.random.default_rng(5)
    start = (rng.uniform(0.5, 3, N), rng.uniform(0.5, 3, N), rng.uniform(0.5, 3, (N, N)), rng.uniform(0.5, 3, (N, N)),
             rng.uniform(0.5, 3, (N, N, B)))

    def put(p):
        p.baseline.αv, p.baseline.βv, p.weights.κv, p.weights.νv, p.impulses.γv = (np.array(x) for x in start)

    def get(p):
        return p.baseline.αv, p.baseline.βv, p.weights.κv, p.weights.νv, p.impulses.γv
    want1 = sr.svi_run(orc, c["stacked"], c["conv"], 1.0, priors, start, blocks[:1], Tb, 1.0, 0.6)
    want6 = sr.svi_run(orc, c["stacked"], c["conv"], 1.0, priors, want1, blocks[1:], Tb, 1.0, 0.6, step0=1)
    put(proc)
    res = nhp.svi_(proc, trials, nsteps=1, batch_bins=Tb, delay=1.0, forgetting=0.6, blocks=blocks[:1])
    for g, w in zip(get(proc), want1):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)
    assert res.step == 1
    put(proc)
    nhp.svi_(proc, nhp.convolve(proc, trials), nsteps=6, batch_bins=Tb, delay=1.0, forgetting=0.6, blocks=blocks)
    for g, w in zip(get(proc), want6):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)


def test_network_vb_step_on_trials(nhp, orc):
    """update_ on a network process with spike-and-slab weights: the seven tables of one step against
    disc_netvb_ref.netvb_step fed the stacked counts and the stacked per-trial Ŝ, at tests/test_disc_netvb_gpu.py's bound."""
    import disc_netvb_ref as nr
    c = shared(nhp, orc)
    proc = nr.make_process(nhp, N, B, L, nr.PARITY_PRIORS, nr.PARITY_NET, seed=N)
    start = nr.random_start(N, B)
    want = nr.netvb_step(np.array(c["stacked"]), np.array(c["conv"]), 1.0, nr.PARITY_PRIORS, nr.PARITY_NET, start)
    nr.put(proc, start)
    nhp.update_(proc, c["trials"], None)
    got = nr.get(proc)
    for g, w in zip(got[:7], want[:7]):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)
    naive = nr.netvb_step(np.array(c["stacked"]), tr.convolve_naive(orc, c["trials"], orc.disc_basis(L, B, 1.0)), 1.0, nr.PARITY_PRIORS,
                          nr.PARITY_NET, start)
    assert not np.allclose(got[6], naive[6], rtol=1e-6, atol=0.0)          # γv of the concatenation is another answer
