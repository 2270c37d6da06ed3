"""Streaming quantiles on the GPU (nhp_cont_model_quantiles_*, nhp_disc_model_quantiles_*, csrc/chain_quantiles.hip) against
the numpy restatement of their definition (tests/chain_quantiles_ref.py), bit for bit: a scripted chain of arbitrary doubles,
the grid-stride loop, real chains on every route, the discrete resident chain, and the state's life cycle and refusals.
Only correctly rounded operations are involved, so every comparison is np.array_equal."""
import copy
import ctypes as C

import numpy as np
import pytest

import chain_quantiles_ref as ref
from helpers import random_case

pytestmark = pytest.mark.gpu

PROBS = {1: (0.5,), 3: (0.025, 0.5, 0.975), 4: (0.05, 0.25, 0.75, 0.95)}


def configure(ctx, model, probs, every=1, effective=False, disc=False):
    from nhp_amd import _lib
    fn = _lib.lib().nhp_disc_model_quantiles_configure if disc else _lib.lib().nhp_cont_model_quantiles_configure
    p = None if probs is None else _lib.f64(probs)
    _lib.check(fn(ctx.h, model.h, _lib.dptr(p), 0 if probs is None else len(probs), every, int(effective)), ctx.h)


def fetch(ctx, model, L, m, disc=False, extremes=True):
    from nhp_amd import _lib
    fn = _lib.lib().nhp_disc_model_quantiles_fetch if disc else _lib.lib().nhp_cont_model_quantiles_fetch
    values, rho, cnt = np.empty((m, L)), np.empty(m + 2), C.c_int64()
    lo, hi = (np.empty(L), np.empty(L)) if extremes else (None, None)
    _lib.check(fn(ctx.h, model.h, _lib.dptr(values), _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(rho), L, C.byref(cnt)), ctx.h)
    return values, lo, hi, rho, cnt.value


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


class Script:
    """A scripted chain, after the one of tests/test_chain_diagnostics_gpu.py: every "step" writes chosen values into the
    process fields, refreshes the device model (which leaves the sums and the markers alone) and calls the two accumulates,
    as a step-by-step driver does after its sweeps.  The values are arbitrary doubles (uniform and Gamma draws, nothing
    dyadic); entry 1 of every group is constant, entries 4 and 5 of W share one history, entry 7 of W is exactly 0 on about
    half the steps, and for a network process A flips (two links never do) and ρ is a uniform draw."""

    def __init__(self, nhp, N, kind, network, seed, effective=False):
        from nhp_amd import _lib, inference
        from nhp_amd.components import param_layout
        self.nhp, self._lib, self.N, self.network, self.effective = nhp, _lib, N, network, effective
        self.proc = random_case(N, 10, 5.0, kind, 1.0, network=network, seed=1, nhp=nhp)["proc"]
        self.lay = param_layout(self.proc)
        self.L = inference.moments_length(self.proc)
        self.P = self.lay.weights.stop
        self.ctx = nhp.default_context()
        self.rng = np.random.default_rng(seed)
        self.model = None
        NN = N * N
        i0 = self.lay.impulses.start
        self.slices = [self.lay.baseline, slice(i0, i0 + NN), slice(i0 + NN, self.lay.impulses.stop), self.lay.weights]

    def draw(self):
        x = np.concatenate([self.rng.uniform(0.1, 3.0, self.L // 2), self.rng.gamma(0.7, 1.3, self.L - self.L // 2)])
        self.rng.shuffle(x)
        for s in self.slices:
            if s.stop - s.start > 1:
                x[s.start + 1] = 0.3
        w0 = self.lay.weights.start
        x[w0 + 5] = x[w0 + 4]
        if self.rng.uniform() < 0.5:
            x[w0 + 7] = 0.0
        if self.network:
            x[self.lay.adjacency] = self.rng.integers(0, 2, self.N * self.N)
            x[self.lay.adjacency.start + 1] = 0.0
            x[self.lay.adjacency.start + 2] = 1.0
            x[self.lay.adjacency.start + 5] = x[self.lay.adjacency.start + 4]       # (one history under effective weights too)
        return x, self.rng.uniform(0.05, 0.95)

    def write(self, x):
        p, lay, N = self.proc, self.lay, self.N
        p.baseline.λ = x[lay.baseline].copy()
        p.impulses.params_(x[lay.impulses])
        p.weights.params_(x[lay.weights])
        if self.network:
            p.adjacency_matrix = x[lay.adjacency].reshape((N, N), order="F").copy()
        self.model = p.device_model(self.ctx)

    def fed(self, x):
        """What the quantiles are fed for the state x: the first P entries, W as A·W with effective weights."""
        v = x[:self.P].copy()
        if self.effective and self.network:
            v[self.lay.weights] = x[self.lay.adjacency] * x[self.lay.weights]
        return v

    def start(self, probs, every=1):
        x, _ = self.draw()                                   # (a model to configure: the first step overwrites the values)
        self.write(x)
        configure(self.ctx, self.model, probs, every, self.effective)
        self._lib.check(self._lib.lib().nhp_cont_model_moments_reset(self.ctx.h, self.model.h), self.ctx.h)
        self.probs = probs
        self.acc, self.acc_rho = ref.P2(probs, self.P), ref.P2(probs, 1)

    def run(self, n):
        lib = self._lib.lib()
        for _ in range(n):
            x, rho = self.draw()
            self.write(x)
            if self.network:
                self._lib.check(lib.nhp_cont_model_set_rho(self.ctx.h, self.model.h, float(rho)), self.ctx.h)
            self._lib.check(lib.nhp_cont_model_moments_accumulate(self.ctx.h, self.model.h), self.ctx.h)
            self._lib.check(lib.nhp_cont_model_quantiles_accumulate(self.ctx.h, self.model.h), self.ctx.h)
            self.acc.add(self.fed(x))
            self.acc_rho.add(np.array([rho]))

    def check(self):
        m = len(self.probs)
        values, lo, hi, rho, n = fetch(self.ctx, self.model, self.L, m)
        assert n == self.acc.n
        want = self.acc.values()
        bad = int(np.sum(~((values[:, :self.P] == want) | (np.isnan(values[:, :self.P]) & np.isnan(want)))))
        print(f"n = {n}: {bad} of {want.size} estimates differ from the restatement")
        assert same(values[:, :self.P], want)
        assert same(lo[:self.P], self.acc.min()) and same(hi[:self.P], self.acc.max())
        # vec(A) has no state
        assert np.all(np.isnan(values[:, self.P:])) and np.all(np.isnan(lo[self.P:])) and np.all(np.isnan(hi[self.P:]))
        if self.network:
            assert same(rho, np.concatenate([self.acc_rho.values()[:, 0], self.acc_rho.min(), self.acc_rho.max()]))
        else:
            assert np.all(np.isnan(rho))
        # without the extremes the estimates are the same
        again = fetch(self.ctx, self.model, self.L, m, extremes=False)
        assert same(again[0], values)
        return values, lo, hi


@pytest.mark.parametrize("m", [1, 3, 4])
@pytest.mark.parametrize("N,kind,network,effective", [(3, "exponential", False, False), (40, "logitnormal", True, False),
                                                     (40, "logitnormal", True, True)])
def test_scripted_chain_bit_for_bit(nhp, N, kind, network, effective, m):
    """N = 3 exponential: P = len = 21, odd.  N = 40 logit-normal network: P = 4840 of len = 6440, several workgroups, a ragged
    tail, the A seam, raw W and A·W.  Fetched after 4 steps (fewer than K = 2m + 3 for every m: K = 5 at m = 1), after 5, at
    exactly K, at K + 1 and at 60 steps."""
    s = Script(nhp, N, kind, network, seed=11 + m, effective=effective)
    assert (s.P, s.L) == ((21, 21) if N == 3 else (4840, 6440))
    K = 2 * m + 3
    s.start(PROBS[m])
    done = 0
    for stop in sorted({4, 5, K, K + 1, 60}):
        s.run(stop - done)
        done = stop
        values, lo, hi = s.check()
        if stop < K:
            assert np.all(np.isnan(values)) and np.all(np.isfinite(lo[:s.P])) and np.all(lo[:s.P] <= hi[:s.P])
        else:
            assert np.all(np.isfinite(values[:, :s.P]))
    w0 = s.lay.weights.start
    assert np.all(values[:, s.lay.baseline.start + 1] == 0.3)                   # a constant entry: that constant everywhere
    if not effective:
        assert np.all(values[:, w0 + 1] == 0.3) and lo[w0 + 1] == hi[w0 + 1] == 0.3
    assert np.array_equal(values[:, w0 + 4], values[:, w0 + 5])                 # two entries with one history
    assert lo[w0 + 7] == 0.0 and hi[w0 + 7] > 0.0                               # the entry that is exactly 0 half the time
    if effective:                                                               # a link that is never there: A·W = 0 throughout
        assert np.all(values[:, w0 + 1] == 0.0) and hi[w0 + 1] == 0.0
    configure(s.ctx, s.model, None)


def test_grid_stride(nhp):
    """P = 524 800 entries exceed 2048·256, so the stride loop runs twice: N = 512, exponential, standard, m = 3, 12 steps (the
    warm-up's nine and three updates)."""
    s = Script(nhp, 512, "exponential", False, seed=5)
    assert s.P == s.L == 524800 > 2048 * 256
    s.start(PROBS[3])
    s.run(12)
    values, lo, hi = s.check()
    assert np.all(np.isfinite(values)) and s.acc.n == 12
    configure(s.ctx, s.model, None)


def case(nhp, kind, network):
    return random_case(8, 400, 60.0, kind, 1.0, network=network, seed=17, nhp=nhp)


def stateful(proc, network):
    """Mask over params(process): the entries that have a quantile state (everything but vec(A))."""
    from nhp_amd.components import param_layout
    keep = np.ones(len(proc.params()), dtype=bool)
    if network:
        keep[param_layout(proc, True).adjacency] = False
    return keep


@pytest.mark.parametrize("kind,network", [("exponential", False), ("logitnormal", True)])
def test_real_chains_on_every_route(nhp, kind, network):
    """60 steps, burn 10: the step-by-step device route with its samples kept against the restatement fed those samples, the
    resident route against the same bits, every third kept step, and the sums and diagnostics untouched by the new launch."""
    def chain(**kw):
        c = case(nhp, kind, network)
        return c["proc"], nhp.mcmc_(c["proc"], c["data"], nsteps=60, burn=10, seed=3, moments=True, **kw)

    proc, res = chain(keep_samples=True, quantiles=True)
    q = res.quantiles
    S = np.array(res.samples[10:])
    assert q.n == 50 and q.every == 1 and tuple(q.probs) == PROBS[3] and q.values.shape == (3, S.shape[1])
    keep = stateful(proc, network)
    want = ref.feed(PROBS[3], S)
    print(f"{int(np.sum(q.values[:, keep] != want.values()[:, keep]))} of {3 * keep.sum()} estimates differ from the restatement")
    assert same(q.values[:, keep], want.values()[:, keep])
    assert same(q.min[keep], S.min(axis=0)[keep]) and same(q.max[keep], S.max(axis=0)[keep])
    assert np.all(np.isfinite(q.values[:, keep]))
    assert np.all(np.isnan(q.values[:, ~keep])) and np.all(np.isnan(q.min[~keep]))
    lo, hi = q.interval(0.95)
    assert np.array_equal(lo, q.values[0], equal_nan=True) and np.array_equal(hi, q.values[2], equal_nan=True)
    assert np.all(lo[keep] <= hi[keep]) and np.any(lo[keep] < hi[keep])
    if network:                                               # entry 0 is the Bernoulli network's ρ: it moved
        assert keep[0] and q.min[0] < q.values[1, 0] < q.max[0]
    # the resident route: the same bits
    _, resident = chain(keep_samples=False, quantiles=True)
    assert same(resident.quantiles.values, q.values) and same(resident.quantiles.min, q.min) and same(resident.quantiles.max, q.max)
    # ... and cut into pieces of 7 steps
    _, cut = chain(keep_samples=False, quantiles=True, verbose=True, log_freq=7)
    assert same(cut.quantiles.values, q.values)
    # every third kept step, on both routes
    for kw in (dict(keep_samples=True), dict(keep_samples=False)):
        _, third = chain(quantiles=PROBS[3], quantiles_every=3, **kw)
        assert third.quantiles.n == 17 and third.quantiles.every == 3
        assert same(third.quantiles.values[:, keep], ref.feed(PROBS[3], S, every=3).values()[:, keep])
    # the sums and the diagnostics keep their bits
    _, plain = chain(keep_samples=False, diagnostics="full")
    _, both = chain(keep_samples=False, diagnostics="full", quantiles=True)
    assert not hasattr(plain, "quantiles")
    assert np.array_equal(both.mean, plain.mean) and np.array_equal(both.m2, plain.m2)
    assert np.array_equal(res.mean, plain.mean) and np.array_equal(res.m2, plain.m2)
    for name in ("ess", "mcse", "rhat"):
        assert same(both.diagnostics[name], plain.diagnostics[name])
    assert both.diagnostics["summary"] == plain.diagnostics["summary"] or all(
        same(list(both.diagnostics["summary"][g].values()), list(plain.diagnostics["summary"][g].values())) for g in plain.diagnostics["summary"])
    assert same(both.quantiles.values, q.values)
    if network:                                               # effective weights: A·W in W's place, one rounded product
        from nhp_amd.components import param_layout
        lay = param_layout(proc, True)
        _, eff = chain(keep_samples=True, quantiles=True, effective_weights=True)
        E = S.copy()
        E[:, lay.weights] = S[:, lay.adjacency] * S[:, lay.weights]
        assert same(eff.quantiles.values[:, keep], ref.feed(PROBS[3], E).values()[:, keep])
        assert same(eff.quantiles.min[keep], E.min(axis=0)[keep])


# ---- the discrete resident chain: the small generator of tests/test_disc_chain_gpu.py, restated ---------------------------------
def make_disc(nhp, N, T, B, L, rate, seed, network):
    rng = np.random.default_rng(seed)
    data = rng.poisson(rate, (N, T)).astype(np.int64)
    th = rng.dirichlet(np.ones(B), (N, N))
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    while not np.all(th.sum(axis=2) == 1.0):                    # the constructor checks the sum exactly
        th = rng.dirichlet(np.ones(B), (N, N))
        th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.05, 0.3, N), 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(th, L, 1.0),
                                             nhp.DenseWeightModel(rng.uniform(0.0, 0.5, (N, N)) / N * (4.0 if network else 1.0)), 1.0)
    if network:
        A = (np.random.default_rng(seed + 50).uniform(size=(N, N)) < 0.5).astype(np.float64)
        proc = nhp.DiscreteNetworkHawkesProcess(proc.baseline, proc.impulses, proc.weights, A, nhp.BernoulliNetworkModel(0.3, N), proc.dt)
    return proc, data


@pytest.mark.parametrize("network", [False, True])
def test_discrete_resident_chain(nhp, network):
    """N = 6, B = 3, T = 400: the resident route that also keeps its draws (keep_samples=True, moments=True) against the
    restatement fed those draws -- for the standard process the products W∘θ -- and the whole chain inside the library
    (keep_samples=False) against the same bits."""
    N, B = 6, 3
    proc, data = make_disc(nhp, N, 400, B, 5, 0.4, seed=21, network=network)
    start = copy.deepcopy(proc)
    res = nhp.mcmc_(proc, data, nsteps=40, burn=6, seed=2, keep_samples=True, moments=True, quantiles=True)
    q = res.quantiles
    S = np.array(res.samples[6:])
    keep = np.ones(S.shape[1], dtype=bool)
    if network:
        keep[1 + N + N * N + N * N * B:] = False              # params(process) = [ρ; λ0; W; θ; vec(A)]
        assert S.shape[1] == 1 + N + N * N * (B + 2)
    else:
        assert S.shape[1] == N + N * N * B
    assert q.n == 34 and q.values.shape == (3, S.shape[1])
    want = ref.feed(PROBS[3], S)
    print(f"{int(np.sum(q.values[:, keep] != want.values()[:, keep]))} of {3 * keep.sum()} estimates differ from the restatement")
    assert same(q.values[:, keep], want.values()[:, keep])
    assert same(q.min[keep], S.min(axis=0)[keep]) and same(q.max[keep], S.max(axis=0)[keep])
    assert np.all(np.isfinite(q.values[:, keep])) and np.all(np.isnan(q.values[:, ~keep]))
    resident = nhp.mcmc_(copy.deepcopy(start), data, nsteps=40, burn=6, seed=2, keep_samples=False, moments=True, quantiles=True)
    assert same(resident.quantiles.values, q.values) and same(resident.quantiles.max, q.max)
    assert np.array_equal(resident.mean, res.mean)
    third = nhp.mcmc_(copy.deepcopy(start), data, nsteps=40, burn=6, seed=2, keep_samples=False, moments=True, quantiles=True,
                      quantiles_every=3)
    assert third.quantiles.n == 12
    assert same(third.quantiles.values[:, keep], ref.feed(PROBS[3], S, every=3).values()[:, keep])
    if network:
        eff = nhp.mcmc_(copy.deepcopy(start), data, nsteps=40, burn=6, seed=2, keep_samples=False, moments=True, quantiles=True,
                        effective_weights=True)
        E = S.copy()
        W, A = slice(1 + N, 1 + N + N * N), slice(1 + N + N * N * (B + 1), None)
        E[:, W] = S[:, A] * S[:, W]
        assert same(eff.quantiles.values[:, keep], ref.feed(PROBS[3], E).values()[:, keep])


def test_state_and_refusals(nhp):
    from nhp_amd import _lib, inference
    s = Script(nhp, 3, "exponential", False, seed=2)
    lib = _lib.lib()
    s.start(PROBS[3])
    s.run(12)
    s.check()
    # another m: other planes, from zero
    s.start(PROBS[4])
    assert fetch(s.ctx, s.model, s.L, 4)[4] == 0
    s.run(13)
    s.check()
    # a moments reset clears the markers too
    _lib.check(lib.nhp_cont_model_moments_reset(s.ctx.h, s.model.h), s.ctx.h)
    values, lo, hi, rho, n = fetch(s.ctx, s.model, s.L, 4)
    assert n == 0 and np.all(np.isnan(values)) and np.all(np.isnan(lo)) and np.all(np.isnan(hi))
    s.acc, s.acc_rho = ref.P2(PROBS[4], s.P), ref.P2(PROBS[4], 1)
    s.run(12)
    s.check()
    with pytest.raises(ValueError, match="length"):
        fetch(s.ctx, s.model, s.L + 1, 4)
    # bad configurations are refused and leave the state as it was
    for probs, every in (((0.1, 0.2, 0.3, 0.4, 0.5), 1), ((0.5, 0.5), 1), ((0.5, 0.2), 1), ((0.0, 0.5), 1), ((0.5, 1.0), 1), ((0.5,), 0)):
        with pytest.raises(_lib.NhpError, match="quantiles"):
            configure(s.ctx, s.model, probs, every)
    s.check()
    # m = 0 frees the state: nothing to fetch, nothing to feed
    configure(s.ctx, s.model, None)
    with pytest.raises(_lib.NhpError, match="nothing configured"):
        fetch(s.ctx, s.model, s.L, 4)
    with pytest.raises(_lib.NhpError, match="nothing configured"):
        _lib.check(lib.nhp_cont_model_quantiles_accumulate(s.ctx.h, s.model.h), s.ctx.h)
    _lib.check(lib.nhp_cont_model_moments_accumulate(s.ctx.h, s.model.h), s.ctx.h)      # the sums go on
    # an LGCP baseline is not covered
    g = random_case(3, 60, 10.0, "exponential", 1.0, lgcp=True, seed=4, nhp=nhp)
    with pytest.raises(NotImplementedError, match="homogeneous"):
        configure(s.ctx, g["proc"].device_model(s.ctx), PROBS[3])
    # a column shard cannot keep quantiles: each rank would see its own columns only
    c = random_case(4, 500, 50.0, "exponential", 1.0, seed=2, nhp=nhp)
    model = c["proc"].device_model(s.ctx)
    configure(s.ctx, model, PROBS[1])
    t, n, T = c["data"]
    shard = C.c_void_p()
    _lib.check(lib.nhp_cont_dataset_create_columns(s.ctx.h, _lib.dptr(_lib.f64(t)), _lib.iptr(np.ascontiguousarray(n, dtype=np.int64)), len(t), 4,
                                                  float(T), 1.0, 0, 2, C.byref(shard)), s.ctx.h)
    try:
        pri = inference._priors(c["proc"])
        with pytest.raises(NotImplementedError, match="column shard"):
            _lib.check(lib.nhp_cont_mcmc_run(s.ctx.h, None, shard, model.h, C.byref(pri), 0.0, 0.0, 1, 0, 2, 0), s.ctx.h)
    finally:
        lib.nhp_cont_dataset_destroy(shard)
        configure(s.ctx, model, None)
    with pytest.raises(NotImplementedError, match="sharded"):
        nhp.mcmc_(c["proc"], nhp.sharded.ShardedDataset(c["proc"], c["data"], s.ctx), nsteps=4, keep_samples=False, moments=True, quantiles=True)
    # the discrete model: nothing configured, then configured, then freed
    proc, data = make_disc(nhp, 4, 50, 2, 4, 0.4, seed=3, network=False)
    from nhp_amd.discrete import DiscreteDeviceModel, disc_moments_length
    dm = DiscreteDeviceModel(s.ctx, proc)
    try:
        L = disc_moments_length(proc)
        with pytest.raises(_lib.NhpError, match="nothing configured"):
            fetch(s.ctx, dm, L, 3, disc=True)
        configure(s.ctx, dm, PROBS[3], disc=True)
        _lib.check(lib.nhp_disc_model_quantiles_accumulate(s.ctx.h, dm.h), s.ctx.h)
        values, lo, hi, rho, n = fetch(s.ctx, dm, L, 3, disc=True)
        assert n == 1 and np.all(np.isnan(values)) and np.array_equal(lo, proc.params()) and np.array_equal(hi, lo)
        _lib.check(lib.nhp_disc_model_moments_reset(s.ctx.h, dm.h), s.ctx.h)
        assert fetch(s.ctx, dm, L, 3, disc=True)[4] == 0
        configure(s.ctx, dm, None, disc=True)
        with pytest.raises(_lib.NhpError, match="nothing configured"):
            fetch(s.ctx, dm, L, 3, disc=True)
    finally:
        dm.close()
