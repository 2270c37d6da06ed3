"""The discrete chain on the device (nhp_disc_model_*, nhp_disc_mcmc_run, csrc/disc_chain.hip): step-for-step identity with
the default route and with the one-step host entries, the running sums and streaming diagnostics against the numpy
restatement of their definitions (tests/chain_diagnostics_ref.py), identity between the routes, and the refusals."""
import copy
import ctypes as C

import numpy as np
import pytest

import chain_diagnostics_ref as ref
from helpers import random_case

pytestmark = pytest.mark.gpu

GROUPS = ("baseline", "group1", "group2", "weights", "adjacency", "network.ρ")


# the small generator of tests/test_discrete_gibbs_gpu.py, restated
def make(nhp, N, T, B, L, rate, seed, dt=1.0):
    rng = np.random.default_rng(seed)
    data = rng.poisson(rate, (N, T)).astype(np.int64)
    th = rng.dirichlet(np.ones(B), (N, N))
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    while not np.all(th.sum(axis=2) == 1.0):                    # the constructor checks the sum exactly
        th = rng.dirichlet(np.ones(B), (N, N))
        th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.05, 0.3, N), dt),
                                             nhp.DiscreteGaussianImpulseResponse(th, L, dt),
                                             nhp.DenseWeightModel(rng.uniform(0.0, 0.5, (N, N)) / N), dt)
    return proc, data


def make_network(nhp, N, T, B, L, rate, seed):
    proc, data = make(nhp, N, T, B, L, rate, seed)
    rng = np.random.default_rng(seed + 50)
    A = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
    net = nhp.DiscreteNetworkHawkesProcess(proc.baseline, proc.impulses, proc.weights, A,
                                           nhp.BernoulliNetworkModel(0.3, N), proc.dt)
    return net, data


# ---- Test 1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,B,L,rate", [(3, 500, 4, 10, 0.3), (17, 129, 5, 9, 0.8), (130, 700, 2, 5, 0.05)])
def test_chain_identity_standard_process(nhp, N, T, B, L, rate):
    """The resident chain is the default route's chain, sample for sample and bit for bit: T off the tile, N past the
    128-node tile and N²B past one workgroup of the draw kernel."""
    proc, data = make(nhp, N, T, B, L, rate, seed=N + T)
    default, stepwise, resident = copy.deepcopy(proc), copy.deepcopy(proc), copy.deepcopy(proc)
    want = nhp.mcmc_(default, data, nsteps=6, seed=4)
    got = nhp.mcmc_(stepwise, data, nsteps=6, seed=4, keep_samples=True, moments=True)
    assert got.steps == 6 and len(got.samples) == 6
    for k in range(6):
        assert np.array_equal(got.samples[k], want.samples[k]), k
    assert not np.array_equal(want.samples[0], want.samples[5])
    last = nhp.mcmc_(resident, data, nsteps=6, seed=4, keep_samples=False)
    assert last.steps == 6 and len(last.samples) == 1
    for p in (stepwise, resident):
        assert np.array_equal(p.baseline.λ, default.baseline.λ)
        assert np.array_equal(p.weights.W, default.weights.W)
        assert np.array_equal(p.impulses.θ, default.impulses.θ)
    assert np.array_equal(last.samples[0], want.samples[5])


# ---- Test 2 ------------------------------------------------------------------------------------------------------------
def split_network_sample(x, N, B):
    NN = N * N
    rho, l0, W, th, A = np.split(x, [1, 1 + N, 1 + N + NN, 1 + N + NN + NN * B])
    return float(rho[0]), l0, W.reshape((N, N), order="F"), th.reshape((N, N, B), order="F"), A.reshape((N, N), order="F")


@pytest.mark.parametrize("N,T,B,L,rate", [(3, 300, 3, 6, 0.5), (5, 257, 2, 4, 1.5), (6, 1000, 8, 5, 0.2)])
def test_chain_identity_network_process(nhp, N, T, B, L, rate):
    """Five resident steps; step k replayed on the host from sample k − 1 (with its ρ) through nhp_disc_gibbs_step and the
    adjacency sweep's own entry: λ0, W, θ, A equal; ρ_k the bits nhp_cont_network_rho leaves for (α, β, ΣA_k, N², seed, k)."""
    from nhp_amd import _lib
    seed = 9
    proc, data = make_network(nhp, N, T, B, L, rate, seed=3 * N + T)
    proc.weights.W = proc.weights.W * N * 1.5                       # links that matter
    host = copy.deepcopy(proc)
    start = (proc.network.ρ, proc.baseline.λ.copy(), proc.weights.W.copy(), proc.impulses.θ.copy(), proc.adjacency_matrix.copy())
    res = nhp.mcmc_(proc, data, nsteps=5, seed=seed, keep_samples=True, moments=True)
    assert len(res.samples) == 5
    ctx = nhp.default_context()
    ds = nhp.convolve(host, data)
    lib = _lib.lib()
    # a throwaway continuous model for the ρ draw
    cm = random_case(N, 50, 10.0, "exponential", 1.0, network=True, seed=1, nhp=nhp)["proc"].device_model(ctx)
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
        _lib.check(lib.nhp_cont_network_rho(ctx.h, cm.h, 1.0, 1.0, float(links), float(N * N), seed, k), ctx.h)
        r3 = np.empty(3)
        _lib.check(lib.nhp_cont_model_get_rho(ctx.h, cm.h, _lib.dptr(r3)), ctx.h)
        assert got[0] == r3[0], (k, got[0], r3[0])
        prev = got
    assert flipped >= 1, "vacuous: A never changed"
    assert proc.network.ρ == prev[0] and np.array_equal(proc.adjacency_matrix, prev[4])


# ---- the C ABI by hand --------------------------------------------------------------------------------------------------
class Raw:
    """An nhp_disc_model driven entry by entry."""

    def __init__(self, nhp, N, B, network, dt=1.0):
        from nhp_amd import _lib
        self._lib, self.lib, self.ctx = _lib, _lib.lib(), nhp.default_context()
        self.N, self.B, self.network = N, B, network
        NN = N * N
        self.L = N + NN + NN * B + NN if network else N + NN * B
        self.h = C.c_void_p()
        self.ok(self.lib.nhp_disc_model_create(self.ctx.h, N, B, int(network), dt, C.byref(self.h)))

    def ok(self, rc):
        self._lib.check(rc, self.ctx.h)

    def set(self, l0, W, th, A=None, rho=None):
        d = self._lib.dptr
        self.ok(self.lib.nhp_disc_model_set(self.ctx.h, self.h, d(l0), d(W), d(th), d(A)))
        if rho is not None:
            self.ok(self.lib.nhp_disc_model_set_rho(self.ctx.h, self.h, float(rho)))

    def get(self):
        N, B = self.N, self.B
        out = [np.empty(N), np.empty(N * N), np.empty(N * N * B), np.empty(N * N) if self.network else None]
        self.ok(self.lib.nhp_disc_model_get(self.ctx.h, self.h, *[self._lib.dptr(v) for v in out]))
        return out

    def configure(self, b, n):
        self.ok(self.lib.nhp_disc_model_diagnostics_configure(self.ctx.h, self.h, b, n))

    def reset(self):
        self.ok(self.lib.nhp_disc_model_moments_reset(self.ctx.h, self.h))

    def accumulate(self):
        self.ok(self.lib.nhp_disc_model_moments_accumulate(self.ctx.h, self.h))

    def moments(self):
        s, q, n = np.empty(self.L), np.empty(self.L), C.c_int64()
        self.ok(self.lib.nhp_disc_model_moments_fetch(self.ctx.h, self.h, self._lib.dptr(s), self._lib.dptr(q), self.L, C.byref(n)))
        return s, q, n.value

    def rho(self):
        r3 = np.empty(3)
        self.ok(self.lib.nhp_disc_model_get_rho(self.ctx.h, self.h, self._lib.dptr(r3)))
        return r3

    def fetch(self, ess_below, rhat_above, full=True):
        summary = np.empty(self._lib.DIAG_GROUPS * self._lib.DIAG_FIELDS)
        planes = [np.empty(self.L) for _ in range(3)] if full else [None] * 3
        self.ok(self.lib.nhp_disc_model_diagnostics_fetch(self.ctx.h, self.h, ess_below, rhat_above, self._lib.dptr(summary),
                                                          *[self._lib.dptr(v) for v in planes], self.L))
        rows = [dict(zip(ref.FIELDS, row)) for row in summary.reshape(self._lib.DIAG_GROUPS, self._lib.DIAG_FIELDS)]
        return dict(zip(GROUPS, rows)), planes

    def run(self, ds, pri, net, seed, step0, n, burn):
        self.ok(self.lib.nhp_disc_mcmc_run(self.ctx.h, ds.h, self.h, *pri, *net, seed, step0, n, burn))

    def close(self):
        self.lib.nhp_disc_model_destroy(self.h)


def group_slices(N, B, network):
    """The five array groups in the order of the sums: 0 λ0, 1 θ | W∘θ, 2 empty, 3 W, 4 vec(A)."""
    NN = N * N
    if network:
        return [slice(0, N), slice(N + NN, N + NN + NN * B), slice(0, 0), slice(N, N + NN), slice(N + NN + NN * B, N + 2 * NN + NN * B)]
    return [slice(0, N), slice(N, N + NN * B), slice(0, 0), slice(0, 0), slice(0, 0)]


def same_summary(got, want, name):
    for f in ref.FIELDS:
        g, w = got[f], want[f]
        assert g == w or (np.isnan(g) and np.isnan(w)), (name, f, g, w)


# ---- Test 3 ------------------------------------------------------------------------------------------------------------
class Script:
    """Scripted states in exact arithmetic, through _set and _accumulate alone.  λ0, W: k/8 with k in 1..64; θ: j/8 with j in
    1..8 (so W·θ = kj/64 is exact, and so are its sums and the sums of its squares); A: 0 / 1; ρ: k/8 with k in 1..8.  Entry 1
    of λ0, W and θ is constant, two links never flip, entries 4 and 5 of W (and of θ) share one history."""

    def __init__(self, nhp, N, B, network, seed):
        self.m = Raw(nhp, N, B, network)
        self.N, self.B, self.network, self.rng = N, B, network, np.random.default_rng(seed)

    def draw(self):
        N, B, rng = self.N, self.B, self.rng
        NN = N * N
        l0, W, th = rng.integers(1, 65, N) / 8.0, rng.integers(1, 65, NN) / 8.0, rng.integers(1, 9, NN * B) / 8.0
        A = rng.integers(0, 2, NN).astype(np.float64) if self.network else None
        for v in (l0, W, th):
            if len(v) > 1:
                v[1] = 0.375
            if len(v) > 5:
                v[5] = v[4]
        if self.network and NN > 2:
            A[1], A[2] = 0.0, 1.0
        rho = rng.integers(1, 9) / 8.0 if self.network else None
        x = np.concatenate([l0, W, th, A]) if self.network else np.concatenate([l0, np.tile(W, B) * th])
        return (l0, W, th, A, rho), x

    def start(self, b, n_planned):
        self.m.configure(b, n_planned)
        self.m.reset()
        self.acc, self.acc_rho = ref.Accumulator(self.m.L, b, n_planned), ref.Accumulator(1, b, n_planned)

    def run(self, n):
        for _ in range(n):
            state, x = self.draw()
            self.m.set(*state)
            self.m.accumulate()
            self.acc.add(x)
            if self.network:
                self.acc_rho.add([state[4]])

    def check(self, ess_below, rhat_above):
        got, (ess, mcse, rhat) = self.m.fetch(ess_below, rhat_above)
        want = self.acc.fetch()
        s, q, n = self.m.moments()
        assert n == want["n"] and np.array_equal(s, self.acc.S1) and np.array_equal(q, self.acc.S2)
        for name, g, w in (("ess", ess, want["ess"]), ("mcse", mcse, want["mcse"]), ("rhat", rhat, want["rhat"])):
            ok = np.isfinite(w)
            err = np.max(np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300), initial=0.0)
            print(f"{name}: {ok.sum()} finite of {len(w)}, max relative difference {err:.2e}")
            assert np.array_equal(g, w, equal_nan=True), name          # NaN and ±inf in the same places, finite values equal
        for name, sl in zip(GROUPS, group_slices(self.N, self.B, self.network)):
            same_summary(got[name], ref.summarize(want, ess_below, rhat_above, sl), name)
        if self.network:
            same_summary(got["network.ρ"], ref.summarize(self.acc_rho.fetch(), ess_below, rhat_above), "network.ρ")
            r3 = self.m.rho()
            assert r3[1] == self.acc_rho.S1[0] and r3[2] == self.acc_rho.S2[0]
        else:
            assert got["network.ρ"]["entries"] == 0 and got["network.ρ"]["min_ess_index"] == -1
        again, _ = self.m.fetch(ess_below, rhat_above, full=False)        # the summary alone is the same summary
        assert all(np.array_equal(list(again[g].values()), list(got[g].values()), equal_nan=True) for g in GROUPS)
        return got, want


@pytest.mark.parametrize("N,B,network", [(1, 1, False), (1, 1, True), (3, 1, True), (23, 3, False), (23, 3, True), (200, 12, True)])
def test_scripted_states_in_exact_arithmetic(nhp, N, B, network):
    """2b + 1 kept steps with b = 4: two batches and a partial one, n odd so two snapshots.  N = 23, B = 3: 1610 / 2668
    entries, no multiple of 256; N = 200, B = 12 network: 560 200 entries, more than 2048 x 256, so the stride loop takes a
    second trip.  The standard kind's entries are products W·θ that are exact in fp64: the product path, exactly."""
    s = Script(nhp, N, B, network, seed=7 + N)
    NN = N * N
    assert s.m.L == (N + 2 * NN + NN * B if network else N + NN * B)
    if N == 200:
        assert s.m.L == 560200 > 2048 * 256
    try:
        s.start(4, 9)
        s.run(5)                                                  # a = 1: ESS and MCSE are NaN; n != n_planned: R-hat is NaN
        got, want = s.check(10.0, 1.2)
        assert want["a"] == 1 and np.all(np.isnan(want["ess"])) and np.all(np.isnan(want["rhat"]))
        s.run(4)                                                  # the planned 9
        got, want = s.check(10.0, 1.2)
        assert want["a"] == 2 and want["n"] == 9
        assert got["baseline"]["entries"] == N and got["group2"]["entries"] == 0
        assert got["group1"]["entries"] == NN * B
        assert got["weights"]["entries"] == (NN if network else 0) and got["adjacency"]["entries"] == (NN if network else 0)
        if N >= 3:
            assert got["baseline"]["undefined"] == 1 and np.isfinite(want["rhat"]).sum() > s.m.L // 2
            assert got["group1"]["min_ess_index"] >= 0 and got["group1"]["max_rhat_index"] >= 0
            assert got["group1"]["min_ess_index"] != 5 and got["group1"]["max_rhat_index"] != 5      # the tie goes to entry 4
        if network and N >= 3:
            assert got["adjacency"]["undefined"] >= 2 and got["network.ρ"]["entries"] == 1
        # a reset starts clean: other lengths (n even: one snapshot)
        s.start(3, 6)
        s.run(6)
        s.check(5.0, 1.1)
    finally:
        s.m.close()


# ---- Test 4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("network", [False, True])
def test_real_chain_against_the_restatement_on_its_samples(nhp, network):
    """40 kept steps of a real chain, b = 6: every entry's ESS, MCSE and R-hat against the restatement on the kept samples
    within ref.tolerances, the summary group by group, the mean exactly and the mean square within n·ε (every term is
    positive; a fused multiply-add differs from multiply-then-add by at most ε/2 per term)."""
    N, T, B = 5, 2500, 3
    proc, data = (make_network if network else make)(nhp, N, T, B, 6, 0.1, seed=31)
    res = nhp.mcmc_(proc, data, nsteps=50, burn=10, seed=3, keep_samples=True, moments=True, diagnostics="full", batch_len=6)
    d = res.diagnostics
    assert d["n"] == 40 and d["batch_len"] == 6 and d["nbatches"] == 6 and res.n == 40
    S = np.array(res.samples[10:])
    want = ref.diagnose(S, 6)
    tol = ref.tolerances(want)
    defined = tight = 0
    for name in ("ess", "mcse", "rhat"):
        g, w, t = d[name], want[name], tol[name]
        assert g.shape == w.shape == S[0].shape
        ok = np.isfinite(w)
        assert np.array_equal(g[~ok], w[~ok], equal_nan=True), name
        same = g[ok] == w[ok]
        with np.errstate(invalid="ignore", divide="ignore"):
            relerr = np.where(same, 0.0, np.abs(g[ok] - w[ok]) / np.abs(w[ok]))
        print(f"{name}: {ok.sum()} finite of {len(w)}, {same.sum()} equal; max relative difference {relerr.max():.2e}; tolerance "
              f"median {np.median(t[ok]):.2e}, max {t[ok].max():.2e}")
        assert np.all(same | (relerr <= t[ok])), name
        defined += ok.sum()
        tight += np.sum(t[ok] < 1e-9)
    print(f"{tight} of {defined} tolerances below 1e-9: a share of {tight / defined:.3f}")
    assert tight >= 0.9 * defined, "vacuous: the tolerances are too wide to hold anything"
    # the summary is the summary of these values, group by group in params(process) order
    NN = N * N
    if network:
        cut = np.cumsum([0, 1, N, NN, NN * B, NN])
        groups = dict(zip(("network.ρ", "baseline", "weights", "impulses.θ", "adjacency"), (slice(a, b) for a, b in zip(cut, cut[1:]))))
    else:
        groups = {"baseline": slice(0, N), "weights∘impulses": slice(N, N + NN * B)}
    assert sorted(d["summary"]) == sorted(groups)
    dev = {"ess": d["ess"], "mcse": d["mcse"], "rhat": d["rhat"], "undefined": want["undefined"]}
    for name, sl in groups.items():
        w = ref.summarize(dev, 100.0, 1.01, sl)
        for f in ref.FIELDS:
            assert d["summary"][name][f] == w[f] or (np.isnan(d["summary"][name][f]) and np.isnan(w[f])), (name, f)
    # the sums themselves
    s1, s2 = np.zeros(S.shape[1]), np.zeros(S.shape[1])
    for x in S:
        s1 += x
        s2 += x * x
    assert np.array_equal(res.mean, s1 / 40)
    m2 = s2 / 40
    err = np.max(np.abs(res.m2 - m2) / np.where(m2 > 0.0, m2, 1.0))
    print(f"m2: max relative difference {err:.2e} against n·ε = {40 * np.finfo(float).eps:.2e}")
    assert np.all(np.abs(res.m2 - m2) <= 40 * np.finfo(float).eps * m2)


# ---- Test 5 ------------------------------------------------------------------------------------------------------------
def same_diagnostics(a, b):
    assert a["n"] == b["n"] and a["batch_len"] == b["batch_len"] and a["summary"].keys() == b["summary"].keys()
    for g in a["summary"]:
        assert np.array_equal(list(a["summary"][g].values()), list(b["summary"][g].values()), equal_nan=True), g
    for name in ("ess", "mcse", "rhat"):
        assert np.array_equal(a[name], b[name], equal_nan=True), name


@pytest.mark.parametrize("network", [False, True])
def test_routes_and_repeats(nhp, network):
    """keep_samples=False (nhp_disc_mcmc_run), keep_samples=True (step by step), the driver cut at log_freq = 7, and a repeat:
    one chain, the same bits in mean, m2 and every diagnostic; at the C ABI a run in two halves through step0 is the run."""
    N, T, B = 5, 1200, 3

    def chain(**kw):
        proc, data = (make_network if network else make)(nhp, N, T, B, 6, 0.2, seed=12)
        return nhp.mcmc_(proc, data, nsteps=30, burn=7, seed=3, moments=True, diagnostics="full", **kw), proc

    resident, p0 = chain(keep_samples=False)
    assert resident.n == 23 and np.all(np.isfinite(resident.mean))
    plain = nhp.mcmc_(*(make_network if network else make)(nhp, N, T, B, 6, 0.2, seed=12), nsteps=30, burn=7, seed=3, moments=True,
                      keep_samples=False)
    assert not hasattr(plain, "diagnostics")
    assert np.array_equal(plain.mean, resident.mean) and np.array_equal(plain.m2, resident.m2)      # the fused kernel keeps the sums' bits
    for kw in (dict(keep_samples=True), dict(keep_samples=False, verbose=True, log_freq=7), dict(keep_samples=False)):
        other, p1 = chain(**kw)
        assert np.array_equal(other.mean, resident.mean, equal_nan=True) and np.array_equal(other.m2, resident.m2, equal_nan=True), kw
        same_diagnostics(other.diagnostics, resident.diagnostics)
        assert np.array_equal(p1.params(), p0.params())
    brief = nhp.mcmc_(*(make_network if network else make)(nhp, N, T, B, 6, 0.2, seed=12), nsteps=30, burn=7, seed=3, moments=True,
                      keep_samples=False, diagnostics=True)
    assert "ess" not in brief.diagnostics
    for g, row in resident.diagnostics["summary"].items():
        assert np.array_equal(list(brief.diagnostics["summary"][g].values()), list(row.values()), equal_nan=True), g

    # the C ABI: 30 steps in one call and as 13 + 17 through step0
    from nhp_amd import _lib
    proc, data = (make_network if network else make)(nhp, N, T, B, 6, 0.2, seed=12)
    ds = nhp.convolve(proc, data)
    l0, W, th, A = proc._lowered()
    pri = (proc.baseline.α0, proc.baseline.β0, proc.weights.κ, proc.weights.ν, proc.impulses.γ)
    out = []
    for pieces in ((30,), (13, 17)):
        m = Raw(nhp, N, B, network)
        try:
            m.set(l0, W, th, A, 0.3 if network else None)
            m.configure(4, 23)
            m.reset()
            step = 0
            for n in pieces:
                m.run(ds, pri, (1.0, 1.0), 3, step, n, 7)
                step += n
            out.append((m.moments(), m.fetch(100.0, 1.01), m.get(), m.rho() if network else None))
        finally:
            m.close()
    (mo0, (su0, pl0), st0, r0), (mo1, (su1, pl1), st1, r1) = out
    assert mo0[2] == mo1[2] == 23 and np.array_equal(mo0[0], mo1[0]) and np.array_equal(mo0[1], mo1[1])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(pl0, pl1))
    assert all(np.array_equal(list(su0[g].values()), list(su1[g].values()), equal_nan=True) for g in GROUPS)
    assert all(np.array_equal(a, b) for a, b in zip(st0, st1) if a is not None)
    if network:
        assert np.array_equal(r0, r1)
    # ... and it is the Python route's chain: same sums
    k = 1 if network else 0
    assert np.array_equal(mo0[0] / 23, resident.mean[k:]) and np.array_equal(mo0[1] / 23, resident.m2[k:])


def test_dense_network_keeps_its_link_probability(nhp):
    proc, data = make_network(nhp, 4, 400, 2, 4, 0.4, seed=5)
    proc.network = nhp.DenseNetworkModel(4)
    res = nhp.mcmc_(proc, data, nsteps=6, seed=2, keep_samples=False, moments=True, diagnostics=True)
    assert res.n == 6 and len(res.mean) == len(proc.params()) and "network.ρ" not in res.diagnostics["summary"]
    assert set(np.unique(proc.adjacency_matrix)) <= {0.0, 1.0}


# ---- Test 6 ------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_c_abi(nhp):
    from nhp_amd import _lib
    proc, data = make(nhp, 3, 200, 2, 4, 0.4, seed=8)
    ds = nhp.convolve(proc, data)
    pri = (1.0, 1.0, 1.0, 1.0, 1.0)
    for N, B in ((4, 2), (3, 3)):                              # a model whose N or B is not the dataset's
        m = Raw(nhp, N, B, False)
        try:
            with pytest.raises(_lib.NhpError, match="does not match the dataset"):
                m.run(ds, pri, (0.0, 0.0), 1, 0, 1, 0)
            with pytest.raises(_lib.NhpError, match="does not match the dataset"):
                m.ok(m.lib.nhp_disc_model_gibbs_step(m.ctx.h, ds.h, m.h, *pri, 1, 0))
        finally:
            m.close()
    m = Raw(nhp, 3, 2, False)
    try:
        l0, W, th, _ = proc._lowered()
        m.set(l0, W, th)
        with pytest.raises(_lib.NhpError, match="nothing accumulated"):
            m.moments()
        with pytest.raises(_lib.NhpError, match="nothing configured"):
            m.fetch(100.0, 1.01)
        with pytest.raises(_lib.NhpError, match="batch_len"):
            m.configure(0, 10)
        m.configure(2, 10)
        with pytest.raises(_lib.NhpError, match="nothing accumulated"):
            m.fetch(100.0, 1.01)
        with pytest.raises(_lib.NhpError):                      # no adjacency matrix: no network step, no ρ
            m.ok(m.lib.nhp_disc_model_set_rho(m.ctx.h, m.h, 0.5))
        # configured in the middle of the sums: refused at fetch, not answered wrongly
        m.configure(0, 0)
        m.reset()
        m.accumulate()
        m.configure(2, 10)
        m.accumulate()
        with pytest.raises(_lib.NhpError, match="configured after"):
            m.fetch(100.0, 1.01)
        with pytest.raises(ValueError):                         # a wrong length
            m.ok(m.lib.nhp_disc_model_moments_fetch(m.ctx.h, m.h, _lib.dptr(np.empty(5)), _lib.dptr(np.empty(5)), 5, C.byref(C.c_int64())))
    finally:
        m.close()
    net = Raw(nhp, 3, 2, True)
    try:
        with pytest.raises(_lib.NhpError, match="link probability first"):
            net.run(ds, pri, (1.0, 1.0), 1, 0, 1, 0)
        with pytest.raises(_lib.DomainError):
            net.ok(net.lib.nhp_disc_model_set_rho(net.ctx.h, net.h, 1.5))
    finally:
        net.close()
