"""Streaming convergence diagnostics on the GPU (nhp_cont_model_diagnostics_*, csrc/cont_diagnostics.hip) against the numpy
restatement of their definitions (tests/chain_diagnostics_ref.py): a scripted chain in exact arithmetic, real chains with
tolerances from the conditioning of their sums, bit identity between the routes, and the network scalars."""
import ctypes as C

import numpy as np
import pytest

import chain_diagnostics_ref as ref
from helpers import random_case

pytestmark = pytest.mark.gpu

GROUPS = ("baseline", "impulses.1", "impulses.2", "weights", "adjacency", "network.ρ")


def configure(ctx, model, b, n_planned):
    from nhp_amd import _lib
    _lib.check(_lib.lib().nhp_cont_model_diagnostics_configure(ctx.h, model.h, b, n_planned), ctx.h)


def fetch(ctx, model, L, ess_below, rhat_above, full=True):
    from nhp_amd import _lib
    summary = np.empty(_lib.DIAG_GROUPS * _lib.DIAG_FIELDS)
    planes = [np.empty(L) for _ in range(3)] if full else [None] * 3
    _lib.check(_lib.lib().nhp_cont_model_diagnostics_fetch(ctx.h, model.h, ess_below, rhat_above, _lib.dptr(summary),
                                                          *[_lib.dptr(v) for v in planes], L), ctx.h)
    rows = [dict(zip(ref.FIELDS, row)) for row in summary.reshape(_lib.DIAG_GROUPS, _lib.DIAG_FIELDS)]
    return dict(zip(GROUPS, rows)), planes


class Script:
    """A scripted chain: every "step" writes values into the process fields, refreshes the device model (which leaves the
    sums alone) and calls nhp_cont_model_moments_accumulate, as a chain driver does after its sweeps.  Values are k/8 with
    k in 1..64 (A: 0 / 1, ρ: k/8 with k in 1..8), entry 1 of every group constant: every sum is exact in fp64."""

    def __init__(self, nhp, N, kind, network, seed):
        from nhp_amd import _lib, inference
        from nhp_amd.components import param_layout
        self.nhp, self._lib, self.N, self.network = nhp, _lib, N, network
        self.proc = random_case(N, 10, 5.0, kind, 1.0, network=network, seed=1, nhp=nhp)["proc"]
        self.lay = param_layout(self.proc)
        self.L = inference.moments_length(self.proc)
        self.ctx = nhp.default_context()
        self.rng = np.random.default_rng(seed)
        self.model = None
        self.slices = [self.lay.baseline]
        NN = N * N
        i0 = self.lay.impulses.start
        self.slices += [slice(i0, i0 + NN), slice(i0 + NN, self.lay.impulses.stop), self.lay.weights, self.lay.adjacency]

    def draw(self):
        x = self.rng.integers(1, 65, self.L) / 8.0
        for s in self.slices[:4]:
            if s.stop - s.start > 1:
                x[s.start + 1] = 0.375
        if self.network:
            x[self.lay.adjacency] = self.rng.integers(0, 2, self.N * self.N)
            x[self.lay.adjacency.start + 1] = 0.0            # two links that never flip
            x[self.lay.adjacency.start + 2] = 1.0
        x[self.lay.weights.start + 5] = x[self.lay.weights.start + 4]     # two entries with one history: a tie
        return x, self.rng.integers(1, 9) / 8.0

    def step(self, x, rho):
        p, lay, N = self.proc, self.lay, self.N
        p.baseline.λ = x[lay.baseline].copy()
        p.impulses.params_(x[lay.impulses])
        p.weights.params_(x[lay.weights])
        if self.network:
            p.adjacency_matrix = x[lay.adjacency].reshape((N, N), order="F").copy()
        self.model = p.device_model(self.ctx)
        lib = self._lib.lib()
        if self.network:
            self._lib.check(lib.nhp_cont_model_set_rho(self.ctx.h, self.model.h, float(rho)), self.ctx.h)
        self._lib.check(lib.nhp_cont_model_moments_accumulate(self.ctx.h, self.model.h), self.ctx.h)

    def start(self, b, n_planned):
        x, rho = self.draw()                                 # (a model to configure: values are overwritten by the first step)
        p, lay, N = self.proc, self.lay, self.N
        p.baseline.λ = x[lay.baseline].copy()
        p.impulses.params_(x[lay.impulses])
        p.weights.params_(x[lay.weights])
        self.model = p.device_model(self.ctx)
        configure(self.ctx, self.model, b, n_planned)
        self._lib.check(self._lib.lib().nhp_cont_model_moments_reset(self.ctx.h, self.model.h), self.ctx.h)
        self.acc, self.acc_rho = ref.Accumulator(self.L, b, n_planned), ref.Accumulator(1, b, n_planned)

    def run(self, n):
        for _ in range(n):
            x, rho = self.draw()
            self.step(x, rho)
            self.acc.add(x)
            self.acc_rho.add([rho])

    def check(self, ess_below, rhat_above):
        got, (ess, mcse, rhat) = fetch(self.ctx, self.model, self.L, ess_below, rhat_above)
        want = self.acc.fetch()
        for name, g, w in (("ess", ess, want["ess"]), ("mcse", mcse, want["mcse"]), ("rhat", rhat, want["rhat"])):
            ok = np.isfinite(w)                                # NaN and ±inf (equal batch means) in the same places
            assert np.array_equal(g[~ok], w[~ok], equal_nan=True), name
            err = np.max(np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300), initial=0.0)
            print(f"{name}: {ok.sum()} finite of {len(w)}, max relative difference {err:.2e}")
            assert np.all(np.abs(g[ok] - w[ok]) <= 1e-13 * np.abs(w[ok])), name
        dev = {"ess": ess, "mcse": mcse, "rhat": rhat, "undefined": want["undefined"]}
        for name, sl in zip(GROUPS, self.slices):
            self.same_summary(got[name], ref.summarize(want, ess_below, rhat_above, sl), name)
            # ... and exactly the summary of the per-entry values the device itself returned
            self.same_summary(got[name], ref.summarize(dev, ess_below, rhat_above, sl), name, exact=True)
        rho_want = self.acc_rho.fetch() if self.network else None
        if self.network:
            self.same_summary(got["network.ρ"], ref.summarize(rho_want, ess_below, rhat_above), "network.ρ")
        else:
            assert got["network.ρ"]["entries"] == 0 and got["network.ρ"]["min_ess_index"] == -1
        # the summary alone (no per-entry planes) is the same summary
        again, _ = fetch(self.ctx, self.model, self.L, ess_below, rhat_above, full=False)
        assert all(np.array_equal(list(again[g].values()), list(got[g].values()), equal_nan=True) for g in GROUPS)
        return got, want

    @staticmethod
    def same_summary(got, want, name, exact=False):
        for f in ref.FIELDS:
            g, w = got[f], want[f]
            if f in ("min_ess", "max_rhat", "max_mcse"):
                assert (np.isnan(g) and np.isnan(w)) or g == w or (not exact and abs(g - w) <= 1e-13 * abs(w)), (name, f, g, w)
            else:
                assert g == w, (name, f, g, w)


@pytest.mark.parametrize("N,kind,network", [(3, "exponential", False), (40, "logitnormal", True)])
def test_scripted_chain_in_exact_arithmetic(nhp, N, kind, network):
    """N = 3 exponential: len = 21, odd, so every second plane starts off 16-byte alignment.  N = 40 logit-normal network:
    len = 6440, several workgroups, the params / A seam, a ragged tail; 0 / 1 links, two that never flip.  b = 4 and 23
    steps: five batches and a partial one, n odd so two snapshots."""
    from nhp_amd import _lib
    s = Script(nhp, N, kind, network, seed=7)
    assert s.L == (21 if N == 3 else 6440)
    s.start(4, 23)
    s.run(7)                                                  # a = 1: ESS and MCSE are NaN; n != n_planned: R-hat is NaN
    got, want = s.check(10.0, 1.2)
    assert want["a"] == 1 and np.all(np.isnan(want["ess"])) and np.all(np.isnan(want["rhat"]))
    assert got["weights"]["min_ess_index"] == -1 and got["weights"]["undefined"] == 1
    s.run(13)                                                 # fewer steps than planned: ESS is defined, R-hat is not
    got, want = s.check(10.0, 1.2)
    assert want["a"] == 5 and np.all(np.isnan(want["rhat"])) and np.sum(~np.isnan(want["ess"])) == s.L - want["undefined"].sum() >= s.L - 6
    assert got["weights"]["min_ess_index"] >= 0 and got["weights"]["max_rhat_index"] == -1
    s.run(3)                                                  # the planned 23
    got, want = s.check(10.0, 1.2)
    assert np.isfinite(want["rhat"]).sum() >= s.L - 6 and got["weights"]["max_rhat_index"] >= 0
    assert got["baseline"]["entries"] == N and got["baseline"]["undefined"] == 1
    assert got["impulses.2"]["entries"] == (N * N if kind == "logitnormal" else 0)
    assert got["adjacency"]["undefined"] == (2 if network else 0) and got["adjacency"]["entries"] == (N * N if network else 0)
    if network:                                               # 0 / 1 entries: the tie rule is exercised by equal values
        assert got["network.ρ"]["entries"] == 1
    # entries 4 and 5 of W share one history: the lower index wins wherever they are the extreme
    w0 = s.lay.weights.start
    assert want["ess"][w0 + 4] == want["ess"][w0 + 5]
    assert got["weights"]["min_ess_index"] != 5 and got["weights"]["max_rhat_index"] != 5
    # reconfigure + reset starts clean: another script, other lengths (n even: one snapshot)
    s.start(3, 12)
    s.run(12)
    got, want = s.check(5.0, 1.1)
    assert want["a"] == 4 and np.isfinite(want["rhat"]).sum() > s.L // 2       # (a link constant inside both halves has W = 0: NaN)
    # reset alone zeroes the planes too
    _lib.check(_lib.lib().nhp_cont_model_moments_reset(s.ctx.h, s.model.h), s.ctx.h)
    s.acc, s.acc_rho = ref.Accumulator(s.L, 3, 12), ref.Accumulator(1, 3, 12)
    s.run(12)
    s.check(5.0, 1.1)
    # off: the fetch has nothing to report, the moments go on
    configure(s.ctx, s.model, 0, 0)
    with pytest.raises(_lib.NhpError, match="nothing configured"):
        fetch(s.ctx, s.model, s.L, 5.0, 1.1)
    x, rho = s.draw()
    s.step(x, rho)
    # configured in the middle of the sums: refused at fetch, not answered wrongly
    configure(s.ctx, s.model, 3, 12)
    s.step(x, rho)
    with pytest.raises(_lib.NhpError, match="configured after"):
        fetch(s.ctx, s.model, s.L, 5.0, 1.1)
    configure(s.ctx, s.model, 0, 0)


def params_order_slices(proc, network):
    from nhp_amd.components import param_layout
    return param_layout(proc, network)


@pytest.mark.parametrize("kind,network", [("exponential", False), ("logitnormal", True)])
def test_real_chain_against_the_restatement_on_its_samples(nhp, kind, network):
    """40 kept steps of a real chain, b = 6: every entry's ESS, MCSE and R-hat against the restatement on the kept samples,
    within 16·n·ε·κ relative, κ the condition of the raw-sum subtraction behind the value (ref.tolerances); for the network
    process entry 0 is the Bernoulli network's ρ.  Seed 31 / chain seed 3, the case of the moments test in
    test_cont_inference_gpu.py."""
    c = random_case(5, 2500, 250.0, kind, 1.0, network=network, seed=31, nhp=nhp)
    res = nhp.mcmc_(c["proc"], c["data"], nsteps=50, burn=10, seed=3, keep_samples=True, moments=True, diagnostics="full")
    d = res.diagnostics
    assert d["n"] == 40 and d["batch_len"] == 6 and d["nbatches"] == 6
    S = np.array(res.samples[10:])
    want = ref.diagnose(S, 6)
    tol = ref.tolerances(want)
    defined = tight = 0
    for name in ("ess", "mcse", "rhat"):
        g, w, t = d[name], want[name], tol[name]
        assert g.shape == w.shape == S[0].shape
        ok = np.isfinite(w)                                    # NaN and ±inf (equal batch means) in the same places, exactly
        assert np.array_equal(g[~ok], w[~ok], equal_nan=True), name
        same = g[ok] == w[ok]                                  # (the MCSE of an entry that never moved is 0 on both sides)
        with np.errstate(invalid="ignore", divide="ignore"):
            relerr = np.where(same, 0.0, np.abs(g[ok] - w[ok]) / np.abs(w[ok]))
        print(f"{name}: {ok.sum()} finite of {len(w)}, {same.sum()} equal; max relative difference {relerr.max():.2e}; tolerance "
              f"median {np.median(t[ok]):.2e}, max {t[ok].max():.2e}; worst entry at {np.max(relerr - np.where(same, 0.0, t[ok])):.2e} "
              f"past its tolerance")
        assert np.all(same | (relerr <= t[ok])), name
        defined += ok.sum()
        tight += np.sum(t[ok] < 1e-9)
    print(f"{tight} of {defined} tolerances below 1e-9")
    assert tight >= 0.9 * defined, "vacuous: the tolerances are too wide to hold anything"
    # the summary is the summary of these values, group by group in params(process) order
    lay = params_order_slices(c["proc"], network)
    NN = 25
    groups = {"baseline": lay.baseline, "weights": lay.weights}
    if kind == "exponential":
        groups["impulses.θ"] = lay.impulses
    else:
        groups["impulses.μ"] = slice(lay.impulses.start, lay.impulses.start + NN)
        groups["impulses.τ"] = slice(lay.impulses.start + NN, lay.impulses.stop)
    if network:
        groups["adjacency"], groups["network.ρ"] = lay.adjacency, slice(0, 1)
    assert sorted(d["summary"]) == sorted(groups)
    dev = {"ess": d["ess"], "mcse": d["mcse"], "rhat": d["rhat"], "undefined": want["undefined"]}
    for name, sl in groups.items():
        w = ref.summarize(dev, 100.0, 1.01, sl)
        for f in ref.FIELDS:
            assert d["summary"][name][f] == w[f] or (np.isnan(d["summary"][name][f]) and np.isnan(w[f])), (name, f)


@pytest.mark.parametrize("kind,network", [("exponential", False), ("logitnormal", True)])
def test_bit_identity_between_the_routes(nhp, kind, network):
    def chain(**kw):
        c = random_case(5, 2500, 250.0, kind, 1.0, network=network, seed=31, nhp=nhp)
        return nhp.mcmc_(c["proc"], c["data"], nsteps=30, burn=7, seed=3, moments=True, **kw)

    def same(a, b):
        assert a["n"] == b["n"] and a["batch_len"] == b["batch_len"] and a["summary"].keys() == b["summary"].keys()
        for g in a["summary"]:
            assert np.array_equal(list(a["summary"][g].values()), list(b["summary"][g].values()), equal_nan=True), g
        for name in ("ess", "mcse", "rhat"):
            assert np.array_equal(a[name], b[name], equal_nan=True), name

    plain = chain(keep_samples=False)
    assert not hasattr(plain, "diagnostics")
    resident = chain(keep_samples=False, diagnostics="full")
    # the sums keep their bits under the fused kernel
    assert np.array_equal(resident.mean, plain.mean) and np.array_equal(resident.m2, plain.m2)
    stepwise = chain(keep_samples=True, diagnostics="full")
    assert np.array_equal(stepwise.mean, plain.mean) and np.array_equal(stepwise.m2, plain.m2)
    same(stepwise.diagnostics, resident.diagnostics)
    cut = chain(keep_samples=False, diagnostics="full", verbose=True, log_freq=4)       # the resident driver in pieces of 4 steps
    same(cut.diagnostics, resident.diagnostics)
    same(chain(keep_samples=False, diagnostics="full").diagnostics, resident.diagnostics)
    # diagnostics=True: the summary alone, the same one
    brief = chain(keep_samples=False, diagnostics=True)
    assert "ess" not in brief.diagnostics and brief.diagnostics["summary"].keys() == resident.diagnostics["summary"].keys()
    for g, row in resident.diagnostics["summary"].items():
        assert np.array_equal(list(brief.diagnostics["summary"][g].values()), list(row.values()), equal_nan=True), g
    # a chain after one with diagnostics, on the same cached device model, runs without them
    c = random_case(5, 2500, 250.0, kind, 1.0, network=network, seed=31, nhp=nhp)
    nhp.mcmc_(c["proc"], c["data"], nsteps=6, seed=3, keep_samples=False, moments=True, diagnostics=True)
    for name in ("baseline", "impulses", "weights"):
        setattr(c["proc"], name, getattr(random_case(5, 2500, 250.0, kind, 1.0, network=network, seed=31, nhp=nhp)["proc"], name))
    if network:
        fresh = random_case(5, 2500, 250.0, kind, 1.0, network=network, seed=31, nhp=nhp)["proc"]
        c["proc"].adjacency_matrix, c["proc"].network = fresh.adjacency_matrix, fresh.network
    after = nhp.mcmc_(c["proc"], c["data"], nsteps=30, burn=7, seed=3, keep_samples=False, moments=True)
    assert np.array_equal(after.mean, plain.mean) and np.array_equal(after.m2, plain.m2)


def test_network_scalars(nhp):
    """The Bernoulli network's ρ is diagnosed (entry 0 of params(process), group "network.ρ") against the restatement on the
    kept ρ; a block network's ρ / π and a latent distance network's b are NaN and have no group."""
    c = random_case(6, 2500, 250.0, "exponential", 1.0, network=True, seed=12, nhp=nhp)
    res = nhp.mcmc_(c["proc"], c["data"], nsteps=44, burn=8, seed=5, keep_samples=True, moments=True, diagnostics="full", batch_len=5)
    rho = np.array(res.samples[8:])[:, 0]
    want = ref.diagnose(rho, 5)
    tol = ref.tolerances(want)
    d = res.diagnostics
    for name in ("ess", "mcse", "rhat"):
        print(name, d[name][0], want[name][0], tol[name][0])
        assert np.isfinite(want[name][0]) and tol[name][0] < 1e-9
        assert abs(d[name][0] - want[name][0]) <= tol[name][0] * abs(want[name][0])
    g = d["summary"]["network.ρ"]
    assert g["entries"] == 1 and g["undefined"] == 0 and g["min_ess_index"] == 0 and g["max_rhat_index"] == 0
    assert g["min_ess"] == d["ess"][0] and g["max_rhat"] == d["rhat"][0] and g["max_mcse"] == d["mcse"][0]

    N, K = 12, 2
    rng = np.random.default_rng(3)
    b = random_case(N, 2000, 150.0, "exponential", 1.0, network=True, seed=3, nhp=nhp)
    b["proc"].network = nhp.StochasticBlockNetworkModel(N, K, ρ=rng.uniform(0.2, 0.8, (K, K)), z=rng.integers(0, K, N))
    rb = nhp.mcmc_(b["proc"], b["data"], nsteps=12, seed=8, keep_samples=False, moments=True, diagnostics="full")
    k = K * K + K
    assert len(rb.diagnostics["ess"]) == len(rb.mean) and "network.ρ" not in rb.diagnostics["summary"]
    for name in ("ess", "mcse", "rhat"):
        assert np.all(np.isnan(rb.diagnostics[name][:k])) and np.isfinite(rb.diagnostics[name][k:]).any()
    lat = random_case(N, 2000, 150.0, "exponential", 1.0, network=True, seed=3, nhp=nhp)
    lat["proc"].network = nhp.LatentDistanceNetworkModel(N, 2, z=rng.standard_normal((N, 2)), b=0.4, σ=1.5, μb=0.2, σb=2.0)
    rl = nhp.mcmc_(lat["proc"], lat["data"], nsteps=12, seed=8, keep_samples=False, moments=True, diagnostics="full")
    assert len(rl.diagnostics["ess"]) == len(rl.mean) and "network.ρ" not in rl.diagnostics["summary"]
    for name in ("ess", "mcse", "rhat"):
        assert np.isnan(rl.diagnostics[name][0]) and np.isfinite(rl.diagnostics[name][1:]).any()
    assert rl.diagnostics["summary"]["adjacency"]["entries"] == N * N


def test_sharded_chains_and_bad_arguments_are_refused(nhp):
    from nhp_amd import _lib
    c = random_case(4, 500, 50.0, "exponential", 1.0, seed=2, nhp=nhp)
    ctx = nhp.default_context()
    model = c["proc"].device_model(ctx)
    lib = _lib.lib()
    with pytest.raises(_lib.NhpError, match="batch_len"):
        _lib.check(lib.nhp_cont_model_diagnostics_configure(ctx.h, model.h, 0, 10), ctx.h)
    configure(ctx, model, 2, 10)
    with pytest.raises(_lib.NhpError, match="nothing accumulated"):
        fetch(ctx, model, 4 + 32, 100.0, 1.01)
    # a column shard cannot be diagnosed: each rank would see its own columns' sums only
    from nhp_amd import inference
    t, n, T = c["data"]
    shard = C.c_void_p()
    _lib.check(lib.nhp_cont_dataset_create_columns(ctx.h, _lib.dptr(_lib.f64(t)), _lib.iptr(np.ascontiguousarray(n, dtype=np.int64)), len(t), 4,
                                                  float(T), 1.0, 0, 2, C.byref(shard)), ctx.h)
    try:
        pri = inference._priors(c["proc"])
        with pytest.raises(NotImplementedError, match="column shard"):
            _lib.check(lib.nhp_cont_mcmc_run(ctx.h, None, shard, model.h, C.byref(pri), 0.0, 0.0, 1, 0, 2, 0), ctx.h)
    finally:
        lib.nhp_cont_dataset_destroy(shard)
        configure(ctx, model, 0, 0)
