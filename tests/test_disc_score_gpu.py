"""The chain scorer on the device (nhp_disc_score_*, nhp_disc_model_attach_score, csrc/disc_score.hip) against the 50-digit
restatement of its definitions (tests/disc_score_ref.py), at the shapes where the pass can go wrong; the extremes; the
invariants on a real chain; identity between the routes; the refusals.

Bounds: the device may differ from the 50-digit value by 16 times what the plain numpy fp64 restatement differs by on the
same case and quantity, and not less than 1e-12 of Σ|ℓ| (a pointwise value: of that cell's own |ℓ_i|, cell by cell) -- disc_score_ref.tolerances.
Every figure is printed before it is asserted.

The 50-digit reference of the 130-node case (26 000 cells, seven draws) is the one costly piece, seconds per model; its
cell table is computed once per session and shared by that case's S = 1, 2 and 7."""
import ctypes as C
import math

import numpy as np
import pytest

import disc_score_ref as ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
#        N    T    B  L  bins         dt   rate
SHAPES = [(1, 5, 1, 2, None, 1.0, 0.8),                  # one node, one basis, five bins
          (3, 37, 2, 4, None, 0.5, 0.5),                 # everything ragged, dt off 1
          (17, 129, 5, 9, (5, 128), 1.0, 0.5),           # odd start, odd length: λ and the counts start 8 bytes off 16
          (130, 300, 2, 5, (100, 300), 1.0, 0.05),       # two column tiles of the GEMM
          (6, 1000, 8, 5, (999, 1000), 1.0, 0.3)]        # one row


def make_process(nhp, N, B, L, dt=1.0, network=False):
    th = np.zeros((N, N, B))
    th[:, :, 0] = 1.0
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), dt),
                                             nhp.DiscreteGaussianImpulseResponse(th, L, dt), nhp.DenseWeightModel(np.full((N, N), 0.1 / N)), dt)
    if network:
        proc = nhp.DiscreteNetworkHawkesProcess(proc.baseline, proc.impulses, proc.weights, np.ones((N, N)), nhp.BernoulliNetworkModel(0.5, N), dt)
    return proc


class Raw:
    """nhp_disc_model and nhp_disc_score driven entry by entry."""

    def __init__(self, nhp, N, B, network, dt=1.0):
        from nhp_amd import _lib
        self._lib, self.lib, self.ctx = _lib, _lib.lib(), nhp.default_context()
        self.N, self.network = N, network
        self.h = C.c_void_p()
        self.ok(self.lib.nhp_disc_model_create(self.ctx.h, N, B, int(network), dt, C.byref(self.h)))
        self.scores = []

    def ok(self, rc):
        self._lib.check(rc, self.ctx.h)

    def set(self, draw):
        l0, W, th, A = draw
        cm = self._lib.colmajor
        self.ok(self.lib.nhp_disc_model_set(self.ctx.h, self.h, self._lib.dptr(self._lib.f64(l0)), self._lib.dptr(cm(W)), self._lib.dptr(cm(th)),
                                            self._lib.dptr(cm(A))))

    def scorer(self, ds, t0, t1):
        s = C.c_void_p()
        self.ok(self.lib.nhp_disc_score_create(self.ctx.h, ds.h, t0, t1, C.byref(s)))
        self.scores.append(s)
        return s

    def accumulate(self, s):
        self.ok(self.lib.nhp_disc_score_accumulate(self.ctx.h, s, self.h))

    def fetch(self, s, R, pointwise=True):
        summary, per_node = np.empty(10), np.empty(3 * self.N)
        pw = np.empty(R * self.N) if pointwise else None
        self.ok(self.lib.nhp_disc_score_fetch(self.ctx.h, s, self._lib.dptr(summary), self._lib.dptr(per_node), self._lib.dptr(pw)))
        return dict(summary=dict(zip(ref.FIELDS, summary)), per_node=per_node.reshape(3, self.N),
                    pointwise=pw.reshape((R, self.N), order="F") if pointwise else None)

    def planes(self, s, R):
        out = [np.empty(R * self.N) for _ in range(3)]
        self.ok(self.lib.nhp_disc_score_fetch_planes(self.ctx.h, s, *[self._lib.dptr(v) for v in out]))
        return [v.reshape((R, self.N), order="F") for v in out]              # lse, mean, M2 of ℓ without its loggamma

    def close(self):
        for s in self.scores:
            self.lib.nhp_disc_score_destroy(s)
        self.scores = []
        if self.h:
            self.lib.nhp_disc_model_destroy(self.h)
            self.h = None


# ---- scripted draws against the reference ---------------------------------------------------------------------------------
REFERENCES = {}         # (shape, network) -> the case, its 50-digit cell table (shared by S = 1, 2, 7), {S: reference}


def scripted(nhp, shape, network, S):
    if (shape, network) not in REFERENCES:
        N, T, B, L, bins, dt, rate = shape
        phi = make_process(nhp, N, B, L, dt).impulses.basis()
        case = ref.make_case(N, T, B, L, bins, 7, network, seed=11 * N + T + network, rate=rate, dt=dt, phi=phi)
        REFERENCES[shape, network] = (case, ref.cells_mp(case), {})
    case, ells, done = REFERENCES[shape, network]
    if S not in done:
        done[S] = ref.score_mp_prefix(ells, S)
    return dict(case, draws=case["draws"][:S]), done[S]


def device_score(nhp, case, network):
    N, T = case["data"].shape
    L, B = case["phi"].shape
    t0, t1 = case["bins"]
    ds = nhp.convolve(make_process(nhp, N, B, L, case["dt"]), case["data"])
    m = Raw(nhp, N, B, network, case["dt"])
    try:
        s = m.scorer(ds, t0, t1)
        for draw in case["draws"]:
            m.set(draw)
            m.accumulate(s)
        return m.fetch(s, t1 - t0)
    finally:
        m.close()


def hold_to_reference(got, case, mpr, label):
    yard = ref.errors(ref.score_numpy(case), mpr)
    err, tol = ref.errors(got, mpr), ref.tolerances(yard, mpr)
    for k in err:
        bound = tol[k] if np.ndim(tol[k]) == 0 else tol[k].min()          # (pointwise: one bound per cell, the tightest shown)
        print(f"{label} {k}: device {err[k]:.3e}  numpy {yard[k]:.3e}  bound {bound:.3e}")
    for k in err:
        if np.ndim(tol[k]) == 0 and math.isnan(tol[k]):
            assert math.isnan(err[k]), (k, err[k])               # undefined in the reference: NaN on the device
        elif k == "pointwise":                                   # every cell against its own floor, 1e-12 of its own |ℓ_i|
            cells = ref.pointwise_errors(got, mpr)
            print(f"{label} pointwise: largest error / bound over the cells {np.max(cells / tol[k]):.3e}")
            assert np.all(cells <= tol[k]), (k, float(np.max(cells / tol[k])))
        else:
            assert err[k] <= tol[k], (k, err[k], tol[k])


@pytest.mark.parametrize("S", [1, 2, 7])
@pytest.mark.parametrize("network", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-T{s[1]}")
def test_scripted_draws_against_the_reference(nhp, shape, network, S):
    case, mpr = scripted(nhp, shape, network, S)
    got = device_score(nhp, case, network)
    assert got["summary"]["n"] == S and got["summary"]["cells"] == (case["bins"][1] - case["bins"][0]) * shape[0]
    hold_to_reference(got, case, mpr, f"N={shape[0]} T={shape[1]} network={network} S={S}")


# ---- extremes -------------------------------------------------------------------------------------------------------------------
def test_draws_a_factor_of_a_million_apart(nhp):
    """A cell with s = 40 whose λ differs by 2·10⁶ between two draws: ℓ differs by more than a thousand, exp(−|Δ|) underflows,
    and the log-sum-exp is the larger ℓ, finite."""
    N, T, B, L = 2, 30, 1, 2
    data = np.zeros((N, T), dtype=np.int64)
    data[0, 10], data[1, 3], data[1, 11] = 40, 2, 1
    th, W = np.ones((N, N, B)), np.full((N, N), 0.05)
    case = dict(data=data, phi=make_process(nhp, N, B, L).impulses.basis(), dt=1.0, bins=(0, T),
                draws=[(np.array([1e-3, 0.2]), W, th, None), (np.array([2e3, 0.2]), W, th, None)])
    got = device_score(nhp, case, False)
    ell = [ref.loglik_cells_numpy(case, d)[10, 0] for d in case["draws"]]
    assert abs(ell[0] - ell[1]) > 1000 and math.exp(-abs(ell[0] - ell[1])) == 0.0
    assert all(np.isfinite(v) for v in got["summary"].values()) and np.all(np.isfinite(got["pointwise"]))
    hold_to_reference(got, case, ref.score_mp(case)[2], "far apart")
    # on the device's own numbers: ℓ of each draw is the lse plane after that draw alone; after both, the plane at the
    # cell IS the larger of the two, bit for bit, and nowhere below it
    ds = nhp.convolve(make_process(nhp, N, B, L), data)
    m = Raw(nhp, N, B, False)
    try:
        both, second = m.scorer(ds, 0, T), m.scorer(ds, 0, T)
        m.set(case["draws"][0])
        m.accumulate(both)
        ell1 = m.planes(both, T)[0]
        m.set(case["draws"][1])
        m.accumulate(both)
        m.accumulate(second)
        ell2, (lse, mean, m2) = m.planes(second, T)[0], m.planes(both, T)
    finally:
        m.close()
    top = np.maximum(ell1, ell2)
    print(f"far apart: device ℓ at the cell {ell1[10, 0]!r}, {ell2[10, 0]!r}; lse {lse[10, 0]!r}")
    assert abs(ell1[10, 0] - ell2[10, 0]) > 1000 and lse[10, 0] == top[10, 0] and np.isfinite(lse).all()
    assert np.all(lse >= top) and np.all(lse <= top + math.log(2) + 4 * np.spacing(np.abs(top))) and np.all(m2 >= 0)


def test_empty_columns(nhp):
    """Nodes without a single event: ℓ = −λ, no logarithm taken."""
    case = ref.make_case(4, 70, 2, 3, (1, 70), 3, True, seed=2, rate=0.6, phi=make_process(nhp, 4, 2, 3).impulses.basis())
    case["data"][[0, 2], :] = 0
    got = device_score(nhp, case, True)
    assert np.all(np.isfinite(got["pointwise"])) and np.all(got["per_node"][0, [0, 2]] < 0)
    hold_to_reference(got, case, ref.score_mp(case)[3], "empty columns")


def test_one_draw_leaves_the_variance_undefined(nhp):
    case = ref.make_case(3, 40, 2, 4, None, 1, False, seed=1, phi=make_process(nhp, 3, 2, 4).impulses.basis())
    s = device_score(nhp, case, False)["summary"]
    for k in ("p_waic", "elpd_waic", "waic", "se_elpd", "joint_sd"):
        assert math.isnan(s[k]), k
    for k in ("lppd", "joint_lpd", "joint_mean"):
        assert math.isfinite(s[k]), k
    assert s["n"] == 1 and s["joint_lpd"] == s["joint_mean"]


def test_fetch_before_any_accumulate(nhp):
    from nhp_amd import _lib
    proc = make_process(nhp, 3, 2, 4)
    ds = nhp.convolve(proc, np.ones((3, 20), dtype=np.int64))
    m = Raw(nhp, 3, 2, False)
    try:
        s = m.scorer(ds, 0, 20)
        with pytest.raises(_lib.NhpError, match="nothing accumulated"):
            m.fetch(s, 20)
        m.set((np.full(3, 0.2), np.full((3, 3), 0.1), np.full((3, 3, 2), 0.5), None))
        m.accumulate(s)
        assert m.fetch(s, 20)["summary"]["n"] == 1
        m.ok(m.lib.nhp_disc_score_reset(m.ctx.h, s))
        with pytest.raises(_lib.NhpError, match="nothing accumulated"):
            m.fetch(s, 20)
    finally:
        m.close()


# ---- a real chain: invariants and routes ------------------------------------------------------------------------------------
def chain_case(nhp, N, T, B, L, network, seed):
    rng = np.random.default_rng(seed)
    data = rng.poisson(0.4, (N, T)).astype(np.int64)
    proc = make_process(nhp, N, B, L, network=network)
    proc.impulses.θ = np.full((N, N, B), 1.0 / B)
    if network:
        proc.adjacency_matrix = (rng.uniform(size=(N, N)) < 0.5).astype(np.float64)
        proc.weights.W = proc.weights.W * N * 1.5
    return proc, data


def same_score(a, b):
    for k in ref.FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), (k, getattr(a, k), getattr(b, k))
    assert np.array_equal(a.per_node, b.per_node, equal_nan=True) and a.bins == b.bins
    assert (a.pointwise is None) == (b.pointwise is None)
    if a.pointwise is not None:
        assert np.array_equal(a.pointwise, b.pointwise, equal_nan=True)


def split_sample(proc, x, network):
    from nhp_amd import discrete
    N, B = proc.ndims(), proc.impulses.nbasis()
    l0, W, th, A = discrete._sample_arrays(proc, x)
    return (l0, W.reshape((N, N), order="F"), th.reshape((N, N, B), order="F"), A.reshape((N, N), order="F") if network else None)


@pytest.mark.parametrize("network", [False, True])
def test_invariants_on_a_real_chain(nhp, network):
    """Jensen's inequality per cell and for the joint score, p >= 0, and the nodes add up to the summary -- on what the device
    holds and nothing else: the draws of a real chain are set into a model one by one, and the lse and mean planes
    (nhp_disc_score_fetch_planes; both without the cell's loggamma, which cancels) must satisfy lse_i − log S >= mean_i within
    4 ulp of |ℓ_i|, M2_i >= 0 exactly.  The scorer fed this way is the chain's own, bit for bit."""
    N, T, B, L = 5, 257, 2, 4
    proc, data = chain_case(nhp, N, T, B, L, network, seed=7)
    res = nhp.mcmc_(proc, data, nsteps=10, burn=2, seed=5, keep_samples=True, moments=True, waic=True, pointwise=True)
    w = res.waic
    assert w.n == 8 and w.cells == N * T and w.bins == (0, T) and w.pointwise.shape == (T, N)
    ds = nhp.convolve(proc, data)
    m = Raw(nhp, N, B, network)
    try:
        s = m.scorer(ds, 0, T)
        for x in res.samples[2:]:
            m.set(split_sample(proc, x, network))
            m.accumulate(s)
        got, (lse, mean, m2) = m.fetch(s, T), m.planes(s, T)
    finally:
        m.close()
    assert np.array_equal(got["pointwise"], w.pointwise) and got["summary"]["lppd"] == w.lppd and got["summary"]["p_waic"] == w.p_waic
    gap, ulp = (lse - math.log(8)) - mean, np.spacing(np.abs(mean))
    print(f"network={network}: min over the cells of (lse_i − log S − mean_i) = {gap.min():.3e} = {np.min(gap / ulp):.3e} ulp of |ℓ_i|, "
          f"min M2_i = {m2.min():.3e}, joint_lpd − joint_mean = {w.joint_lpd - w.joint_mean:.3e}, min per-node p = {w.per_node[1].min():.3e}")
    assert np.all(gap >= -4 * ulp)
    assert np.all(m2 >= 0) and np.all(w.per_node[1] >= 0) and w.p_waic >= 0
    lg = np.vectorize(lambda v: math.lgamma(v + 1.0))(data.T.astype(np.float64))
    assert np.all(w.pointwise <= (lse - math.log(8)) - lg + 4 * np.spacing(np.abs(lse) + lg))           # elpd_i <= lppd_i: p_i >= 0
    assert w.joint_lpd >= w.joint_mean and w.joint_sd >= 0 and w.se_elpd >= 0
    for k, name in enumerate(("lppd", "p_waic", "elpd_waic")):
        assert abs(w.per_node[k].sum() - getattr(w, name)) <= N * EPS * np.abs(w.per_node[k]).sum(), name
    assert w.waic == -2.0 * w.elpd_waic and abs(w.elpd_waic - (w.lppd - w.p_waic)) <= 4 * EPS * abs(w.lppd)
    assert abs(w.pointwise.sum() - w.elpd_waic) <= N * T * EPS * np.abs(w.pointwise).sum()


@pytest.mark.parametrize("N,T,B,L,network", [(5, 257, 2, 4, True), (17, 129, 5, 9, False)])
def test_routes_and_repeats(nhp, N, T, B, L, network):
    """12 steps, burn 3, every second kept step: the resident chain in one nhp_disc_mcmc_run, cut into three calls, step by
    step with its samples, disc_score_samples on those samples -- and for the standard process the default route -- give the
    same bits, twice; the default route's scores are those of disc_score_samples on its own samples for both models; nothing attached leaves the chain's sums alone; two scorers do not disturb each other."""
    t0 = (3 * T) // 4
    kw = dict(nsteps=12, burn=3, seed=6, score_every=2, pointwise=True)

    def chain(**more):
        proc, full = chain_case(nhp, N, T, B, L, network, seed=21)
        held = (full, (t0, T))
        args = dict(kw, waic=True, heldout=held)
        args.update(more)
        return nhp.mcmc_(proc, full[:, :t0], **args), proc, full

    one, p_one, full = chain(keep_samples=False)
    assert one.waic.n == 5 and one.heldout.n == 5                              # kept steps 3..11, every second: 3, 5, 7, 9, 11
    assert one.waic.bins == (0, t0) and one.heldout.bins == (t0, T) and one.heldout.cells == (T - t0) * N
    assert np.isfinite(one.waic.waic) and np.isfinite(one.heldout.joint_lpd) and one.waic.p_waic > 0
    cut, p_cut, _ = chain(keep_samples=False, verbose=True, log_freq=4)        # three calls of nhp_disc_mcmc_run
    again, _, _ = chain(keep_samples=False)
    steps, p_steps, _ = chain(keep_samples=True, moments=True)
    for other in (cut, again, steps):
        same_score(other.waic, one.waic)
        same_score(other.heldout, one.heldout)
    assert np.array_equal(p_cut.params(), p_one.params()) and np.array_equal(p_steps.params(), p_one.params())
    fresh = chain_case(nhp, N, T, B, L, network, seed=21)[0]
    same_score(nhp.disc_score_samples(fresh, steps.samples, full[:, :t0], burn=3, every=2, pointwise=True), one.waic)
    same_score(nhp.disc_score_samples(fresh, steps.samples, full, bins=(t0, T), burn=3, every=2, pointwise=True), one.heldout)
    # the default route (every step through the host; the scored step's state pushed into a scoring-only device model).  Its
    # scores are those of its own samples, bit for bit, whatever the model; for the standard process its chain is the resident
    # one as well (a Bernoulli network's ρ is drawn by numpy there: another chain)
    default, p_def, _ = chain()
    assert default.waic.n == 5 and default.heldout.n == 5 and len(default.samples) == 12
    same_score(nhp.disc_score_samples(fresh, default.samples, full[:, :t0], burn=3, every=2, pointwise=True), default.waic)
    same_score(nhp.disc_score_samples(fresh, default.samples, full, bins=(t0, T), burn=3, every=2, pointwise=True), default.heldout)
    if not network:
        assert np.array_equal(p_def.params(), p_one.params())
        same_score(default.waic, one.waic)
        same_score(default.heldout, one.heldout)
    # one scorer at a time: the same bits as with its neighbour attached
    same_score(chain(keep_samples=False, heldout=None)[0].waic, one.waic)
    same_score(chain(keep_samples=False, waic=False)[0].heldout, one.heldout)
    # nothing attached: the chain and its sums are what they are with scorers
    scored, p_s, _ = chain(keep_samples=False, moments=True)
    plain, p_p, _ = chain(keep_samples=False, moments=True, waic=False, heldout=None)
    assert not hasattr(plain, "waic") and not hasattr(plain, "heldout")
    assert np.array_equal(plain.mean, scored.mean) and np.array_equal(plain.m2, scored.m2) and plain.n == scored.n == 9
    assert np.array_equal(p_p.params(), p_s.params()) and np.array_equal(p_p.params(), p_one.params())
    same_score(scored.waic, one.waic)


# ---- refusals at the C ABI ------------------------------------------------------------------------------------------------------
def test_refusals_at_the_c_abi(nhp):
    from nhp_amd import _lib
    proc = make_process(nhp, 3, 2, 4)
    data = np.random.default_rng(0).poisson(0.5, (3, 50)).astype(np.int64)
    ds = nhp.convolve(proc, data)
    m = Raw(nhp, 3, 2, False)
    try:
        for t0, t1 in ((-1, 10), (10, 10), (20, 10), (0, 51), (50, 51)):
            with pytest.raises(_lib.NhpError, match="0 <= t0 < t1 <= T"):
                m.scorer(ds, t0, t1)
        with pytest.raises(_lib.NhpError, match="convolve"):
            m.scorer(nhp.DiscreteDataset(m.ctx, data), 0, 50)
        lg = nhp.convolve(proc, data)
        grid = np.linspace(0.0, 51.0, 6)
        m.ok(m.lib.nhp_disc_set_lgcp_baseline(m.ctx.h, lg.h, _lib.dptr(grid), 6, _lib.dptr(np.ones(18)), 1.0))
        with pytest.raises(NotImplementedError, match="LGCP"):
            m.scorer(lg, 0, 50)
        s = m.scorer(ds, 0, 50)
        for N, B in ((4, 2), (3, 3)):                                      # a model whose N or B is not the dataset's
            other = Raw(nhp, N, B, False)
            try:
                with pytest.raises(_lib.NhpError, match="does not match the dataset"):
                    other.accumulate(s)
                with pytest.raises(_lib.NhpError, match="does not match the dataset"):
                    other.ok(other.lib.nhp_disc_model_attach_score(other.ctx.h, other.h, s, 1))
            finally:
                other.close()
        with pytest.raises(_lib.NhpError, match="every must be >= 1"):
            m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, s, 0))
        s2, s3 = m.scorer(ds, 10, 20), m.scorer(ds, 49, 50)
        m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, s, 1))
        m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, s2, 3))
        m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, s, 2))           # again: its rhythm changes, no third slot taken
        with pytest.raises(_lib.NhpError, match="at most two"):
            m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, s3, 1))
        m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, None, 1))         # detach: room again
        m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, s3, 1))
        m.ok(m.lib.nhp_disc_model_attach_score(m.ctx.h, m.h, None, 1))
    finally:
        m.close()
