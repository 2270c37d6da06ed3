"""The stochastic block network model on the GPU (csrc/sbm.hip) against the numpy restatement in tests/sbm_ref.py: the
label sweep's conditionals and decisions node by node, the block counts, the sweep's own uniform stream, the ρ and π
draws, a planted partition, and the model inside the continuous and the discrete chains."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import sbm_ref as sr
from helpers import random_case

pytestmark = pytest.mark.gpu

P_MIN = 1e-4          # the threshold of tests/test_device_draws_gpu.py


def lib_ctx(nhp):
    from nhp_amd import _lib
    return _lib, _lib.lib(), nhp.default_context()


def gpu_sweep(nhp, A, z, rho, pi, u=None, seed=0, step=0, n_sweeps=1, want_probs=True):
    """nhp_sbm_resample_blocks -> (labels, u_used, probs [steps, K])."""
    _lib, lib, ctx = lib_ctx(nhp)
    N, K = len(z), len(pi)
    Af = _lib.colmajor(A)
    zz = np.ascontiguousarray(z, dtype=np.int32).copy()
    rf, pf = _lib.colmajor(rho), _lib.f64(pi)
    uu = None if u is None else _lib.f64(u)
    used = np.empty(n_sweeps * N)
    probs = np.empty(n_sweeps * N * K) if want_probs else None
    _lib.check(lib.nhp_sbm_resample_blocks(ctx.h, _lib.dptr(Af), N, K, zz.ctypes.data, _lib.dptr(rf), _lib.dptr(pf), _lib.dptr(uu), seed, step,
                                           n_sweeps, _lib.dptr(used), _lib.dptr(probs)), ctx.h)
    return zz, used, None if probs is None else probs.reshape((n_sweeps * N, K))


def check_replay(case, z_new_by_sweep, probs, used):
    """Every step of the device's sweeps against the reference at the state the device was in: probs to 1e-10, decisions
    equal except where the reference's margin is below 1e-9 (at most 1 % of the nodes)."""
    N = case["N"]
    assert np.array_equal(used, case["u"])
    z_old = case["z0"].astype(np.int64)
    excused = total = 0
    for s, z_new in enumerate(z_new_by_sweep):
        want_p, want_z, margins = sr.replay(case["A"], z_old, z_new, case["rho"], case["pi"], case["u"][s * N:(s + 1) * N])
        got_p = probs[s * N:(s + 1) * N]
        err = np.max(np.abs(got_p - want_p))
        print(f"sweep {s}: max |probs - reference| = {err:.3e}, moved {int(np.sum(z_new != z_old))} of {N}")
        assert err <= 1e-10, err
        differ = z_new != want_z
        assert not np.any(differ & (margins >= 1e-9)), np.nonzero(differ & (margins >= 1e-9))
        excused += int(np.sum(margins < 1e-9)); total += N
        z_old = z_new.astype(np.int64)
    assert excused <= 0.01 * total


# ---- 1. conditionals and decisions, node by node ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.decision_cases()))
def test_conditionals_and_decisions_node_by_node(nhp, name):
    c = sr.decision_cases()[name]
    z, used, probs = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], u=c["u"])
    assert z.min() >= 0 and z.max() < c["K"]
    check_replay(c, [z], probs, used)


# ---- 2. stale tables: three sweeps in one call, most nodes move ----------------------------------------------------------
def test_three_sweeps_in_one_call_keep_their_tables_current(nhp):
    c = sr.stale_case()
    N = c["N"]
    z3, used, probs = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], u=c["u"], n_sweeps=3)
    # the labels after the first and the second sweep: the same call cut short (same uniforms, same arithmetic)
    z1, _, _ = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], u=c["u"][:N], n_sweeps=1)
    z2, _, _ = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], u=c["u"][:2 * N], n_sweeps=2)
    assert np.mean(z1 != c["z0"]) > 0.5
    check_replay(c, [z1, z2, z3], probs, used)


# ---- 3. counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.decision_cases()))
def test_block_counts_are_exact(nhp, name):
    c = sr.decision_cases()[name]
    net = nhp.StochasticBlockNetworkModel(c["N"], c["K"], z=c["z0"])
    L, n = net.block_counts(c["A"])
    wantL, wantn = sr.counts(c["A"], c["z0"], c["K"])
    assert np.array_equal(L, wantL) and np.array_equal(n, wantn)


# ---- 4. the sweep's own stream --------------------------------------------------------------------------------------------
def test_own_uniform_stream(nhp):
    c = sr.decision_cases()["65x5"]
    za, ua, _ = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], seed=11, step=3)
    zb, ub, _ = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], seed=11, step=3)
    zc, uc, _ = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], seed=11, step=4)
    assert np.array_equal(za, zb) and np.array_equal(ua, ub)
    assert not np.array_equal(ua, uc) and np.all((ua >= 0) & (ua < 1))
    assert abs(ua.mean() - 0.5) < 0.2
    zd, ud, _ = gpu_sweep(nhp, c["A"], c["z0"], c["rho"], c["pi"], u=ua)
    assert np.array_equal(zd, za) and np.array_equal(ud, ua)
    # not the parent sampler's stream, nor the adjacency sweeps'
    _lib = lib_ctx(nhp)[0]
    for key in (0, 0xBE5466CF34E90C6C, 0xAD7AC3117D15C0DE):
        other = np.empty(len(ua))
        _lib.lib().nhp_uniform_stream(11 ^ key, 3, len(ua), _lib.dptr(other))
        assert not np.any(other == ua)


# ---- 5. draws ---------------------------------------------------------------------------------------------------------------
def test_rho_and_pi_draws_follow_their_posteriors(nhp):
    _lib, lib, ctx = lib_ctx(nhp)
    K, alpha, beta, gamma = 3, 2.0, 1.5, 0.7
    sizes = np.array([12, 0, 30], dtype=np.int64)                       # block 1 is empty: its pairs draw from the prior
    L = np.array([[40, 0, 100], [0, 0, 0], [7, 0, 893]], dtype=np.int64)
    Lf = np.ascontiguousarray(L.ravel(order="F"))
    steps = 2000
    rho, pi = np.empty((steps, K * K)), np.empty((steps, K))
    r, p = np.empty(K * K), np.empty(K)
    for s in range(steps):
        _lib.check(lib.nhp_sbm_draw(ctx.h, K, Lf.ctypes.data, sizes.ctypes.data, alpha, beta, gamma, 5, s, _lib.dptr(r), _lib.dptr(p)), ctx.h)
        rho[s], pi[s] = r, p
    assert np.all((rho > 0) & (rho < 1)) and np.all(pi > 0)
    for k, l in ((0, 0), (2, 0), (1, 2)):
        a, b = alpha + L[k, l], beta + sizes[k] * sizes[l] - L[k, l]
        if (k, l) == (1, 2):
            assert (a, b) == (alpha, beta)
        pv = stats.kstest(stats.beta.cdf(rho[:, k + K * l], a, b), "uniform").pvalue
        print(f"rho[{k},{l}] ~ Beta({a}, {b}): KS p = {pv:.3g}")
        assert pv > P_MIN
    g = gamma + sizes
    pv = stats.kstest(stats.beta.cdf(pi[:, 2], g[2], g.sum() - g[2]), "uniform").pvalue
    print(f"pi[2] ~ Beta({g[2]}, {g.sum() - g[2]}): KS p = {pv:.3g}")
    assert pv > P_MIN
    import math
    worst = max(abs(math.fsum(row) - 1.0) for row in pi)
    assert worst <= K * 2.0 ** -52, worst
    # and at the largest K
    K = 64
    sizes = np.arange(K, dtype=np.int64)
    Lf = np.zeros(K * K, dtype=np.int64)
    r, p = np.empty(K * K), np.empty(K)
    _lib.check(lib.nhp_sbm_draw(ctx.h, K, Lf.ctypes.data, sizes.ctypes.data, 1.0, 1.0, 1.0, 5, 0, _lib.dptr(r), _lib.dptr(p)), ctx.h)
    assert abs(math.fsum(p) - 1.0) <= K * 2.0 ** -52 and np.all((r > 0) & (r < 1))


# ---- 6. recovery, identical to the reference chain -----------------------------------------------------------------------------
def test_planted_partition_chain_equals_the_reference(nhp):
    c = sr.planted_case()
    z_ref = c["z0"].astype(np.int64)
    z_dev = c["z0"].copy()
    for it in range(sr.RECOVERY_ITERS):
        rho, pi, u = sr.recovery_draws(c, z_ref, c["rng"])
        z_ref, _, margins = sr.sweep(c["A"], z_ref, rho, pi, u)
        assert margins.min() > 1e-9
        z_dev, _, _ = gpu_sweep(nhp, c["A"], z_dev, rho, pi, u=u, want_probs=False)
        assert np.array_equal(z_dev, z_ref), it
    assert sr.same_partition(z_ref, c["truth"])


# ---- 7. K = 1 is Bernoulli ------------------------------------------------------------------------------------------------------
def test_one_block_sweeps_the_adjacency_matrix_like_the_bernoulli_model(nhp):
    def swept(network):
        c = random_case(9, 1500, 120.0, "exponential", 1.0, network=True, seed=5, nhp=nhp)
        c["proc"].network = network
        nhp.invalidate_device_datasets()
        links = nhp.resample_adjacency_matrix_(c["proc"], c["data"], seed=21, step=6)
        return c["proc"].adjacency_matrix.copy(), links
    A1, l1 = swept(nhp.StochasticBlockNetworkModel(9, 1, ρ=[[0.3]]))
    A2, l2 = swept(nhp.BernoulliNetworkModel(0.3, 9))
    assert np.array_equal(A1, A2) and l1 == l2 and 0 < l1 < 81


# ---- 8. chain routes agree ----------------------------------------------------------------------------------------------------------
def block_process(nhp, N=12, M=2000, K=2, seed=3):
    c = random_case(N, M, 150.0, "exponential", 1.0, network=True, seed=seed, nhp=nhp)
    rng = np.random.default_rng(seed)
    c["proc"].network = nhp.StochasticBlockNetworkModel(N, K, ρ=rng.uniform(0.2, 0.8, (K, K)), z=rng.integers(0, K, N))
    return c


def test_chain_routes_agree(nhp):
    N, K, steps = 12, 2, 20
    a = block_process(nhp)
    ra = nhp.mcmc_(a["proc"], a["data"], nsteps=steps, seed=8, keep_samples=False, moments=True)
    b = block_process(nhp)
    rb = nhp.mcmc_(b["proc"], b["data"], nsteps=steps, seed=8, keep_samples=True, moments=True)
    na, nb = a["proc"].network, b["proc"].network
    assert np.array_equal(a["proc"].adjacency_matrix, b["proc"].adjacency_matrix)
    assert np.array_equal(na.z, nb.z) and np.array_equal(na.ρ, nb.ρ) and np.array_equal(na.π, nb.π)
    assert np.array_equal(a["proc"].params(), b["proc"].params())
    nk = K * K + K
    samples = np.array(rb.samples)
    assert samples.shape == (steps, len(a["proc"].params()))
    for r in (ra, rb):
        assert r.n == steps
        assert np.max(np.abs(r.mean[:nk] - samples[:, :nk].mean(axis=0))) <= 1e-12
        assert np.max(np.abs(r.m2[:nk] - (samples[:, :nk] ** 2).mean(axis=0))) <= 1e-12
        assert r.block_counts.shape == (N, K) and np.all(r.block_counts.sum(axis=1) == steps)
    assert np.array_equal(ra.block_counts, rb.block_counts)
    assert np.allclose(ra.mean, rb.mean, rtol=0, atol=1e-12)
    # the host-draw route: A comes back every step, the network is resampled through the stand-alone entries
    h = block_process(nhp)
    rh = nhp.mcmc_(h["proc"], h["data"], nsteps=5, seed=8, device_draws=False)
    nh = h["proc"].network
    assert rh.steps == 5 and len(rh.samples) == 5
    assert nh.z.shape == (N,) and nh.z.min() >= 0 and nh.z.max() < K
    assert np.all((nh.ρ > 0) & (nh.ρ < 1)) and abs(nh.π.sum() - 1.0) < 1e-12 and np.all(nh.π > 0)
    assert set(np.unique(h["proc"].adjacency_matrix)) <= {0.0, 1.0}
    assert np.array_equal(rh.samples[-1][:nk], nh.params())


def test_device_step_equals_the_stand_alone_entries(nhp):
    """One device-resident network step (link probabilities, adjacency sweep, counts, draws, labels -- nothing leaves the
    device) against the same step made of the host-visible pieces: resample_adjacency_matrix_ on link_probability(), then
    the component's resample_ through the stand-alone entries, all keyed by the same (seed, step)."""
    _lib, lib, ctx = lib_ctx(nhp)
    N, K, seed, step = 12, 2, 13, 5
    a = block_process(nhp)
    proc, net = a["proc"], a["proc"].network
    ds, model = nhp.device_dataset(proc, a["data"], ctx), proc.device_model(ctx)
    z = np.ascontiguousarray(net.z, dtype=np.int32)
    _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, model.h, K, z.ctypes.data, _lib.dptr(_lib.colmajor(net.ρ)), _lib.dptr(_lib.f64(net.π)),
                                          net.α, net.β, net.γ), ctx.h)
    _lib.check(lib.nhp_cont_sbm_step(ctx.h, ds.h, model.h, seed, step), ctx.h)
    zd, rd, pd, Ad = np.empty(N, dtype=np.int32), np.empty(K * K), np.empty(K), np.empty(N * N)
    _lib.check(lib.nhp_cont_model_get_sbm(ctx.h, model.h, zd.ctypes.data, _lib.dptr(rd), _lib.dptr(pd), None, None), ctx.h)
    _lib.check(lib.nhp_cont_model_get_adjacency(ctx.h, model.h, _lib.dptr(Ad), N * N), ctx.h)
    b = block_process(nhp)
    links = nhp.resample_adjacency_matrix_(b["proc"], b["data"], seed=seed, step=step)
    assert 0 < links < N * N
    b["proc"].network.resample_(b["proc"].adjacency_matrix, None, seed=seed, step=step)
    assert np.array_equal(Ad.reshape((N, N), order="F"), b["proc"].adjacency_matrix)
    assert np.array_equal(rd.reshape((K, K), order="F"), b["proc"].network.ρ) and np.array_equal(pd, b["proc"].network.π)
    assert np.array_equal(zd, b["proc"].network.z)


@pytest.mark.parametrize("kind", ["bernoulli", "dense"])
def test_a_bernoulli_or_dense_chain_after_a_block_chain_is_the_chain_of_a_fresh_process(nhp, kind):
    """The device model is cached on the process and carries the block state; swapping process.network for another kind
    must detach it (nhp_cont_model_set_rho does), or the resident route would go on sampling the block model."""
    def network():
        return nhp.BernoulliNetworkModel(0.4, 12, 2.0, 3.0) if kind == "bernoulli" else nhp.DenseNetworkModel(12)

    def state(p, r):
        rho = p.network.ρ if kind == "bernoulli" else 1.0
        return p.params(), p.adjacency_matrix, rho, r.mean, r.m2

    used = block_process(nhp)
    nhp.mcmc_(used["proc"], used["data"], nsteps=3, seed=8, keep_samples=False, moments=True)
    model = used["proc"]._dev
    fresh = block_process(nhp)
    # the same starting state for both: the fresh process's
    for name in ("baseline", "impulses", "weights"):
        setattr(used["proc"], name, getattr(block_process(nhp)["proc"], name))
    used["proc"].adjacency_matrix = fresh["proc"].adjacency_matrix.copy()
    used["proc"].network, fresh["proc"].network = network(), network()
    ru = nhp.mcmc_(used["proc"], used["data"], nsteps=6, seed=9, keep_samples=False, moments=True)
    assert used["proc"]._dev is model                                # the cached device model was reused
    rf = nhp.mcmc_(fresh["proc"], fresh["data"], nsteps=6, seed=9, keep_samples=False, moments=True)
    for a, b in zip(state(used["proc"], ru), state(fresh["proc"], rf)):
        assert np.array_equal(a, b)
    # ... and the stepwise route on the used process agrees with its resident route
    again = block_process(nhp)
    again["proc"].network = network()
    rs = nhp.mcmc_(again["proc"], again["data"], nsteps=6, seed=9, keep_samples=True, moments=True)
    for a, b in zip(state(again["proc"], rs), state(fresh["proc"], rf)):
        assert np.array_equal(a, b)
    if kind == "bernoulli":
        assert used["proc"].network.ρ != 0.4                         # ρ was drawn
    # the block state is gone from the model
    _lib, lib, ctx = lib_ctx(nhp)
    with pytest.raises(_lib.NhpError, match="no block network"):
        _lib.check(lib.nhp_cont_model_get_sbm(ctx.h, model.h, None, None, None, None, None), ctx.h)


def test_labels_every_keeps_the_labels_between_sweeps(nhp):
    a = block_process(nhp)
    z0 = a["proc"].network.z.copy()
    nhp.mcmc_(a["proc"], a["data"], nsteps=3, seed=8, keep_samples=False, labels_every=1000)       # step 0 only
    b = block_process(nhp)
    nhp.mcmc_(b["proc"], b["data"], nsteps=1, seed=8, keep_samples=False)
    assert np.array_equal(a["proc"].network.z, b["proc"].network.z)
    assert not np.array_equal(a["proc"].network.ρ, b["proc"].network.ρ)
    assert z0.shape == a["proc"].network.z.shape


# ---- 9. discrete ------------------------------------------------------------------------------------------------------------------------
def test_discrete_chain_with_the_block_model(nhp):
    def run():
        N, T, K, B = 8, 500, 2, 3
        rng = np.random.default_rng(2)
        data = rng.poisson(0.3, (N, T)).astype(np.int64)
        net = nhp.StochasticBlockNetworkModel(N, K, ρ=[[0.6, 0.2], [0.3, 0.7]], z=rng.integers(0, K, N))
        proc = nhp.DiscreteNetworkHawkesProcess(
            nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), 1.0), nhp.DiscreteGaussianImpulseResponse(np.full((N, N, B), 1.0 / B), 6, 1.0),
            nhp.DenseWeightModel(np.full((N, N), 0.05)), (rng.uniform(size=(N, N)) < 0.5).astype(np.float64), net, 1.0)
        res = nhp.mcmc_(proc, data, nsteps=5, seed=4)                 # (dispatches to disc_mcmc_)
        return proc, res
    p1, r1 = run()
    p2, r2 = run()
    assert r1.steps == 5
    assert p1.network.z.min() >= 0 and p1.network.z.max() < 2 and p1.network.z.shape == (8,)
    assert np.array_equal(p1.network.z, p2.network.z) and np.array_equal(p1.network.ρ, p2.network.ρ)
    assert np.array_equal(p1.adjacency_matrix, p2.adjacency_matrix) and np.array_equal(p1.params(), p2.params())


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(nhp):
    _lib, lib, ctx = lib_ctx(nhp)
    c = sr.decision_cases()["2x2"]
    A, z, rho, pi = c["A"], c["z0"], c["rho"], c["pi"]

    def blocks(K=2, z=z, rho=rho, pi=pi, N=2, A=A):
        zz = np.ascontiguousarray(z, dtype=np.int32).copy()
        _lib.check(lib.nhp_sbm_resample_blocks(ctx.h, _lib.dptr(_lib.colmajor(A)), N, K, zz.ctypes.data, _lib.dptr(_lib.colmajor(rho)),
                                               _lib.dptr(_lib.f64(pi)), None, 0, 0, 1, None, None), ctx.h)

    blocks()
    with pytest.raises(_lib.NhpError, match="must lie in 1..64"):
        blocks(K=0)
    with pytest.raises(_lib.NhpError, match="must lie in 1..64"):
        blocks(K=65)
    with pytest.raises(nhp.DomainError, match="label"):
        blocks(z=[0, 2])
    with pytest.raises(nhp.DomainError, match="label"):
        blocks(z=[-1, 0])
    for bad in (0.0, 1.0, -0.1, np.nan):
        with pytest.raises(nhp.DomainError, match="open interval"):
            blocks(rho=np.array([[0.5, bad], [0.5, 0.5]]))
    with pytest.raises(nhp.DomainError, match="positive"):
        blocks(pi=np.array([0.0, 1.0]))
    with pytest.raises(nhp.DomainError, match="sums to"):
        blocks(pi=np.array([0.5, 0.5 + 1e-9]))
    # the priors
    L, n, r, p = np.zeros(4, dtype=np.int64), np.array([1, 1], dtype=np.int64), np.empty(4), np.empty(2)
    for pri in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, 0.0)):
        with pytest.raises(nhp.DomainError, match="alpha, beta, gamma > 0"):
            _lib.check(lib.nhp_sbm_draw(ctx.h, 2, L.ctypes.data, n.ctypes.data, *pri, 0, 0, _lib.dptr(r), _lib.dptr(p)), ctx.h)
    # above the LDS tables: refused with the reason, no fallback
    N = 2600                                                            # 8·N·K = 162.5 KiB
    with pytest.raises(NotImplementedError, match="LDS tables"):
        blocks(K=8, N=N, A=np.zeros((N, N)), z=np.zeros(N, dtype=np.int32), rho=np.full((8, 8), 0.5), pi=np.full(8, 0.125))
    # (189, 64) is the largest N at K = 64 (tests/sbm_ref.py sweeps it); one more node is refused
    with pytest.raises(NotImplementedError, match="LDS tables"):
        blocks(K=64, N=190, A=np.zeros((190, 190)), z=np.zeros(190, dtype=np.int32), rho=np.full((64, 64), 0.5), pi=np.full(64, 1.0 / 64))
    # the device-resident state: same checks, and a column shard is refused
    cc = block_process(nhp)
    proc = cc["proc"]
    model = proc.device_model(ctx)
    net = proc.network

    def set_sbm(K=2, z=net.z, rho=net.ρ, pi=net.π, pri=(1.0, 1.0, 1.0)):
        zz = np.ascontiguousarray(z, dtype=np.int32)
        _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, model.h, K, zz.ctypes.data, _lib.dptr(_lib.colmajor(rho)), _lib.dptr(_lib.f64(pi)), *pri),
                   ctx.h)

    with pytest.raises(_lib.NhpError, match="no block network"):
        _lib.check(lib.nhp_cont_sbm_step(ctx.h, nhp.device_dataset(proc, cc["data"], ctx).h, model.h, 0, 0), ctx.h)
    with pytest.raises(_lib.NhpError, match="must lie in 1..64"):
        set_sbm(K=65)
    with pytest.raises(nhp.DomainError, match="label"):
        set_sbm(z=np.full(12, 2))
    with pytest.raises(nhp.DomainError, match="open interval"):
        set_sbm(rho=np.ones((2, 2)))
    with pytest.raises(nhp.DomainError, match="sums to"):
        set_sbm(pi=np.array([0.5, 0.4]))
    with pytest.raises(nhp.DomainError, match="alpha, beta, gamma > 0"):
        set_sbm(pri=(1.0, 0.0, 1.0))
    set_sbm()
    times, nodes, T = cc["data"]
    h = C.c_void_p()
    _lib.check(lib.nhp_cont_dataset_create_columns(ctx.h, _lib.dptr(_lib.f64(times)), _lib.iptr(np.ascontiguousarray(nodes, dtype=np.int64)),
                                                   len(times), 12, T, 1.0, 0, 6, C.byref(h)), ctx.h)
    try:
        with pytest.raises(NotImplementedError, match="column shard"):
            _lib.check(lib.nhp_cont_sbm_step(ctx.h, h, model.h, 0, 0), ctx.h)
    finally:
        lib.nhp_cont_dataset_destroy(h)
    from nhp_amd.sharded import ShardedDataset
    shard = ShardedDataset.__new__(ShardedDataset)
    with pytest.raises(NotImplementedError, match="not sharded"):
        nhp.mcmc_(proc, shard, nsteps=1, keep_samples=False)
