"""The latent distance network model on the GPU (csrc/latent.hip) against the numpy restatement in tests/latent_ref.py:
every slice step of a sweep replayed at the state the device was in, the fallback batches and exhaustion with steered
streams, the kernel's own stream, the exact posterior at N = 2, two planted clusters, and the model inside the
continuous and the discrete chains."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import latent_ref as lr
from helpers import random_case

pytestmark = pytest.mark.gpu

P_MIN = lr.P_MIN


def lib_ctx(nhp):
    from nhp_amd import _lib
    return _lib, _lib.lib(), nhp.default_context()


def gpu_resample(nhp, case, z=None, b=None, draws="case", seed=0, step=0, n_sweeps=None, do_offset=True, trace=True):
    """nhp_latent_resample -> dict(z, b, draws, attempts [sweeps, N+1], trace [sweeps, N+1, 101], exhausted)."""
    _lib, lib, ctx = lib_ctx(nhp)
    N, D = case["N"], case["D"]
    n_sweeps = case["n_sweeps"] if n_sweeps is None else n_sweeps
    sweeps = max(1, n_sweeps)
    steps = N + 1 if n_sweeps else 1
    rs = N * (D + 101) + 102 if n_sweeps else 102
    zz = _lib.colmajor(case["z0"] if z is None else z).copy()
    bb, ex = C.c_double(case["b0"] if b is None else b), C.c_int64(-1)
    dd = _lib.f64(case["draws"][:sweeps * rs]) if isinstance(draws, str) else (None if draws is None else _lib.f64(draws))
    used, att = np.empty(sweeps * rs), np.full(sweeps * steps, -1, dtype=np.int32)
    tr = np.full(sweeps * steps * 101, np.nan) if trace else None
    _lib.check(lib.nhp_latent_resample(ctx.h, _lib.dptr(_lib.colmajor(case["A"])), N, D, _lib.dptr(zz), C.byref(bb), case["sigma"], case["mu_b"],
                                       case["sigma_b"], _lib.dptr(dd), seed, step, n_sweeps, 1 if do_offset else 0, _lib.dptr(used),
                                       att.ctypes.data, _lib.dptr(tr), C.byref(ex)), ctx.h)
    return {"z": zz.reshape((N, D), order="F"), "b": bb.value, "draws": used, "attempts": att.reshape((sweeps, steps)),
            "trace": None if tr is None else tr.reshape((sweeps, steps, 101)), "exhausted": ex.value}


def check_replay(case, states, out):
    """Every slice step of the device's sweeps against the reference at the state the device was in.  states[s] = (z, b)
    after sweep s, from the same call cut short.  Threshold and candidates to 1e-10·max(1, |L|), attempts equal except
    where the reference's margin is below 1e-9·max(1, |L|) (at most 1 % of the steps), the new value to 1e-12."""
    assert np.array_equal(out["draws"], case["draws"])
    z_old, b_old = case["z0"], case["b0"]
    excused = total = 0
    for s, (z_new, b_new) in enumerate(states):
        want_z, want_b, att, traces, margins = lr.replay(case["A"], z_old, z_new, b_old, case, case["draws"], sweep_index=s)
        worst = 0.0
        for n, (k, t, m) in enumerate(zip(att, traces, margins)):
            got_k, got_t = int(out["attempts"][s, n]), out["trace"][s, n]
            scale = max(1.0, max(abs(v) for v in t if np.isfinite(v)) if any(np.isfinite(v) for v in t) else 1.0)
            total += 1
            if got_k != k:
                assert m < 1e-9 * scale, (s, n, got_k, k, m)
                excused += 1
                continue
            upto = min(k, lr.MAX_ATTEMPTS)
            for a, w in zip(got_t[:upto + 1], t[:upto + 1]):
                if np.isfinite(w):
                    worst = max(worst, abs(a - w) / scale)
                    assert abs(a - w) <= 1e-10 * scale, (s, n, a, w)
                else:
                    assert a == w
            got = z_new[n] if n < case["N"] else b_new
            want = want_z[n] if n < case["N"] else want_b
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want)))), (s, n, got, want)
        print(f"sweep {s}: worst |L - reference| / max(1, |L|) = {worst:.3e}, mean attempts {np.mean(att):.2f}")
        z_old, b_old = z_new, b_new
    assert excused <= 0.01 * total
    return excused


# ---- 1. every slice step against the replay ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lr.decision_cases()))
def test_slice_steps_against_the_replay(nhp, name):
    c = lr.decision_cases()[name]
    out = gpu_resample(nhp, c)
    assert out["exhausted"] == 0 and np.all(np.isfinite(out["z"])) and np.isfinite(out["b"])
    assert check_replay(c, [(out["z"], out["b"])], out) == 0
    if c["N"] == 1:
        assert out["attempts"][0, 0] == 1 and out["trace"][0, 0, 1] == 0.0          # L ≡ 0


def test_loglikelihood_and_conditionals(nhp):
    for name in ("65x8", "33x2-far", "33x2-b-30", "257x3", "1x1"):
        c = lr.decision_cases()[name]
        net = nhp.LatentDistanceNetworkModel(c["N"], c["D"], z=c["z0"], b=c["b0"])
        ll, cond = net.loglikelihood(c["A"], conditionals=True)
        want = lr.loglik_vec(c["A"], c["z0"], c["b0"])
        assert abs(ll - want) <= 1e-10 * max(1.0, abs(want)), (name, ll, want)
        for n in range(c["N"]):
            w = lr.conditional_vec(c["A"], c["z0"], c["b0"], n)
            assert abs(cond[n] - w) <= 1e-10 * max(1.0, abs(w)), (name, n)


# ---- 2. stale state: three sweeps in one call ------------------------------------------------------------------------------
def test_three_sweeps_in_one_call_equal_three_calls(nhp):
    c = lr.stale_case()
    rs = c["N"] * (c["D"] + 101) + 102
    for do_offset in (True, False):                       # (False: the three sweeps are ONE launch of the sweep kernel)
        three = gpu_resample(nhp, c, do_offset=do_offset)
        z, b, states = c["z0"], c["b0"], []
        for s in range(3):
            one = gpu_resample(nhp, c, z=z, b=b, draws=c["draws"][s * rs:(s + 1) * rs], n_sweeps=1, do_offset=do_offset)
            assert np.array_equal(one["attempts"][0], three["attempts"][s])
            upto = one["attempts"][0]
            for n in range(c["N"] + (1 if do_offset else 0)):
                assert np.array_equal(one["trace"][0, n, :upto[n] + 1], three["trace"][s, n, :upto[n] + 1])
            assert np.all(np.linalg.norm(one["z"] - z, axis=1) > 0)
            z, b = one["z"], one["b"]
            states.append((z, b))
        assert np.array_equal(z, three["z"]) and b == three["b"]
        assert (b != c["b0"]) == do_offset
        if do_offset:
            check_replay(c, states, three)


# ---- 3. batches that accept nothing ----------------------------------------------------------------------------------------
def test_fallback_batches(nhp):
    c = lr.fallback_case()
    out = gpu_resample(nhp, c)
    plan = [[6, 7, 8, 15, 16, 14], [23, 0, 40, 99, 1, 15], [2, 3, 4, 5, 6, 16], [0, 0, 0, 0, 0, 99]]
    assert out["attempts"].tolist() == [[f + 1 for f in fails] for fails in plan]
    assert out["exhausted"] == 0
    z, b, states = c["z0"], c["b0"], []
    for s in range(c["n_sweeps"]):
        z, b, _, _, _ = lr.sweep(c["A"], z, b, 1.0, 0.0, 1.0, c["draws"], sweep_index=s)
        states.append((z, b))
    assert np.max(np.abs(out["z"] - z)) <= 1e-12 and abs(out["b"] - b) <= 1e-12
    # the replay needs the device's state after every sweep: the same call cut short
    cut = [gpu_resample(nhp, c, n_sweeps=s + 1) for s in range(c["n_sweeps"])]
    assert check_replay(c, [(o["z"], o["b"]) for o in cut], out) == 0


# ---- 4. exhaustion ------------------------------------------------------------------------------------------------------------
def test_exhaustion_keeps_the_value_and_is_counted(nhp):
    c = lr.exhaustion_case()
    out = gpu_resample(nhp, c)
    assert out["attempts"].tolist() == [[101, 1, 4, 101, 1, 101]]
    assert out["exhausted"] == 3
    assert np.array_equal(out["z"][0], c["z0"][0]) and np.array_equal(out["z"][3], c["z0"][3]) and out["b"] == c["b0"]
    check_replay(c, [(out["z"], out["b"])], out)


# ---- 5. the kernel's own stream --------------------------------------------------------------------------------------------------
def test_own_stream(nhp):
    c = dict(lr.decision_cases()["65x8"], n_sweeps=4)
    N, D = c["N"], c["D"]
    a = gpu_resample(nhp, c, draws=None, seed=11, step=3, trace=False)
    b = gpu_resample(nhp, c, draws=None, seed=11, step=3, trace=False)
    d = gpu_resample(nhp, c, draws=None, seed=11, step=4, trace=False)
    assert np.array_equal(a["z"], b["z"]) and a["b"] == b["b"] and np.array_equal(a["draws"], b["draws"])
    assert np.array_equal(a["attempts"], b["attempts"])
    assert not np.any(a["draws"] == d["draws"]) and not np.array_equal(a["z"], d["z"])
    e = gpu_resample(nhp, c, draws=a["draws"], trace=False)                          # the stream handed back in
    assert np.array_equal(e["z"], a["z"]) and e["b"] == a["b"] and np.array_equal(e["attempts"], a["attempts"])
    assert a["exhausted"] == 0 and a["attempts"].min() >= 1
    normals, uniforms = [], []
    for s in range(4):
        for n in range(N + 1):
            nrm, u0, us = lr.node_draws(a["draws"], N, D, s, n)
            normals.append(nrm); uniforms.append([u0]); uniforms.append(us)
    normals, uniforms = np.concatenate(normals), np.concatenate(uniforms)
    assert len(normals) == 4 * (N * D + 1) and np.all((uniforms >= 0) & (uniforms < 1))
    assert stats.kstest(normals, "norm").pvalue > P_MIN
    assert stats.kstest(uniforms, "uniform").pvalue > P_MIN
    # one sweep of a longer call draws what the first sweep of a one-sweep call draws
    one = gpu_resample(nhp, dict(c, n_sweeps=1), draws=None, seed=11, step=3, trace=False)
    assert np.array_equal(one["draws"], a["draws"][:len(one["draws"])])


# ---- 6. the posterior, exactly ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lr.posterior_cases()))
def test_positions_follow_the_exact_posterior(nhp, name):
    A, sigma, b = lr.posterior_cases()[name], 1.0, 0.5
    c = {"N": 2, "D": 1, "A": A, "sigma": sigma, "mu_b": 0.0, "sigma_b": 1.0, "n_sweeps": lr.POSTERIOR_THIN}
    z, out, exhausted = np.array([[0.3], [-0.2]]), [], 0
    for k in range(lr.POSTERIOR_SAMPLES):
        r = gpu_resample(nhp, c, z=z, b=b, draws=None, seed=31, step=k, do_offset=False, trace=False)
        z = r["z"]
        exhausted += r["exhausted"]
        out.append(z[0, 0] - z[1, 0])
    p = stats.kstest(out, lambda x: lr.delta_cdf(A[0, 1] + A[1, 0], b, sigma, x)).pvalue
    print(f"{name}: KS p = {p:.4f} over {len(out)} samples, {lr.POSTERIOR_THIN} sweeps apart")
    assert exhausted == 0 and p > P_MIN


def test_offset_follows_the_exact_posterior(nhp):
    A, z, mu_b, sigma_b = lr.offset_posterior_case()
    c = {"N": 3, "D": 2, "A": A, "sigma": 1.0, "mu_b": mu_b, "sigma_b": sigma_b}
    b, out, k = 0.0, [], 0
    for _ in range(lr.POSTERIOR_SAMPLES):
        for _ in range(lr.OFFSET_THIN):
            r = gpu_resample(nhp, c, z=z, b=b, draws=None, seed=32, step=k, n_sweeps=0, trace=False)
            assert r["exhausted"] == 0 and np.array_equal(r["z"], z)
            b, k = r["b"], k + 1
        out.append(b)
    p = stats.kstest(out, lambda x: lr.offset_cdf(A, z, mu_b, sigma_b, x)).pvalue
    print(f"offset: KS p = {p:.4f}")
    assert p > P_MIN


# ---- 7. two planted clusters ----------------------------------------------------------------------------------------------------------
def test_planted_clusters_are_recovered(nhp):
    c = lr.planted_case()
    net = nhp.LatentDistanceNetworkModel(c["N"], c["D"], z=c["z0"], b=c["b0"], σ=c["sigma"], μb=c["mu_b"], σb=c["sigma_b"])
    acc, exhausted = np.zeros((c["N"], c["N"])), 0
    for s in range(lr.RECOVERY_SWEEPS):
        net.resample_(c["A"], None, seed=9, step=s)
        exhausted += net.exhausted
        if s >= lr.RECOVERY_BURN:
            acc += net.link_probability()
    gap = lr.cluster_gap(acc / (lr.RECOVERY_SWEEPS - lr.RECOVERY_BURN), c["truth"])
    want = lr.reference_recovery_gap(c)
    print(f"gap of the posterior mean link probabilities: GPU chain {gap:.3f}, reference chain {want:.3f}")
    assert exhausted == 0 and want > 0.1 and gap >= 0.5 * want


# ---- 8. chains ----------------------------------------------------------------------------------------------------------------------------
def latent_process(nhp, N=12, M=2000, D=2, seed=3):
    c = random_case(N, M, 150.0, "exponential", 1.0, network=True, seed=seed, nhp=nhp)
    rng = np.random.default_rng(seed)
    c["proc"].network = nhp.LatentDistanceNetworkModel(N, D, z=rng.standard_normal((N, D)), b=0.4, σ=1.5, μb=0.2, σb=2.0)
    return c


def test_chain_routes_agree(nhp):
    N, steps = 12, 20
    a = latent_process(nhp)
    ra = nhp.mcmc_(a["proc"], a["data"], nsteps=steps, seed=8, keep_samples=False, moments=True)
    b = latent_process(nhp)
    rb = nhp.mcmc_(b["proc"], b["data"], nsteps=steps, seed=8, keep_samples=True, moments=True)
    na, nb = a["proc"].network, b["proc"].network
    assert np.array_equal(a["proc"].adjacency_matrix, b["proc"].adjacency_matrix)
    assert np.array_equal(na.z, nb.z) and na.b == nb.b and na.b != 0.4
    assert np.array_equal(a["proc"].params(), b["proc"].params())
    samples = np.array(rb.samples)
    assert samples.shape == (steps, len(a["proc"].params()))
    for r in (ra, rb):
        assert r.n == steps and r.exhausted == 0
        assert abs(r.mean[0] - samples[:, 0].mean()) <= 1e-12 and abs(r.m2[0] - (samples[:, 0] ** 2).mean()) <= 1e-12
        assert r.link_probability_mean.shape == (N, N) and np.all((r.link_probability_mean > 0) & (r.link_probability_mean < 1))
    assert np.max(np.abs(ra.link_probability_mean - rb.link_probability_mean)) <= 1e-12
    assert np.allclose(ra.mean, rb.mean, rtol=0, atol=1e-12) and np.allclose(ra.m2, rb.m2, rtol=0, atol=1e-12)
    # one kept step: the mean link probability is that of the final state
    o = latent_process(nhp)
    ro = nhp.mcmc_(o["proc"], o["data"], nsteps=3, seed=8, keep_samples=False, moments=True, burn=2)
    assert ro.n == 1 and np.max(np.abs(ro.link_probability_mean - o["proc"].network.link_probability())) <= 1e-12
    # the host-draw route: A comes back every step, the network is resampled through the stand-alone entry
    h = latent_process(nhp)
    rh = nhp.mcmc_(h["proc"], h["data"], nsteps=5, seed=8, device_draws=False)
    nh = h["proc"].network
    assert rh.steps == 5 and len(rh.samples) == 5 and rh.exhausted == 0
    assert nh.z.shape == (N, 2) and np.all(np.isfinite(nh.z)) and np.isfinite(nh.b)
    assert set(np.unique(h["proc"].adjacency_matrix)) <= {0.0, 1.0}
    assert rh.samples[-1][0] == nh.b


def test_device_step_equals_the_stand_alone_entries(nhp):
    """One device-resident network step (link probabilities, adjacency sweep, positions, offset -- nothing leaves the
    device) against the same step made of the host-visible pieces, keyed by the same (seed, step)."""
    _lib, lib, ctx = lib_ctx(nhp)
    N, seed, step = 12, 13, 6
    a = latent_process(nhp)
    proc, net = a["proc"], a["proc"].network
    ds, model = nhp.device_dataset(proc, a["data"], ctx), proc.device_model(ctx)
    _lib.check(lib.nhp_cont_model_set_latent(ctx.h, model.h, net.ndims, _lib.dptr(_lib.colmajor(net.z)), net.b, net.σ, net.μb, net.σb), ctx.h)
    _lib.check(lib.nhp_cont_latent_step(ctx.h, ds.h, model.h, seed, step), ctx.h)
    zd, bd, Ad, ex = np.empty(N * 2), C.c_double(), np.empty(N * N), C.c_int64(-1)
    _lib.check(lib.nhp_cont_model_get_latent(ctx.h, model.h, _lib.dptr(zd), C.byref(bd), None, None, C.byref(ex)), ctx.h)
    _lib.check(lib.nhp_cont_model_get_adjacency(ctx.h, model.h, _lib.dptr(Ad), N * N), ctx.h)
    b = latent_process(nhp)
    links = nhp.resample_adjacency_matrix_(b["proc"], b["data"], seed=seed, step=step)
    assert 0 < links < N * N
    b["proc"].network.resample_(b["proc"].adjacency_matrix, None, seed=seed, step=step)
    assert np.array_equal(Ad.reshape((N, N), order="F"), b["proc"].adjacency_matrix)
    assert np.array_equal(zd.reshape((N, 2), order="F"), b["proc"].network.z) and bd.value == b["proc"].network.b
    assert ex.value == 0 and not np.array_equal(b["proc"].network.z, net.z)


def test_positions_every_keeps_the_positions_between_sweeps(nhp):
    a = latent_process(nhp)
    nhp.mcmc_(a["proc"], a["data"], nsteps=3, seed=8, keep_samples=False, positions_every=3)       # positions at step 0 only
    b = latent_process(nhp)
    nhp.mcmc_(b["proc"], b["data"], nsteps=1, seed=8, keep_samples=False)
    assert np.array_equal(a["proc"].network.z, b["proc"].network.z)
    assert a["proc"].network.b != b["proc"].network.b
    # ... and on the route through the stand-alone entry
    h = latent_process(nhp)
    nhp.mcmc_(h["proc"], h["data"], nsteps=3, seed=8, device_draws=False, positions_every=3)
    g = latent_process(nhp)
    nhp.mcmc_(g["proc"], g["data"], nsteps=1, seed=8, device_draws=False)
    assert np.array_equal(h["proc"].network.z, g["proc"].network.z) and h["proc"].network.b != g["proc"].network.b


@pytest.mark.parametrize("kind", ["bernoulli", "dense", "block"])
def test_another_network_after_a_latent_chain_is_the_chain_of_a_fresh_process(nhp, kind):
    """The device model is cached on the process and carries the latent state; another network kind must detach it
    (nhp_cont_model_set_rho and _set_sbm do), or the resident route would go on sampling the latent model."""
    def network():
        if kind == "bernoulli":
            return nhp.BernoulliNetworkModel(0.4, 12, 2.0, 3.0)
        return nhp.DenseNetworkModel(12) if kind == "dense" else nhp.StochasticBlockNetworkModel(12, 2, ρ=[[0.6, 0.2], [0.3, 0.7]])

    def state(p, r):
        return p.params(), p.adjacency_matrix, r.mean, r.m2

    used = latent_process(nhp)
    nhp.mcmc_(used["proc"], used["data"], nsteps=3, seed=8, keep_samples=False, moments=True)
    model = used["proc"]._dev
    fresh = latent_process(nhp)
    for name in ("baseline", "impulses", "weights"):
        setattr(used["proc"], name, getattr(latent_process(nhp)["proc"], name))
    used["proc"].adjacency_matrix = fresh["proc"].adjacency_matrix.copy()
    used["proc"].network, fresh["proc"].network = network(), network()
    ru = nhp.mcmc_(used["proc"], used["data"], nsteps=6, seed=9, keep_samples=False, moments=True)
    assert used["proc"]._dev is model                                # the cached device model was reused
    rf = nhp.mcmc_(fresh["proc"], fresh["data"], nsteps=6, seed=9, keep_samples=False, moments=True)
    for a, b in zip(state(used["proc"], ru), state(fresh["proc"], rf)):
        assert np.array_equal(a, b)
    _lib, lib, ctx = lib_ctx(nhp)
    with pytest.raises(_lib.NhpError, match="no latent distance network"):
        _lib.check(lib.nhp_cont_model_get_latent(ctx.h, model.h, None, None, None, None, None), ctx.h)
    # ... and the reverse: a latent chain on the model the other network used is the latent chain of a fresh process
    used["proc"].network = latent_process(nhp)["proc"].network
    again = latent_process(nhp)
    for name in ("baseline", "impulses", "weights"):
        setattr(used["proc"], name, getattr(latent_process(nhp)["proc"], name))
    used["proc"].adjacency_matrix = again["proc"].adjacency_matrix.copy()
    r1 = nhp.mcmc_(used["proc"], used["data"], nsteps=4, seed=10, keep_samples=False, moments=True)
    r2 = nhp.mcmc_(again["proc"], again["data"], nsteps=4, seed=10, keep_samples=False, moments=True)
    assert used["proc"]._dev is model
    for a, b in zip(state(used["proc"], r1) + (used["proc"].network.z, r1.link_probability_mean),
                    state(again["proc"], r2) + (again["proc"].network.z, r2.link_probability_mean)):
        assert np.array_equal(a, b)
    if kind == "block":
        with pytest.raises(_lib.NhpError, match="no block network"):
            _lib.check(lib.nhp_cont_model_get_sbm(ctx.h, model.h, None, None, None, None, None), ctx.h)


def test_discrete_chain_with_the_latent_model(nhp):
    def run():
        N, T, B = 8, 500, 3
        rng = np.random.default_rng(2)
        data = rng.poisson(0.3, (N, T)).astype(np.int64)
        net = nhp.LatentDistanceNetworkModel(N, 2, z=rng.standard_normal((N, 2)), b=0.5)
        proc = nhp.DiscreteNetworkHawkesProcess(
            nhp.DiscreteHomogeneousProcess(np.full(N, 0.2), 1.0), nhp.DiscreteGaussianImpulseResponse(np.full((N, N, B), 1.0 / B), 6, 1.0),
            nhp.DenseWeightModel(np.full((N, N), 0.05)), (rng.uniform(size=(N, N)) < 0.5).astype(np.float64), net, 1.0)
        res = nhp.mcmc_(proc, data, nsteps=5, seed=4)                 # (dispatches to disc_mcmc_)
        return proc, res
    p1, r1 = run()
    p2, r2 = run()
    assert r1.steps == 5 and p1.network.b != 0.5 and p1.network.z.shape == (8, 2) and np.all(np.isfinite(p1.network.z))
    assert np.array_equal(p1.network.z, p2.network.z) and p1.network.b == p2.network.b
    assert np.array_equal(p1.adjacency_matrix, p2.adjacency_matrix) and np.array_equal(p1.params(), p2.params())


def test_flat_link_probabilities_sweep_the_adjacency_matrix_like_the_bernoulli_model(nhp):
    """D = 1, every position at 0: P is flat at 1 / (1 + exp(-b)), and the adjacency sweep is the Bernoulli model's at that ρ."""
    b = 0.3

    def swept(network):
        c = random_case(9, 1500, 120.0, "exponential", 1.0, network=True, seed=5, nhp=nhp)
        c["proc"].network = network
        nhp.invalidate_device_datasets()
        links = nhp.resample_adjacency_matrix_(c["proc"], c["data"], seed=21, step=6)
        return c["proc"].adjacency_matrix.copy(), links
    A1, l1 = swept(nhp.LatentDistanceNetworkModel(9, 1, b=b, σ=1e-9))
    A2, l2 = swept(nhp.BernoulliNetworkModel(1.0 / (1.0 + np.exp(-b)), 9))
    assert np.array_equal(A1, A2) and l1 == l2 and 0 < l1 < 81
    # ... and inside the device step: with σ tiny the positions stay at 0, so the fill is flat at every step
    _lib, lib, ctx = lib_ctx(nhp)

    def chain(network):
        c = random_case(9, 1500, 120.0, "exponential", 1.0, network=True, seed=5, nhp=nhp)
        c["proc"].network = network
        ds, model = nhp.device_dataset(c["proc"], c["data"], ctx), c["proc"].device_model(ctx)
        if isinstance(network, nhp.LatentDistanceNetworkModel):
            _lib.check(lib.nhp_cont_model_set_latent(ctx.h, model.h, 1, _lib.dptr(_lib.colmajor(network.z)), b, 1e-9, 0.0, 1.0), ctx.h)
            _lib.check(lib.nhp_cont_latent_step(ctx.h, ds.h, model.h, 21, 6), ctx.h)
        else:
            _lib.check(lib.nhp_cont_model_set_rho(ctx.h, model.h, network.ρ), ctx.h)
            _lib.check(lib.nhp_cont_network_step(ctx.h, None, ds.h, model.h, 1.0, 1.0, 21, 6), ctx.h)
        A = np.empty(81)
        _lib.check(lib.nhp_cont_model_get_adjacency(ctx.h, model.h, _lib.dptr(A), 81), ctx.h)
        return A
    assert np.array_equal(chain(nhp.LatentDistanceNetworkModel(9, 1, b=b, σ=1e-9)), chain(nhp.BernoulliNetworkModel(1.0 / (1.0 + np.exp(-b)), 9)))


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(nhp):
    _lib, lib, ctx = lib_ctx(nhp)
    base = lr.decision_cases()["3x2"]

    def resample(**kw):
        c = dict(base, **kw)
        return gpu_resample(nhp, c, draws=None, n_sweeps=kw.get("n_sweeps", 1), trace=False)

    resample()
    with pytest.raises(_lib.NhpError, match="must lie in 1..8"):
        resample(D=0, z0=np.zeros((3, 0)))
    with pytest.raises(NotImplementedError, match="must lie in 1..8"):
        resample(D=9, z0=np.zeros((3, 9)))
    with pytest.raises(_lib.NhpError, match="n_sweeps"):
        resample(n_sweeps=-1)
    with pytest.raises(nhp.DomainError, match="not finite"):
        resample(z0=np.array([[0.0, 1.0], [np.nan, 0.0], [0.0, 0.0]]))
    with pytest.raises(nhp.DomainError, match="not finite"):
        resample(b0=np.inf)
    for kw in ({"sigma": 0.0}, {"sigma": -1.0}, {"sigma_b": 0.0}):
        with pytest.raises(nhp.DomainError, match="sigma"):
            resample(**kw)
    # above the position sweep's LDS: refused with the reason, no fallback
    for N, D in ((8193, 1), (4096, 5)):                                 # N too large; 8·N·D = 160 KiB before the scratch
        with pytest.raises(NotImplementedError, match="LDS"):
            _lib.check(lib.nhp_latent_loglik(ctx.h, _lib.dptr(np.zeros(1)), N, D, _lib.dptr(np.zeros(1)), 0.0, _lib.dptr(np.zeros(1))), ctx.h)
    # the device-resident state: same checks, and a column shard is refused
    cc = latent_process(nhp)
    proc, net = cc["proc"], cc["proc"].network
    model = proc.device_model(ctx)

    def set_latent(D=2, z=net.z, b=0.1, pri=(1.0, 0.0, 1.0)):
        _lib.check(lib.nhp_cont_model_set_latent(ctx.h, model.h, D, _lib.dptr(_lib.colmajor(z)), b, *pri), ctx.h)

    with pytest.raises(_lib.NhpError, match="no latent distance network"):
        _lib.check(lib.nhp_cont_latent_step(ctx.h, nhp.device_dataset(proc, cc["data"], ctx).h, model.h, 0, 0), ctx.h)
    with pytest.raises(NotImplementedError, match="must lie in 1..8"):
        set_latent(D=9, z=np.zeros((12, 9)))
    with pytest.raises(nhp.DomainError, match="not finite"):
        set_latent(z=np.full((12, 2), np.nan))
    with pytest.raises(nhp.DomainError, match="sigma"):
        set_latent(pri=(0.0, 0.0, 1.0))
    set_latent()
    with pytest.raises(_lib.NhpError, match="positive"):
        _lib.check(lib.nhp_cont_model_set_latent_positions_every(ctx.h, model.h, 0), ctx.h)
    times, nodes, T = cc["data"]
    h = C.c_void_p()
    _lib.check(lib.nhp_cont_dataset_create_columns(ctx.h, _lib.dptr(_lib.f64(times)), _lib.iptr(np.ascontiguousarray(nodes, dtype=np.int64)),
                                                   len(times), 12, T, 1.0, 0, 6, C.byref(h)), ctx.h)
    try:
        with pytest.raises(NotImplementedError, match="column shard"):
            _lib.check(lib.nhp_cont_latent_step(ctx.h, h, model.h, 0, 0), ctx.h)
    finally:
        lib.nhp_cont_dataset_destroy(h)
    from nhp_amd.sharded import ShardedDataset
    with pytest.raises(NotImplementedError, match="not sharded"):
        nhp.mcmc_(proc, ShardedDataset.__new__(ShardedDataset), nsteps=1, keep_samples=False)
    from nhp_amd import chains
    import types
    with pytest.raises(NotImplementedError, match="latent distance network"):
        chains.gather_device_summaries({0: (proc, None)}, 1, None, types.SimpleNamespace(world=1, rank=0))
