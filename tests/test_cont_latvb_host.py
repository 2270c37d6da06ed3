"""The continuous latent-distance-network variational fit's definition, checked without a GPU: the gradient of the numpy/scipy
restatement (tests/clatvb_ref.py) against central differences and against 50-digit arithmetic, the quadratic-in-t form of a
rung against F at the moved point, F and the ELBO rising over the restated iterations, variational_init_ and
has_variational_state, ContinuousLatentNetworkVariational's accessors, the argument errors raised before any device work, the
new symbols in _lib.py and libnhp.so, and the host-only checks in a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import clatvb_ref as cl
import cnetvb_ref as cr
import disc_netvb_ref as dn
import em_ref as er
from helpers import random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _soft_links(N, D, seed, planted=False):
    """Random positions and link probabilities; `planted`: A drawn from the positions' own probabilities, softened to 0.05 / 0.95."""
    rng = np.random.default_rng(seed)
    z, b = rng.standard_normal((N, D)), 0.7
    rho = rng.uniform(size=(N, N))
    if planted:
        rho = np.where(rng.uniform(size=(N, N)) < dn.sigmoid(cl.eta(z, b)), 0.95, 0.05)
    return z, b, rho


@pytest.mark.parametrize("N,D", [(5, 1), (7, 3), (6, 8)])
def test_the_gradient_is_the_derivative_of_F(N, D):
    """∇F of the restatement against central differences of F (h = 1e-5: truncation h²·|F'''| and rounding eps·|F|/h are both
    below 1e-6 of these sizes) and against central differences of the 50-digit twin (h = 1e-12, no rounding to speak of: 1e-9)."""
    z, b, rho = _soft_links(N, D, 1)
    rho[0, 1], rho[2, 2], rho[1, 0] = 0.0, 1.0, 1.0
    lp = cl.LPRI
    gz, gb = cl.grad(z, b, rho, lp)
    h = 1e-5
    num = np.zeros_like(z)
    for n in range(N):
        for d in range(D):
            zp, zm = z.copy(), z.copy()
            zp[n, d] += h
            zm[n, d] -= h
            num[n, d] = (cl.F(zp, b, rho, lp) - cl.F(zm, b, rho, lp)) / (2 * h)
    nb = (cl.F(z, b + h, rho, lp) - cl.F(z, b - h, rho, lp)) / (2 * h)
    scale = max(1.0, float(np.max(np.abs(gz))))
    assert np.max(np.abs(num - gz)) <= 1e-6 * scale and abs(nb - gb) <= 1e-6 * scale
    assert abs(cl.F(z, b, rho, lp) - cl.F_mp(z, b, rho, lp)) <= 1e-13 * max(1.0, abs(cl.F(z, b, rho, lp)))
    # the 50-digit twin along two coordinates and the offset
    mp = cl._mp()

    def f_mp(zz, bb):
        return mp.mpf(0) + _F_mp_exact(zz, bb, rho, lp)
    hh = mp.mpf(10) ** -12
    for n, d in ((0, 0), (N - 1, D - 1)):
        zp = [[mp.mpf(float(v)) for v in row] for row in z]
        zm = [[mp.mpf(float(v)) for v in row] for row in z]
        zp[n][d] += hh
        zm[n][d] -= hh
        assert abs(float((f_mp(zp, mp.mpf(b)) - f_mp(zm, mp.mpf(b))) / (2 * hh)) - gz[n, d]) <= 1e-9 * scale
    zq = [[mp.mpf(float(v)) for v in row] for row in z]
    assert abs(float((f_mp(zq, mp.mpf(b) + hh) - f_mp(zq, mp.mpf(b) - hh)) / (2 * hh)) - gb) <= 1e-9 * scale


def _F_mp_exact(Zm, bm, rho, lpri):
    """clatvb_ref.F_mp on mpmath positions (so that a 1e-12 step is not rounded away)."""
    mp = cl._mp()
    s, mu, sb = (mp.mpf(float(v)) for v in lpri)
    N, D = len(Zm), len(Zm[0])
    tot = mp.mpf(0)
    for p in range(N):
        for c in range(N):
            e = bm - mp.fsum((Zm[p][d] - Zm[c][d]) ** 2 for d in range(D))
            tot += mp.mpf(float(rho[p, c])) * e - ((e if e > 0 else mp.mpf(0)) + mp.log1p(mp.exp(-abs(e))))
    return tot - mp.fsum(v * v for row in Zm for v in row) / (2 * s * s) - (bm - mu) ** 2 / (2 * sb * sb)


@pytest.mark.parametrize("N,D", [(5, 1), (12, 2), (9, 8)])
def test_a_rung_is_F_at_the_moved_point(N, D):
    """The quadratic-in-t form of every rung (and of t = 0) against F evaluated directly at (z, b) + t·G: within 16 ulp of the
    terms' magnitudes, η's own terms included."""
    z, b, rho = _soft_links(N, D, 2)
    lp = cl.LPRI
    gz, gb = cl.grad(z, b, rho, lp)
    ts = np.concatenate([cl.ladder(N, lp[0]), [0.0]])
    Fs, mags = cl.ray(z, b, rho, lp, gz, gb, ts)
    for t, f, m in zip(ts, Fs, mags):
        direct = cl.F(z + t * gz, b + t * gb, rho, lp)
        assert abs(f - direct) <= 16 * EPS * m, (t, f, direct)
    assert Fs[-1] == pytest.approx(cl.F(z, b, rho, lp), rel=1e-15)
    assert ts[0] == 4 * ts[1] and ts[1] == 1.0 / (N + 1.0 / lp[0] ** 2) and np.all(ts[1:8] * 4 == ts[:7])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_F_never_falls_over_the_restated_iterations(seed):
    """50 iterations from 0.1·N(0, I) positions at planted soft links: F at every iteration's start never falls (a rung is
    taken only if its F exceeds the current one, both through the same form: the allowance is the form's rounding against the
    next iteration's own evaluation, 16 ulp of the terms), rises overall, and the fitted link probabilities correlate with the
    planted ones."""
    N, D = 12, 2
    zt, bt, rho = _soft_links(N, D, seed, planted=True)
    z0 = 0.1 * np.random.default_rng(seed + 10).standard_normal((N, D))
    lp = cl.LPRI
    z, b, taken, cur = cl.ascent(z0, 0.0, rho, lp, 50)
    cur.append(cl.F(z, b, rho, lp))
    allow = 16 * EPS * cl.F_terms(z, b, rho, lp)
    assert np.all(np.diff(cur) >= -allow) and cur[-1] > cur[0] + 1.0
    assert all(-1 <= r < cl.RUNGS for r in taken) and max(taken) >= 0
    corr = np.corrcoef(dn.sigmoid(cl.eta(z, b)).ravel(), dn.sigmoid(cl.eta(zt, bt)).ravel())[0, 1]
    print(f"seed {seed}: F {cur[0]:.4f} -> {cur[-1]:.4f}, rungs {sorted(set(taken))}, correlation {corr:.3f}")
    assert corr > 0.5
    # a replay with the rungs taken is the same trajectory, and J = 0 moves nothing
    z2, b2, _, _ = cl.ascent(z0, 0.0, rho, lp, 50, rungs=taken)
    assert np.array_equal(z2, z) and b2 == b
    z3, b3, none, _ = cl.ascent(z0, 0.0, rho, lp, 0)
    assert z3 is z0 and b3 == 0.0 and none == []


@pytest.mark.parametrize("kind,dt_max,recursive", [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)])
def test_restated_elbo_never_falls(nhp, kind, dt_max, recursive):
    """15 restated steps with J = 3 from a random guess: every block is a coordinate ascent of one bound, so the trace never
    falls beyond the rounding of its terms (1e-11·max(1, |L|), tests/test_cont_netvb_host.py's bound)."""
    N, D = 4, 2
    c = random_case(N, 400, 40.0, kind, dt_max, seed=11, nhp=nhp)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive)
    guess = er.from_vector(np.random.default_rng(3).uniform(0.2, 0.8, len(c["proc"].params())), N, kind, dt_max)
    q = cl.priors()
    state, trace, Fs = cl.run(guess, pr, q, 15, cl.random_lat(N, D, 1), 3)
    rise = np.diff(trace)
    print(f"{kind} dt_max={dt_max} recursive={recursive}: L {trace[0]:.4f} -> {trace[-1]:.6f}, smallest rise {rise.min():.3e}")
    assert len(trace) == 15 and np.all(np.isfinite(trace)) and rise.min() >= -1e-11 * max(1.0, abs(trace[-1])) and trace[-1] > trace[0]
    back = cl.from_planes(*cl.planes(state), N, D, kind)
    assert all(np.array_equal(back[k], state[k]) for k in state if k not in ("lat", "rungs", "na", "nb"))
    assert np.array_equal(back["lat"][0], state["lat"][0]) and back["lat"][1] == state["lat"][1]
    ent, links, lnz, lnb = cl.network_pieces(state["lat"], state["rho"], q["lpri"])
    assert cl.kl_net(state["lat"], state["rho"], q["lpri"]) == ent - (links + lnz + lnb)
    s_, _, sb_ = q["lpri"]
    quads = (lnz + 0.5 * N * D * np.log(2 * np.pi * s_ ** 2)) + (lnb + 0.5 * np.log(2 * np.pi * sb_ ** 2))      # the constants taken out again
    assert links + quads == pytest.approx(cl.F(state["lat"][0], state["lat"][1], state["rho"], q["lpri"]), rel=1e-13)
    assert np.all(np.diff(Fs) > -1e3) and len(Fs) == 15


def test_the_restatements_own_errors_are_small():
    """The measured errors the GPU tests use as bounds: the logit below 1e-13, F below 1e-14 relative."""
    assert 0.0 < cl.measured_logit_error() < 1e-13
    assert cl.measured_F_error() < 1e-14


def test_variational_init_and_the_bare_object(nhp):
    net = nhp.LatentDistanceNetworkModel(5, 2, σ=1.3)
    assert not net.has_variational_state() and net.zv is None and net.bv is None
    assert not object.__new__(nhp.LatentDistanceNetworkModel).has_variational_state()
    with pytest.raises(ValueError, match="saddle"):
        net.variational_init_(scale=0.0)
    with pytest.raises(ValueError, match="ascent_steps"):
        net.variational_init_(ascent_steps=65)
    with pytest.raises(ValueError, match="scale"):
        net.variational_init_(scale=-1.0)
    assert not net.has_variational_state()
    assert net.variational_init_() is net and net.has_variational_state()
    want = 0.1 * np.random.default_rng(0).standard_normal((5, 2))
    assert np.array_equal(net.zv, want) and net.bv == 0.0 and net.ascent_steps == 4
    assert np.array_equal(net.variational_params(), np.concatenate([want.ravel(order="F"), [0.0]]))
    assert np.all(net.z == 0.0)                                       # the sampler's state is not touched
    apart = nhp.LatentDistanceNetworkModel(3, 1, z=[[0.0], [1.0], [2.0]], b=0.5)
    apart.variational_init_(scale=0.0, ascent_steps=0)
    assert np.array_equal(apart.zv, apart.z) and apart.zv is not apart.z and apart.bv == 0.5 and apart.ascent_steps == 0
    other = nhp.LatentDistanceNetworkModel(5, 2).variational_init_(seed=3, scale=0.5)
    assert np.array_equal(other.zv, 0.5 * np.random.default_rng(3).standard_normal((5, 2)))


def _network_process(nhp, N=3, kind="exponential", network=None, lgcp=False, D=2):
    c = random_case(N, 50, 10.0, kind, 1.0, lgcp=lgcp, seed=1, nhp=nhp)
    base = c["proc"]
    w = nhp.SparseWeightModel(base.weights.W, 0.3, 30.0, 1.5, 2.0)
    net = nhp.LatentDistanceNetworkModel(N, D).variational_init_() if network is None else network
    return nhp.ContinuousNetworkHawkesProcess(base.baseline, base.impulses, w, np.ones((N, N)), net), c["data"]


def _state_object(nhp, state, kind, N, D, q, **kw):
    return nhp.ContinuousLatentNetworkVariational(kind, N, *cl.planes(state), D, prior_kappa=q["kappa"], **kw)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_the_result_class_returns_what_the_planes_hold(nhp, kind):
    N, D, q = 3, 2, cl.priors()
    st = cl.random_state(N, D, kind, seed=5)
    res = _state_object(nhp, st, kind, N, D, q, ascent_steps=7)
    assert isinstance(res, nhp.ContinuousNetworkVariational) and isinstance(res, nhp.ContinuousVariational)
    for name, key in (("kappa0", "kappa0"), ("nu0", "nu0"), ("rho", "rho"), ("kappa", "kappa"), ("nu", "nu"), ("a", "a"), ("b", "b")):
        assert np.array_equal(getattr(res, name), st[key]), name
    assert res.net_alpha is None and res.net_beta is None and not res.dense and res.ascent_steps == 7 and res.ndims == D
    assert np.array_equal(res.positions(), st["lat"][0]) and res.offset() == st["lat"][1] and res.Z.shape == (N * D + 1,)
    assert np.array_equal(res.link_probability(), st["rho"]) and res.link_probability() is not res.rho
    assert np.allclose(res.network_link_probability(), dn.sigmoid(cl.eta(*st["lat"])), rtol=1e-14, atol=0.0)
    assert np.all(np.diag(res.network_link_probability()) == 1.0 / (1.0 + np.exp(-st["lat"][1])))
    S, R, Q, Z = cl.planes(st)
    assert res.mean().shape == S.shape and np.array_equal(res.expected_links(), st["kappa"] - q["kappa"])
    with pytest.raises(ValueError, match="Q must hold"):
        nhp.ContinuousLatentNetworkVariational(kind, N, S, R, np.ones(3 * N * N + 2), Z, D)
    with pytest.raises(ValueError, match="Z must hold"):
        nhp.ContinuousLatentNetworkVariational(kind, N, S, R, Q, Z[:-1], D)
    with pytest.raises(ValueError, match="Z must hold"):
        nhp.ContinuousLatentNetworkVariational(kind, N, S, R, Q, np.ones(N * 9 + 1), 9)
    with pytest.raises(ValueError, match="ascent_steps"):
        nhp.ContinuousLatentNetworkVariational(kind, N, S, R, Q, Z, D, ascent_steps=-1)


def test_argument_errors_are_raised_before_any_device_work(nhp):
    """A latent network without a state: NotImplementedError naming the class and variational_init_; an LGCP baseline and a
    ShardedDataset: NotImplementedError; hyper-parameters, a state, a guess or an init that cannot be: ValueError / TypeError --
    none of them touches a device (there is none here)."""
    N = 3
    for fn in (nhp.vb_, nhp.update_):
        for bare in (nhp.LatentDistanceNetworkModel(N, 2), object.__new__(nhp.LatentDistanceNetworkModel)):
            with pytest.raises(NotImplementedError, match=r"LatentDistanceNetworkModel.*variational_init_"):
                fn(*_network_process(nhp, network=bare))
        with pytest.raises(NotImplementedError, match="LogGaussianCoxProcess"):
            fn(*_network_process(nhp, lgcp=True))
        proc, data = _network_process(nhp)
        with pytest.raises(NotImplementedError, match="shard"):
            fn(proc, object.__new__(nhp.ShardedDataset))
        for holder, name in ((proc.weights, "κ0"), (proc.weights, "ν0"), (proc.weights, "κ1"), (proc.network, "σ"), (proc.network, "σb"),
                             (proc.baseline, "α0")):
            for bad in (0.0, -1.0, np.nan, np.inf):
                keep = getattr(holder, name)
                setattr(holder, name, bad)
                with pytest.raises(ValueError, match="must be positive and finite"):
                    fn(proc, data)
                setattr(holder, name, keep)
        for name, bad, match in (("μb", np.nan, "mu_b"), ("μb", np.inf, "mu_b"), ("ascent_steps", -1, "ascent_steps"), ("ascent_steps", 65, "ascent_steps"),
                                 ("bv", np.nan, "finite"), ("zv", np.zeros((N, 3)), "shape"), ("zv", np.full((N, 2), np.inf), "finite"),
                                 ("ndims", 9, "ndims")):
            keep = getattr(proc.network, name)
            setattr(proc.network, name, bad)
            with pytest.raises(ValueError, match=match):
                fn(proc, data)
            setattr(proc.network, name, keep)
        proc.weights.ρv = np.full((N, N), 1.5)
        with pytest.raises(ValueError, match="ρv"):
            fn(proc, data)
        proc.weights.ρv = None
        bern = nhp.ContinuousNetworkVariational("exponential", N, *cr.planes(cr.random_state(N, "exponential", 1)))
        with pytest.raises(TypeError, match="ContinuousLatentNetworkVariational"):
            fn(proc, data, init=bern)
        other = _state_object(nhp, cl.random_state(N, 2, "logitnormal", 1), "logitnormal", N, 2, cl.priors())
        with pytest.raises(ValueError, match="Parameter vector length"):
            fn(proc, data, init=other)
        wrong_D = _state_object(nhp, cl.random_state(N, 3, "exponential", 1), "exponential", N, 3, cl.priors())
        with pytest.raises(ValueError, match="Parameter vector length"):
            fn(proc, data, init=wrong_D)
    proc, data = _network_process(nhp)
    with pytest.raises(ValueError, match="Parameter vector length"):
        nhp.vb_(proc, data, guess=np.full(7, 0.5))
    with pytest.raises(ValueError):
        nhp.vb_(proc, data, max_steps=0)
    good = _state_object(nhp, cl.random_state(N, 2, "exponential", 1), "exponential", N, 2, cl.priors())
    with pytest.raises(ValueError, match="not both"):
        nhp.vb_(proc, data, init=good, guess=np.full(N + 2 * N * N, 0.5))
    with pytest.raises(ValueError, match="probabilities"):
        proc.network.expected_loglikelihood(np.full((N, N), 1.5))
    with pytest.raises(ValueError, match="probabilities"):
        proc.network.expected_loglikelihood(np.full((N, N + 1), 0.5))
    from nhp_amd import inference
    pr, netp, is_dense = inference._netvb_check(proc, data, "vb!")
    assert not is_dense and (pr.kappa, pr.nu) == (1.5, 2.0) and list(netp[:2]) == [0.3, 30.0]
    fit = inference._network_fit(proc, pr, netp, is_dense)
    assert fit.entry == "latvb" and fit.nstats == 19 + 4 and fit.netpieces == 4 and fit.rungs and fit.lead[2:] == (2, 4)
    arrays, step0 = fit.arrays(None, "vb!")
    assert step0 is None and arrays[2].shape == (3 * N * N,) and np.array_equal(arrays[3], proc.network.variational_params())
    assert np.array_equal(arrays[2][2 * N * N:], proc.network.link_probability().ravel(order="F"))
    # the discrete process keeps its refusal, state or no state
    from nhp_amd import discrete
    fake = object.__new__(discrete.DiscreteNetworkHawkesProcess)
    fake.weights, fake.network = proc.weights, proc.network
    with pytest.raises(NotImplementedError, match="LatentDistanceNetworkModel"):
        discrete._vb_kind(fake, "update!")


def test_the_new_symbols_are_declared_and_built():
    from nhp_amd import _lib
    lib = _lib.lib()
    for name, nargs in (("nhp_cont_latvb_step", 16), ("nhp_cont_latvb_run", 21), ("nhp_latent_expected_loglik", 8)):
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    header = open(os.path.join(ROOT, "include", "nhp.h")).read()
    for name in ("nhp_cont_latvb_step", "nhp_cont_latvb_run", "nhp_latent_expected_loglik"):
        assert f"nhp_status {name}(" in header
    jl = open(os.path.join(ROOT, "networkhawkesprocesses.jl_amd", "julia", "NetworkHawkesHIP.jl")).read()
    assert ":nhp_cont_latvb_run" in jl and ":nhp_cont_latvb_step" in jl and ":nhp_latent_expected_loglik" in jl


def test_the_host_checks_pass_under_the_host_sanitizers(tmp_path):
    """tools/clatvb_host_check.cpp: a program of its own (nothing of it is loaded into this process), built with
    -fsanitize=address,undefined and run; it exits 0."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "clatvb_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "networkhawkesprocesses.jl_amd", "csrc"), os.path.join(ROOT, "tools", "clatvb_host_check.cpp"), "-o", exe]
    # the runtimes inside the program where the compiler can put them there (gcc; clang does by default): nothing to load first
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "clatvb host checks passed" in out.stdout
