"""GPU tests of the continuous latent-distance-network variational fit (csrc/cont_netvb.hip, csrc/nhp_latvb_dev.h,
nhp_cont_latvb_step / _run, nhp_latent_expected_loglik): F and its gradient and one update_ against the numpy/scipy restatement
(tests/clatvb_ref.py), J = 0, the run against its own steps, resuming, trials, device planes, the monotone bound, the refusals
of the C entry points and the planted-network recovery.  Helpers, routes and cases are tests/test_cont_netvb_gpu.py's.

Bounds.  Factor entries (S, R, κv0, νv0, zv, bv, ∇F): the project's TOL = 1e-10.  ELBO pieces, the four network pieces and F
included: TOL_PIECE = 1e-11 relative plus 16 ulp per rounded term of Σ|terms| (clatvb_ref.network_piece_terms / F_terms, η's own
terms b and ‖Δz‖² included).  The link layer: at the tables the device itself wrote and the (zv, bv) it read, ρv within 1 x the
restatement's own rounding error against 50-digit arithmetic (clatvb_ref.measured_logit_error()) and the logit within 4 x that
where 1e-3 < ρv < 1 - 1e-3, plus the rounding of ρv to a double seen through the inverse.  Rungs: F of the rung the device
reports, restated at the device's own ρv, within 16 ulp·Σ|terms| of the restatement's best -- an exact tie may fall either way."""
import ctypes as C

import numpy as np
import pytest

import clatvb_ref as cl
import cnetvb_ref as cr
import disc_netvb_ref as dn
import em_ref as er
import test_cont_netvb_gpu as tn
from helpers import random_case

pytestmark = pytest.mark.gpu

TOL, TOL_PIECE, EPS = tn.TOL, tn.TOL_PIECE, tn.EPS
Q_LATENT = cl.priors()
NET_NAMES = ("entropy", "links", "ln p(z)", "ln p(b)")


def _latent_process(nhp, std, D, q=Q_LATENT, lat=None, J=3, seed=0):
    """The network process on the components of the standard process `std` under a latent distance network with a variational
    state: variational_init_'s (seeded), or `lat` = (zv, bv)."""
    tn._with_priors(std, q)
    N = std.ndims()
    w = nhp.SparseWeightModel(std.weights.W, q["kappa0"], q["nu0"], q["kappa"], q["nu"])
    net = nhp.LatentDistanceNetworkModel(N, D, σ=q["lpri"][0], μb=q["lpri"][1], σb=q["lpri"][2])
    net.variational_init_(seed=seed, ascent_steps=J)
    if lat is not None:
        net.zv, net.bv = np.array(lat[0], dtype=np.float64), float(lat[1])
    return nhp.ContinuousNetworkHawkesProcess(std.baseline, std.impulses, w, np.ones((N, N)), net)


def _state_object(nhp, state, kind, N, D, q, J=3):
    return nhp.ContinuousLatentNetworkVariational(kind, N, *cl.planes(state), D, prior_kappa=q["kappa"], ascent_steps=J)


def _check_network_pieces(got4, got_klnet, lat, rho, lpri, what):
    want, terms = cl.network_pieces(lat, rho, lpri), cl.network_piece_terms(lat, rho, lpri)
    for name, g, w, t in zip(NET_NAMES, got4, want, terms):
        bound = TOL_PIECE * max(1.0, abs(w)) + 16.0 * EPS * t
        print(f"{what} {name}: got {g:.12g} want {w:.12g}, error / bound = {abs(g - w) / bound:.3e}")
        assert abs(g - w) <= bound, (what, name, g, w)
    w = cl.kl_net(lat, rho, lpri)
    bound = TOL_PIECE * max(1.0, abs(w)) + 16.0 * EPS * sum(terms)
    print(f"{what} KL_net: got {got_klnet:.12g} want {w:.12g}, error / bound = {abs(got_klnet - w) / bound:.3e}")
    assert abs(got_klnet - w) <= bound, (what, got_klnet, w)


def _check_first_four(got4, want_state, cnt, T, q, what):
    want4 = cr.pieces(want_state, cnt, T, q)[:4]
    for name, g, w, al in zip(("compensator", "KL_lambda0", "KL_W", "KL_imp"), got4, want4, tn._allowance(dict(want_state, na=1.0, nb=1.0), cnt, T, q)):
        bound = TOL_PIECE * max(1.0, abs(w)) + al
        print(f"{what} {name}: got {g:.12g} want {w:.12g}, error / bound = {abs(g - w) / bound:.3e}")
        assert abs(g - w) <= bound, (what, name, g, w)


def _check_link_layer(got, old_lat, q, what):
    """ρv of the device against the restated logit at the device's own tables, with η of the OLD (zv, bv) as the network term."""
    err = cl.measured_logit_error()
    own = dict(kappa0=got.kappa0, nu0=got.nu0, nu=got.nu)
    lo_want = cl.logit(own, old_lat, q)
    rho = got.rho
    assert np.all(np.isfinite(rho)) and np.all((rho >= 0.0) & (rho <= 1.0))
    d = float(np.max(np.abs(rho - dn.sigmoid(lo_want))))
    inner = (rho > 1e-3) & (rho < 1.0 - 1e-3)
    dl = 0.0
    if inner.any():
        back = 4 * 2.2e-16 / (rho[inner] * (1.0 - rho[inner]))
        gap = np.abs(np.log(rho[inner] / (1.0 - rho[inner])) - lo_want[inner])
        dl = float(gap.max())
        assert np.all(gap <= 4 * err + back), (what, dl, err)
    print(f"{what}: max |Δρv| {d:.2e} (bound {err:.2e}); max |Δlogit| inside {dl:.2e} (bound {4 * err:.2e}); {int(inner.sum())} of {rho.size} inside")
    assert d <= err, (what, d, err)


def _check_factors(got, want, what):
    NN = got.N * got.N
    wS, wR, wQ, _ = cl.planes(want)
    for name, g, w in (("S", got.S, wS), ("R", got.R, wR), ("kappa0, nu0", got.Q[:2 * NN], wQ[:2 * NN])):
        assert g.shape == w.shape and np.all(np.isfinite(g)), (what, name)
        assert tn._ratio(g, w) <= 1.0, (what, name, tn._ratio(g, w))


def _check_rungs_and_replay(got, old_lat, lpri, rungs, what):
    """Every reported rung against the restated ladder at the device's own ρv, and (zv, bv) against the replay with those rungs."""
    z, b = old_lat
    for j, r in enumerate(rungs):
        assert -1 <= r < cl.RUNGS, (what, j, r)
        nz, nb, _, Fs, mags = cl.ascent_iteration(z, b, got.rho, lpri, rung=r)
        best = int(np.argmax(Fs))                                     # (slot 8 is the current point)
        slot = r if r >= 0 else cl.RUNGS
        slack = 16.0 * EPS * (mags[slot] + mags[best])
        print(f"{what} iteration {j}: rung {r} F {Fs[slot]:.12g}, restated best {best if best < cl.RUNGS else -1} F {Fs[best]:.12g}, "
              f"gap / allowance = {(Fs[best] - Fs[slot]) / slack:.3e}")
        assert Fs[slot] >= Fs[best] - slack, (what, j, r, best)
        z, b = nz, nb
    gz = got.positions()
    assert np.all(np.abs(gz - z) <= TOL * np.maximum(1.0, np.abs(z))), (what, float(np.max(np.abs(gz - z))))
    assert abs(got.offset() - b) <= TOL * max(1.0, abs(b)), what


# ---- 1. F and its gradient ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D", [(3, 1), (70, 3), (70, 8), (300, 2), (1, 2)])
def test_expected_loglikelihood_matches_the_restatement(nhp, N, D):
    """Random ρ in [0, 1] with exact 0 and 1 entries (the diagonal too).  N = 70: more than one wave of lanes per node, no multiple
    of 64 or of the transpose tile; N = 300: several tiles and a partial second trip of the 256 lanes; N = 1: the diagonal alone."""
    rng = np.random.default_rng(40 + N + D)
    rho = rng.uniform(size=(N, N))
    rho[0, 0] = 1.0
    if N > 1:
        rho[0, 1], rho[1, 0], rho[N - 1, N - 1], rho[N - 1, 0] = 0.0, 1.0, 0.0, 1.0
    z, b = cl.random_lat(N, D, 3)
    q = Q_LATENT
    net = nhp.LatentDistanceNetworkModel(N, D, z=z, b=b, σ=q["lpri"][0], μb=q["lpri"][1], σb=q["lpri"][2])
    f, gz, gb = net.expected_loglikelihood(rho, gradient=True)
    assert net.expected_loglikelihood(rho) == f
    want, terms = cl.F(z, b, rho, q["lpri"]), cl.F_terms(z, b, rho, q["lpri"])
    bound = TOL_PIECE * max(1.0, abs(want)) + 16.0 * EPS * terms
    wz, wb = cl.grad(z, b, rho, q["lpri"])
    print(f"N={N} D={D}: F got {f:.12g} want {want:.12g}, error / bound = {abs(f - want) / bound:.3e}; "
          f"gradient largest error / bound = {tn._ratio(np.append(gz.ravel(), gb), np.append(wz.ravel(), wb)):.3e}")
    assert abs(f - want) <= bound
    assert gz.shape == (N, D) and np.all(np.abs(gz - wz) <= TOL * np.maximum(1.0, np.abs(wz))) and abs(gb - wb) <= TOL * max(1.0, abs(wb))


# ---- 2. one update_ ------------------------------------------------------------------------------------------------------------

ONE_STEP_CASES = [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)]
ONE_STEP = [c + s for s in cl.SHAPES[:3] for c in ONE_STEP_CASES] + [c + cl.SHAPES[3] for c in ONE_STEP_CASES[:2]]


@pytest.mark.parametrize("kind,dt_max,recursive,N,M,T,D", ONE_STEP)
def test_one_step_matches_the_restatement(nhp, kind, dt_max, recursive, N, M, T, D, monkeypatch):
    """update_ with J = 3 from a random state on both dataset routes.  N = 70: more than one wave of nodes, no multiple of 64 or of
    the transpose tile; D = 8: the largest; N = 300 (exponential only): several tiles and workgroup trips with a partial last one.
    Condition: under the restatement at least half the links have 1e-3 < ρv < 1 - 1e-3 (asserted).  The network pieces of the state
    returned are held at its own (zv, bv) and ρv, (zv, bv) against the restatement replayed with the reported rungs."""
    q, J = Q_LATENT, 3
    case = random_case(N, M, T, kind, dt_max, seed=3, nhp=nhp)
    data = case["data"]
    state = cl.random_state(N, D, kind, 1)
    proc = _latent_process(nhp, case["proc"], D, q, lat=state["lat"], J=J)
    pr = er.Pairs(data[0], data[1], data[2], N, dt_max, recursive=recursive and kind == "exponential")
    model = cr.surrogate(state, dt_max)
    want, loglam, stats = cl.step(model, pr, q, state["lat"], J, exact=N <= 70)
    for route, _ in tn._routes(monkeypatch, nhp, proc, data):
        what = f"{kind} dt_max={dt_max} rec={recursive} N={N} D={D} {route}"
        got = nhp.update_(proc, data, init=_state_object(nhp, state, kind, N, D, q, J), recursive=recursive)
        assert got.ascent_steps == J and got.ndims == D and len(got.pieces["rungs"]) == J
        _check_factors(got, want, what)
        fix = float(pr.T * np.sum(model.lam0) + np.sum(pr.cnt[:, None] * model.W))
        bound = TOL_PIECE * max(1.0, abs(loglam)) + 16.0 * EPS * (abs(stats[0]) + 2.0 * fix)
        assert abs(got.pieces["loglam"] - loglam) <= bound, (what, got.pieces["loglam"], loglam)
        _check_first_four(got.pieces["before"][:4], state, pr.cnt, pr.T, q, what + " before")
        _check_first_four(got.pieces["after"][:4], want, pr.cnt, pr.T, q, what + " after")
        _check_network_pieces(got.pieces["network_before"], got.pieces["before"][4], state["lat"], state["rho"], q["lpri"], what + " before")
        _check_network_pieces(got.pieces["network_after"], got.pieces["after"][4], (got.positions(), got.offset()), got.rho, q["lpri"], what + " after")
        b = got.pieces["before"]
        assert got.elbo == got.pieces["loglam"] - b[0] - b[1] - b[2] - b[3] - b[4]
        _check_link_layer(got, state["lat"], q, what)
        print(f"{what}: rungs {got.pieces['rungs']} (restatement {want['rungs']})")
        _check_rungs_and_replay(got, state["lat"], q["lpri"], got.pieces["rungs"], what)
    inside = np.mean((want["rho"] > 1e-3) & (want["rho"] < 1.0 - 1e-3))
    assert inside >= 0.5, inside


# ---- 3. J = 0 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_no_ascent_returns_the_network_bit_for_bit(nhp, kind):
    """ascent_steps = 0: zv, bv come back bit for bit, no rung is reported, ρv is the restatement's."""
    N, D, q = 9, 3, Q_LATENT
    case = random_case(N, 800, 50.0, kind, 1.5, seed=3, nhp=nhp)
    state = cl.random_state(N, D, kind, 2)
    proc = _latent_process(nhp, case["proc"], D, q, lat=state["lat"], J=0)
    nhp.invalidate_device_datasets()
    got = nhp.update_(proc, case["data"], init=_state_object(nhp, state, kind, N, D, q, 0), recursive=False)
    assert np.array_equal(got.Z, cl.z_vector(state["lat"])) and got.pieces["rungs"] == () and got.ascent_steps == 0
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, 1.5)
    want, _, _ = cl.step(cr.surrogate(state, 1.5), pr, q, state["lat"], 0)
    _check_factors(got, want, f"{kind} J=0")
    _check_link_layer(got, state["lat"], q, f"{kind} J=0")
    _check_network_pieces(got.pieces["network_after"], got.pieces["after"][4], state["lat"], got.rho, q["lpri"], f"{kind} J=0 after")
    # ... and without a state the network's own (zv, bv) are the ones read and returned
    first = nhp.update_(proc, case["data"], recursive=False)
    assert np.array_equal(first.Z, cl.z_vector(state["lat"])) and np.isnan(first.elbo) and first.pieces["network_before"] == (0.0,) * 4


# ---- 4. run, resume, routes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dt_max,recursive", ONE_STEP_CASES)
def test_the_trace_never_falls_and_the_run_is_its_steps(nhp, kind, dt_max, recursive, monkeypatch):
    """N = 7, D = 2, J = 2, 12 updates: min diff(trace) >= -1e-11·|L|; 12 update_ calls reproduce state and trace and two runs agree --
    bit for bit on the fixed-order routes, within TOL otherwise; what vb_ leaves in the process and the network; the first
    restated steps give the same trace."""
    N, D, J, steps, q = 7, 2, 2, 12, Q_LATENT
    exact_rec = tn._fixed_order_recursion(monkeypatch, kind, recursive)
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data, guess = case["data"], case["proc"].params()
    fresh = lambda: _latent_process(nhp, random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"], D, q, J=J)   # noqa: E731

    def same(a, b, exact, what):
        tn._same(a, b, exact, what)
        assert np.array_equal(a.Z, b.Z) if exact else tn._ratio(a.Z, b.Z) <= 1.0, what
    for route, on_slices in tn._routes(monkeypatch, nhp, case["proc"], data):
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        proc = fresh()
        start = proc.network.variational_params().copy()
        res = nhp.vb_(proc, data, max_steps=steps, f_abstol=0.0, guess=guess, recursive=recursive)
        assert res.steps == steps and len(res.trace) == steps and res.elbo == res.trace[-1] and res.ascent_steps == J
        rise = np.diff(res.trace)
        print(f"{kind} dt_max={dt_max} rec={recursive} {route}: L {res.trace[0]:.4f} -> {res.elbo:.6f}, smallest rise {rise.min():.3e}")
        assert np.all(np.isfinite(res.trace)) and rise.min() >= -1e-11 * abs(res.elbo)
        net = proc.network
        assert np.array_equal(tn._device_guess(proc), res.mean()) and np.array_equal(proc.adjacency_matrix, (res.rho > 0.5).astype(float))
        assert np.array_equal(proc.weights.ρv, res.rho) and np.array_equal(net.zv, res.positions()) and net.bv == res.offset()
        assert np.array_equal(net.z, net.zv) and net.b == net.bv and not np.array_equal(res.Z, start)
        again = nhp.vb_(fresh(), data, max_steps=steps, f_abstol=0.0, guess=guess, recursive=recursive)
        same(again, res, exact, (kind, route, "twice"))
        if exact:
            assert np.array_equal(again.trace, res.trace)
        p = fresh()
        std = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"]
        std.params_(guess)
        p.baseline.λ, p.weights.W = std.baseline.λ.copy(), std.weights.W.copy()
        p.impulses.params_(std.impulses.params())
        state, trace = None, []
        for i in range(1, steps + 1):
            state = nhp.update_(p, data, init=state, recursive=recursive)
            trace.append(state.elbo)
            assert np.array_equal(p.network.variational_params(), start)          # update_ does not change the network
        same(state, res, exact, (kind, route, "steps"))
        trace = np.array(trace[1:])
        if exact:
            assert np.array_equal(trace, res.trace[:-1])
        else:
            assert np.max(np.abs(trace - res.trace[:-1]) / np.abs(res.trace[:-1])) <= 1e-10
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, dt_max, recursive=recursive)
    net0 = fresh().network
    _, want, _ = cl.run(er.from_vector(guess, N, kind, dt_max), pr, q, 3, (net0.zv, net0.bv), J, exact=False)
    assert np.max(np.abs(res.trace[:3] - want) / np.maximum(1.0, np.abs(want))) <= 1e-9


def test_resuming_continues_the_run(nhp):
    """init=res: 5 + 5 updates are 10 updates, within TOL (bit for bit is the previous test's matter); the network's state moved."""
    N, D, q = 7, 2, Q_LATENT
    kind, dt_max = "exponential", 1.5
    fresh = lambda: _latent_process(nhp, random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"], D, q, J=2)      # noqa: E731
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data, guess = case["data"], case["proc"].params()
    whole = nhp.vb_(fresh(), data, max_steps=10, f_abstol=0.0, guess=guess)
    p = fresh()
    first = nhp.vb_(p, data, max_steps=5, f_abstol=0.0, guess=guess)
    second = nhp.vb_(p, data, max_steps=5, f_abstol=0.0, init=first)
    assert len(second.trace) == 6 and second.steps == 5
    for g, w in ((second.S, whole.S), (second.R, whole.R), (second.Q, whole.Q), (second.Z, whole.Z)):
        assert tn._ratio(g, w) <= 1.0
    assert np.max(np.abs(second.trace[1:] - whole.trace[5:]) / np.abs(whole.trace[5:])) <= 1e-10
    assert np.array_equal(p.network.zv, second.positions()) and not np.array_equal(first.Z, second.Z)


@pytest.mark.parametrize("kind,recursive", [("exponential", False), ("logitnormal", False)])
def test_two_trials_are_the_sum_of_their_statistics(nhp, kind, recursive):
    """A list of two trials: the restated update on the summed statistics."""
    N, D, dt_max, q, J = 4, 2, 1.5, Q_LATENT, 2
    trials = []
    for s, (M, T) in enumerate(((300, 30.0), (180, 25.0))):
        c = random_case(N, M, T, kind, dt_max, seed=20 + s, nhp=nhp)
        trials.append((c["times"], c["nodes"], T + 1.0))
    state = cl.random_state(N, D, kind, 6)
    proc = _latent_process(nhp, random_case(N, 10, 10.0, kind, dt_max, seed=1, nhp=nhp)["proc"], D, q, lat=state["lat"], J=J)
    model = cr.surrogate(state, dt_max)
    parts = [(er.statistics(model, p), p) for p in (er.Pairs(t, n, T, N, dt_max, recursive=recursive) for t, n, T in trials)]
    summed = [sum(s[i] for s, _ in parts) if parts[0][0][i] is not None else None for i in range(5)]
    cnt, T = sum(p.cnt for _, p in parts), sum(p.T for _, p in parts)
    want = cl.update(model, summed, cnt, T, q, state["lat"], J)
    nhp.invalidate_device_datasets()
    got = nhp.update_(proc, trials, init=_state_object(nhp, state, kind, N, D, q, J), recursive=recursive)
    _check_factors(got, want, f"{kind} trials")
    assert np.all(got.beta == q["beta0"] + T)
    _check_first_four(got.pieces["after"][:4], want, cnt, T, q, f"{kind} trials")
    _check_link_layer(got, state["lat"], q, f"{kind} trials")
    _check_rungs_and_replay(got, state["lat"], q["lpri"], got.pieces["rungs"], f"{kind} trials")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_a_step_on_device_planes_is_the_step_on_host_planes(nhp, kind):
    """output_on_device = 1: S, R, Q and Z are device pointers, read and overwritten; the same numbers as through host arrays
    (within the factor bound: this dataset's route adds with LDS atomics), the same 19 + J scalars likewise."""
    import torch
    from nhp_amd import _lib, inference
    N, D, J, q = 5, 3, 3, Q_LATENT
    case = random_case(N, 600, 60.0, kind, 1.0, seed=8, nhp=nhp)
    st = cl.random_state(N, D, kind, 3)
    proc = _latent_process(nhp, case["proc"], D, q, lat=st["lat"], J=J)
    state = _state_object(nhp, st, kind, N, D, q, J)
    nhp.invalidate_device_datasets()
    host = nhp.update_(proc, case["data"], init=state, recursive=False)
    ctx = nhp.default_context()
    dev = torch.device("cuda", ctx.device)
    dS, dR, dQ, dZ = (torch.as_tensor(v).to(dev) for v in (state.S, state.R, state.Q, state.Z))
    torch.cuda.current_stream(dev).synchronize()
    stats = np.empty(19 + J)
    pr, netp, _ = inference._netvb_check(proc, case["data"], "update!")
    latp = np.array(q["lpri"], dtype=np.float64)
    ds, model = nhp.device_dataset(proc, case["data"], ctx), proc.device_model(ctx)
    _lib.check(_lib.lib().nhp_cont_latvb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), _lib.dptr(netp), _lib.dptr(latp), D, J, dS.data_ptr(),
                                              dR.data_ptr(), len(state.S), dQ.data_ptr(), dZ.data_ptr(), 1, _lib.dptr(stats)), ctx.h)
    for g, w in ((dS.cpu().numpy(), host.S), (dR.cpu().numpy(), host.R), (dQ.cpu().numpy(), host.Q), (dZ.cpu().numpy(), host.Z)):
        assert tn._ratio(g, w) <= 1.0
    want = np.array([host.pieces["loglam"], *host.pieces["before"], *host.pieces["after"], *host.pieces["network_before"],
                     *host.pieces["network_after"]])
    assert np.array_equal(stats[1:6], want[1:6]) and np.array_equal(stats[11:15], want[11:15])      # the state stepped from: no statistics in them
    assert np.max(np.abs(stats[:19] - want) / np.maximum(1.0, np.abs(want))) <= 1e-10
    assert tuple(int(v) for v in stats[19:]) == host.pieces["rungs"]


# ---- 5. the monotone bound ----------------------------------------------------------------------------------------------------

def test_thirty_steps_never_lower_the_bound(nhp):
    """N = 12, D = 2, J = 4, 30 update_ steps from variational_init_'s start: the trace never falls beyond the rounding allowance
    of its terms (-1e-11·|L|, the project's); F restated at each returned (zv, bv) is not below F at the (zv, bv) stepped from,
    both at the returned ρv -- the ρv the ascent ran at -- beyond 16 ulp of F's terms; some rung is taken."""
    N, D, J, q = 12, 2, 4, Q_LATENT
    kind, dt_max = "exponential", 1.5
    case = random_case(N, 3000, 100.0, kind, dt_max, seed=3, nhp=nhp)
    proc = _latent_process(nhp, case["proc"], D, q, J=J)
    nhp.invalidate_device_datasets()
    state, trace, taken = None, [], []
    lat = (proc.network.zv.copy(), proc.network.bv)
    for i in range(31):
        state = nhp.update_(proc, case["data"], init=state, recursive=False)
        trace.append(state.elbo)
        new = (state.positions(), state.offset())
        f_new, f_old = cl.F(new[0], new[1], state.rho, q["lpri"]), cl.F(lat[0], lat[1], state.rho, q["lpri"])
        allow = 16.0 * EPS * (cl.F_terms(new[0], new[1], state.rho, q["lpri"]) + cl.F_terms(lat[0], lat[1], state.rho, q["lpri"]))
        assert f_new >= f_old - allow, (i, f_new, f_old)
        if all(r < 0 for r in state.pieces["rungs"]):
            assert np.array_equal(new[0], lat[0]) and new[1] == lat[1]
        taken += list(state.pieces["rungs"])
        lat = new
    trace = np.array(trace[1:])
    rise = np.diff(trace)
    print(f"L {trace[0]:.4f} -> {trace[-1]:.6f}, smallest rise {rise.min():.3e}; rungs taken {sorted(set(taken))}")
    assert len(trace) == 30 and np.all(np.isfinite(trace)) and rise.min() >= -1e-11 * abs(trace[-1])
    assert max(taken) >= 0 and all(-1 <= r < cl.RUNGS for r in taken)


# ---- 6. refusals of the C entry points ------------------------------------------------------------------------------------------

def test_refusals_of_the_device_entry_points(nhp):
    """nhp_cont_latvb_step / _run themselves: NHP_EINVAL (1) for NULL pointers, D = 0 and 9, J = -1 and 65, a non-finite z or b, σ or
    σb <= 0, a non-finite μb, the dense flag and the state's checks; NHP_ENOTIMPL (6) for a model without A, an LGCP baseline, a
    block network attached and a column shard -- each with a message, and nothing written."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    good = lambda: _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)          # noqa: E731
    N, D0 = 3, 2
    NN = N * N

    def calls(proc, data, net=(0.3, 30.0), lat=(1.3, 0.2, 1.5), D=D0, J=3, flags=0, edit=None, ds_h=None, null=None):
        model = proc.device_model(ctx)
        ds = nhp.device_dataset(proc, data, ctx) if ds_h is None else None
        ds_h = ds.h if ds_h is None else ds_h
        P = N + 2 * NN
        Jb, Db = min(max(J, 0), 64), min(max(D, 1), 8)
        S, R, x, stats = np.full(P, 7.0), np.full(P, 7.0), np.full(P, 0.5), np.full(19 + Jb, 7.0)
        Q = np.concatenate([np.full(2 * NN, 7.0), np.full(NN, 0.5)])
        Z = np.linspace(-0.5, 0.5, N * Db + 1)
        if edit:
            edit(S, R, Q, Z)
        keep = [v.copy() for v in (S, R, Q, Z, x, stats)]
        pr = good()
        netp = None if null == "net" else _lib.dptr(np.array(net, dtype=np.float64))
        latp = None if null == "lat" else _lib.dptr(np.array(lat, dtype=np.float64))
        zp = None if null == "Z" else Z.ctypes.data
        e, st, cv = C.c_double(), C.c_int32(), C.c_int32()
        rc = (lib.nhp_cont_latvb_step(ctx.h, ds_h, model.h, flags, C.byref(pr), netp, latp, D, J, S.ctypes.data, R.ctypes.data, P, Q.ctypes.data, zp, 0,
                                      _lib.dptr(stats)),
              lib.nhp_cont_latvb_run(ctx.h, ds_h, model.h, flags | 256, C.byref(pr), netp, latp, D, J, 1e-6, 5, _lib.dptr(x), _lib.dptr(S),
                                     _lib.dptr(R), P, _lib.dptr(Q), None if null == "Z" else _lib.dptr(Z), C.byref(e), C.byref(st), C.byref(cv), None))
        msg = lib.nhp_last_error(ctx.h)
        assert rc[0] == rc[1] and rc[0] != 0 and msg and len(msg.decode()) > 10, (rc, msg)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, (S, R, Q, Z, x, stats)))
        return rc
    std = random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    net = tn._network(nhp, random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    data = std["data"]
    lgcp = random_case(N, 50, 10.0, "exponential", 1.0, lgcp=True, seed=1, nhp=nhp)
    lgcp_net = nhp.ContinuousNetworkHawkesProcess(lgcp["proc"].baseline, lgcp["proc"].impulses, net.weights, np.ones((N, N)), net.network)
    assert calls(std["proc"], data) == (6, 6) and calls(lgcp_net, lgcp["data"]) == (6, 6)
    blk = tn._network(nhp, random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    rho, pi, z = np.full(4, 0.5), np.full(2, 0.5), np.zeros(N, dtype=np.int32)
    _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, blk.device_model(ctx).h, 2, z.ctypes.data, _lib.dptr(rho), _lib.dptr(pi), 1.0, 1.0, 1.0), ctx.h)
    assert calls(blk, data) == (6, 6)
    for null in ("net", "lat", "Z"):
        assert calls(net, data, null=null) == (1, 1), null
    for bad_D in (0, 9, -1):
        assert calls(net, data, D=bad_D) == (1, 1)
    for bad_J in (-1, 65):
        assert calls(net, data, J=bad_J) == (1, 1)
    assert calls(net, data, flags=1024) == (1, 1)

    def put(plane, at, v):
        def edit(S, R, Q, Z):
            {"S": S, "R": R, "Q": Q, "Z": Z}[plane][at] = v
        return edit
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, N * D0 - 1, N * D0):
            assert calls(net, data, edit=put("Z", at, bad)) == (1, 1), (at, bad)
        assert calls(net, data, lat=(1.3, bad, 1.5)) == (1, 1)
    for bad in (0.0, -1.0, np.nan, np.inf):
        for j in (0, 2):
            s = [1.3, 0.2, 1.5]
            s[j] = bad
            assert calls(net, data, lat=s) == (1, 1), (j, bad)
        for j in range(2):
            s = [0.3, 30.0]
            s[j] = bad
            assert calls(net, data, net=s) == (1, 1), (j, bad)
        for plane, at in (("Q", 0), ("Q", 2 * NN - 1), ("S", N + NN), ("R", N + 2 * NN - 1)):
            assert calls(net, data, edit=put(plane, at, bad)) == (1, 1), (plane, at, bad)
    assert calls(net, data, edit=put("Q", 2 * NN + 4, 1.0 + 1e-9)) == (1, 1)
    # a column shard (the children on nodes 1 and 2 of 3): it would be fitted on its own columns alone
    times, nodes, T = data
    h = C.c_void_p()
    _lib.check(lib.nhp_cont_dataset_create_columns(ctx.h, _lib.dptr(_lib.f64(times)), _lib.iptr(np.ascontiguousarray(nodes, dtype=np.int64)),
                                                   len(times), N, T, 1.0, 0, 2, C.byref(h)), ctx.h)
    try:
        assert calls(net, data, ds_h=h) == (6, 6)
    finally:
        lib.nhp_cont_dataset_destroy(h)
    # nhp_latent_expected_loglik: its own refusals
    rho, zz, out = np.full(NN, 0.5), np.zeros(N * 2), np.full(N * 2 + 2, 7.0)
    latp = np.array([1.3, 0.2, 1.5])
    f = lambda r=rho, n=N, d=2, zv=zz, b=0.1, lp=latp: lib.nhp_latent_expected_loglik(ctx.h, _lib.dptr(r), n, d, _lib.dptr(zv), b, _lib.dptr(lp), _lib.dptr(out))   # noqa: E731
    assert f(d=0) == 1 and f(d=9) == 1 and f(n=0) == 1 and f(b=np.nan) == 1 and f(lp=np.array([0.0, 0.2, 1.5])) == 1
    assert f(r=np.full(NN, 1.5)) == 1 and f(zv=np.full(N * 2, np.inf)) == 1 and np.all(out == 7.0)


# ---- 7. recovery -----------------------------------------------------------------------------------------------------------------

def test_the_planted_network_is_recovered(nhp):
    """clatvb_ref.RECOVERY (N = 12, D = 2, three groups of four at the corners of a triangle, about 8 500 events, 40 steps with
    J = 4 from 0.1·N(0, I) positions).  Under the restatement on the CPU: mean ρv over the planted links 0.9997, over the absent ones
    0.0096, and the correlation of the network's own link probabilities s(η) at (zv, bv) with the planted ones 0.953.  The bar for
    the device is that correlation less 0.05 -- 0.90 -- and the planted mean above the absent one."""
    r = cl.RECOVERY
    times, nodes, T, A, P = cl.recovery_problem()
    N, q = r["N"], cl.priors(r["lpri"], r["spike"])
    std = random_case(N, 5, T, "exponential", r["dt_max"], seed=1, nhp=nhp)["proc"]
    proc = _latent_process(nhp, std, r["D"], q, lat=cl.recovery_start(), J=r["J"])
    nhp.invalidate_device_datasets()
    res = nhp.vb_(proc, (times, nodes, T), max_steps=r["steps"], f_abstol=0.0, guess=cl.recovery_guess(), recursive=False)
    present, absent, corr = cl.recovered(res.rho, res.network_link_probability(), A, P)
    print(f"{len(times)} events, {res.steps} steps: mean rho_v {present:.4f} on the planted links, {absent:.4f} on the absent; "
          f"correlation of s(eta) with the planted probabilities {corr:.3f}; b_v {res.offset():.3f}")
    assert np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo))
    assert present > absent
    assert corr > 0.90
    assert np.array_equal(proc.network.z, res.positions()) and proc.network.b == res.offset()
