"""GPU tests of the continuous block-network variational fit (csrc/cont_netvb.hip, nhp_cont_sbmvb_step / _run): one update_
against the numpy/scipy restatement (tests/csbmvb_ref.py), K = 1 against the Bernoulli fit, the run against its own steps,
resuming, edge shapes, trials, device planes, the refusals of the C entry points, the planted-partition recovery and the example.  Helpers, routes and cases are tests/test_cont_netvb_gpu.py's.

Bounds.  Factor entries (S, R, κv0, νv0, αv, βv, γv, m): the project's TOL = 1e-10.  ELBO pieces, the five network pieces
included: TOL_PIECE = 1e-11 relative plus 16 ulp per rounded term of Σ|terms| (csbmvb_ref.network_piece_terms).  The link
layer: at the tables the device itself wrote and the block state it read, ρv within 1 x the restatement's own rounding error
against 50-digit arithmetic (csbmvb_ref.measured_logit_error()) and the logit within 4 x that where 1e-3 < ρv < 1 - 1e-3,
plus the rounding of ρv to a double seen through the inverse."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

import cnetvb_ref as cr
import csbmvb_ref as cb
import disc_netvb_ref as dn
import disc_sbmvb_ref as sb
import em_ref as er
import test_cont_netvb_gpu as tn
from helpers import random_case

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

TOL, TOL_PIECE, EPS = tn.TOL, tn.TOL_PIECE, tn.EPS
Q_BLOCK = cb.priors()
NET_NAMES = ("entropy", "links", "labels", "KL_Dir", "KL_Beta")


def _block_process(nhp, std, K, q=Q_BLOCK, blk=None, labels_every=1, seed=2):
    """The network process on the components of the standard process `std` under a block network with a variational state:
    variational_init_'s (seeded), or `blk`."""
    tn._with_priors(std, q)
    N = std.ndims()
    w = nhp.SparseWeightModel(std.weights.W, q["kappa0"], q["nu0"], q["kappa"], q["nu"])
    net = nhp.StochasticBlockNetworkModel(N, K, α=q["bpri"][0], β=q["bpri"][1], γ=q["bpri"][2])
    net.variational_init_(seed=seed, sharpness=0.3, labels_every=labels_every)
    if blk is not None:
        net.mv, net.αv, net.βv, net.γv = (np.array(v, dtype=np.float64) for v in blk)
    return nhp.ContinuousNetworkHawkesProcess(std.baseline, std.impulses, w, np.ones((N, N)), net)


def _state_object(nhp, state, kind, N, K, q, vb_step=0, labels_every=1):
    return nhp.ContinuousBlockNetworkVariational(kind, N, *cb.planes(state), K, prior_kappa=q["kappa"], vb_step=vb_step, labels_every=labels_every)


def _check_network_pieces(got5, got_klnet, blk, rho, bpri, what):
    want, terms = cb.network_pieces(blk, rho, bpri), cb.network_piece_terms(blk, rho, bpri)
    for name, g, w, t in zip(NET_NAMES, got5, want, terms):
        bound = TOL_PIECE * max(1.0, abs(w)) + 16.0 * EPS * t
        print(f"{what} {name}: got {g:.12g} want {w:.12g}, error / bound = {abs(g - w) / bound:.3e}")
        assert abs(g - w) <= bound, (what, name, g, w)
    w = cb.kl_net(blk, rho, bpri)
    bound = TOL_PIECE * max(1.0, abs(w)) + 16.0 * EPS * sum(terms)
    print(f"{what} KL_net: got {got_klnet:.12g} want {w:.12g}, error / bound = {abs(got_klnet - w) / bound:.3e}")
    assert abs(got_klnet - w) <= bound, (what, got_klnet, w)


def _check_first_four(got4, want_state, cnt, T, q, what):
    want4 = cr.pieces(want_state, cnt, T, q)[:4]
    for name, g, w, al in zip(("compensator", "KL_lambda0", "KL_W", "KL_imp"), got4, want4, tn._allowance(dict(want_state, na=1.0, nb=1.0), cnt, T, q)):
        bound = TOL_PIECE * max(1.0, abs(w)) + al
        print(f"{what} {name}: got {g:.12g} want {w:.12g}, error / bound = {abs(g - w) / bound:.3e}")
        assert abs(g - w) <= bound, (what, name, g, w)


def _check_link_layer(got, old_blk, q, what):
    err = cb.measured_logit_error()
    own = dict(kappa0=got.kappa0, nu0=got.nu0, nu=got.nu)
    lo_want = cb.logit(own, old_blk, q)
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


def _check_state(got, want, what):
    NN = got.N * got.N
    wS, wR, wQ, wB = cb.planes(want)
    for name, g, w in (("S", got.S, wS), ("R", got.R, wR), ("kappa0, nu0", got.Q[:2 * NN], wQ[:2 * NN]), ("B", got.B, wB)):
        assert g.shape == w.shape and np.all(np.isfinite(g)), (what, name)
        assert tn._ratio(g, w) <= 1.0, (what, name, tn._ratio(g, w))


ONE_STEP_CASES = [("exponential", 1.5, False), ("exponential", np.inf, True), ("logitnormal", 1.5, False)]
ONE_STEP = [c + s for s in cb.SHAPES[:3] for c in ONE_STEP_CASES] + [c + cb.SHAPES[3] for c in ONE_STEP_CASES[:2]]


@pytest.mark.parametrize("kind,dt_max,recursive,N,M,T,K", ONE_STEP)
def test_one_step_matches_the_restatement(nhp, kind, dt_max, recursive, N, M, T, K, monkeypatch):
    """update_ from a random state with a sweep (step 1, labels_every = 1) on both dataset routes.  N = 70: more than one wave of
    nodes, P no multiple of 256; K = 3, 5: padded lanes in the sweep; N = 300 (exponential only): the sweep's NPT = 4
    instantiation with a partial last trip.  Condition: under the restatement at least half the links have
    1e-3 < ρv < 1 - 1e-3 (asserted)."""
    q = Q_BLOCK
    case = random_case(N, M, T, kind, dt_max, seed=3, nhp=nhp)
    data = case["data"]
    state = cb.random_state(N, K, kind, 1)
    proc = _block_process(nhp, case["proc"], K, q, blk=state["blk"])
    pr = er.Pairs(data[0], data[1], data[2], N, dt_max, recursive=recursive and kind == "exponential")
    model = cr.surrogate(state, dt_max)
    want, loglam, stats = cb.step(model, pr, q, state["blk"], True, exact=N <= 70)
    for route, _ in tn._routes(monkeypatch, nhp, proc, data):
        what = f"{kind} dt_max={dt_max} rec={recursive} N={N} K={K} {route}"
        got = nhp.update_(proc, data, init=_state_object(nhp, state, kind, N, K, q), recursive=recursive)
        assert got.vb_step == 1
        _check_state(got, want, what)
        fix = float(pr.T * np.sum(model.lam0) + np.sum(pr.cnt[:, None] * model.W))
        bound = TOL_PIECE * max(1.0, abs(loglam)) + 16.0 * EPS * (abs(stats[0]) + 2.0 * fix)
        assert abs(got.pieces["loglam"] - loglam) <= bound, (what, got.pieces["loglam"], loglam)
        _check_first_four(got.pieces["before"][:4], state, pr.cnt, pr.T, q, what + " before")
        _check_first_four(got.pieces["after"][:4], want, pr.cnt, pr.T, q, what + " after")
        _check_network_pieces(got.pieces["network_before"], got.pieces["before"][4], state["blk"], state["rho"], q["bpri"], what + " before")
        _check_network_pieces(got.pieces["network_after"], got.pieces["after"][4], want["blk"], want["rho"], q["bpri"], what + " after")
        b = got.pieces["before"]
        assert got.elbo == got.pieces["loglam"] - b[0] - b[1] - b[2] - b[3] - b[4]
        _check_link_layer(got, state["blk"], q, what)
        # B at the device's OWN ρv: the tables and the sweep of the restatement from it
        own = sb.network_update(q["bpri"], state["blk"], got.rho, True)
        for name, g, w in zip(("m", "alpha_v", "beta_v", "gamma_v"), (got.mv, got.alpha_v, got.beta_v, got.gamma_v), own):
            assert tn._ratio(g, w) <= 1.0, (what, name)
        assert np.all(np.abs(got.mv.sum(axis=1) - 1.0) <= 1e-12)
    inside = np.mean((want["rho"] > 1e-3) & (want["rho"] < 1.0 - 1e-3))
    assert inside >= 0.5, inside


def test_one_block_is_the_bernoulli_fit(nhp):
    """K = 1: five steps against vb_ on the same process with a BernoulliNetworkModel (same α, β, start (αv, βv) = (α, β)).  State
    within TOL, trace within 1e-10 relative."""
    N, q = 7, Q_BLOCK
    for kind, dt_max in (("exponential", 1.5), ("logitnormal", 1.5)):
        fresh = lambda: random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)        # noqa: E731
        data, guess = fresh()["data"], fresh()["proc"].params()
        qb = cr.priors(net=q["bpri"][:2])
        want = nhp.vb_(tn._network(nhp, fresh()["proc"], qb, start=q["bpri"][:2]), data, max_steps=5, f_abstol=0.0, guess=guess)
        blocks = _block_process(nhp, fresh()["proc"], 1, q, seed=None)
        got = nhp.vb_(blocks, data, max_steps=5, f_abstol=0.0, guess=guess)
        NN = N * N
        assert got.steps == 5 and np.all(got.mv == 1.0) and blocks.network.vb_step == 5
        for g, w in ((got.S, want.S), (got.R, want.R), (got.Q, want.Q[:3 * NN]), (got.alpha_v.ravel(), [want.net_alpha]),
                     (got.beta_v.ravel(), [want.net_beta])):
            assert tn._ratio(np.asarray(g), np.asarray(w)) <= 1.0, kind
        assert got.gamma_v[0] == q["bpri"][2] + N
        assert np.max(np.abs(got.trace - want.trace) / np.abs(want.trace)) <= 1e-10, kind


@pytest.mark.parametrize("labels_every", [1, 3])
@pytest.mark.parametrize("kind,dt_max,recursive", ONE_STEP_CASES)
def test_the_trace_never_falls_and_the_run_is_its_steps(nhp, kind, dt_max, recursive, labels_every, monkeypatch):
    """N = 7, K = 2, 25 updates: min diff(trace) >= -1e-11·|L|; 25 update_ calls reproduce state and trace and two runs agree -- bit
    for bit on the fixed-order routes, within TOL otherwise; mv is bit-identical across steps without a sweep; what vb_
    leaves in the process and the network."""
    N, K, steps, q = 7, 2, 25, Q_BLOCK
    exact_rec = tn._fixed_order_recursion(monkeypatch, kind, recursive)
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data, guess = case["data"], case["proc"].params()
    fresh = lambda: _block_process(nhp, random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"], K, q, labels_every=labels_every)   # noqa: E731

    def same(a, b, exact, what):
        tn._same(a, b, exact, what)
        return [np.array_equal(a.B, b.B) if exact else tn._ratio(a.B, b.B) <= 1.0]
    for route, on_slices in tn._routes(monkeypatch, nhp, case["proc"], data):
        exact = exact_rec or (on_slices and kind == "exponential" and not recursive)
        proc = fresh()
        res = nhp.vb_(proc, data, max_steps=steps, f_abstol=0.0, guess=guess, recursive=recursive)
        assert res.steps == steps and len(res.trace) == steps and res.elbo == res.trace[-1] and res.vb_step == steps
        rise = np.diff(res.trace)
        print(f"{kind} dt_max={dt_max} rec={recursive} every={labels_every} {route}: L {res.trace[0]:.4f} -> {res.elbo:.6f}, smallest rise {rise.min():.3e}")
        assert np.all(np.isfinite(res.trace)) and rise.min() >= -1e-11 * abs(res.elbo)
        net = proc.network
        assert np.array_equal(tn._device_guess(proc), res.mean()) and np.array_equal(proc.adjacency_matrix, (res.rho > 0.5).astype(float))
        assert np.array_equal(proc.weights.ρv, res.rho) and np.array_equal(net.mv, res.mv) and np.array_equal(net.αv, res.alpha_v)
        assert np.array_equal(net.βv, res.beta_v) and np.array_equal(net.γv, res.gamma_v) and net.vb_step == steps
        assert np.array_equal(net.ρ, res.alpha_v / (res.alpha_v + res.beta_v)) and np.array_equal(net.π, res.gamma_v / res.gamma_v.sum())
        assert np.array_equal(net.z, res.labels()) and np.array_equal(res.labels(), np.argmax(res.mv, axis=1))
        again = nhp.vb_(fresh(), data, max_steps=steps, f_abstol=0.0, guess=guess, recursive=recursive)
        assert all(same(again, res, exact, (kind, route, "twice")))
        if exact:
            assert np.array_equal(again.trace, res.trace)
        p = fresh()
        std = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"]
        std.params_(guess)
        p.baseline.λ, p.weights.W = std.baseline.λ.copy(), std.weights.W.copy()
        p.impulses.params_(std.impulses.params())
        state, trace, before = None, [], p.network.mv.copy()
        for i in range(1, steps + 1):
            state = nhp.update_(p, data, init=state, recursive=recursive)
            trace.append(state.elbo)
            assert state.vb_step == i and p.network.vb_step == 0
            if i % labels_every != 0:
                assert np.array_equal(state.mv, before), i
            before = state.mv.copy()
        assert all(same(state, res, exact, (kind, route, "steps")))
        trace = np.array(trace[1:])
        if exact:
            assert np.array_equal(trace, res.trace[:-1])
        else:
            assert np.max(np.abs(trace - res.trace[:-1]) / np.abs(res.trace[:-1])) <= 1e-10
    # the first restated steps from the same guess and block state: the same trace
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, dt_max, recursive=recursive)
    net0 = fresh().network
    _, want = cb.run(er.from_vector(guess, N, kind, dt_max), pr, q, 3, (net0.mv, net0.αv, net0.βv, net0.γv), labels_every, exact=False)
    assert np.max(np.abs(res.trace[:3] - want) / np.maximum(1.0, np.abs(want))) <= 1e-9


def test_resuming_carries_the_step_count(nhp):
    """init=res: 6 + 6 updates are 12 updates with labels_every = 4 (sweeps at steps 4, 8, 12: the second leg's schedule needs the
    first leg's count), within TOL (bit for bit is the previous test's matter)."""
    N, K, q = 7, 2, Q_BLOCK
    kind, dt_max = "exponential", 1.5
    fresh = lambda: _block_process(nhp, random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)["proc"], K, q, labels_every=4)      # noqa: E731
    case = random_case(N, 1500, 80.0, kind, dt_max, seed=3, nhp=nhp)
    data, guess = case["data"], case["proc"].params()
    whole = nhp.vb_(fresh(), data, max_steps=12, f_abstol=0.0, guess=guess)
    p = fresh()
    first = nhp.vb_(p, data, max_steps=6, f_abstol=0.0, guess=guess)
    assert first.vb_step == 6 and p.network.vb_step == 6
    second = nhp.vb_(p, data, max_steps=6, f_abstol=0.0, init=first)
    assert second.vb_step == 12 and p.network.vb_step == 12 and len(second.trace) == 7
    for g, w in ((second.S, whole.S), (second.R, whole.R), (second.Q, whole.Q), (second.B, whole.B)):
        assert tn._ratio(g, w) <= 1.0
    assert np.max(np.abs(second.trace[1:] - whole.trace[6:]) / np.abs(whole.trace[6:])) <= 1e-10
    assert not np.array_equal(first.mv, fresh().network.mv)           # (step 4 swept)


def test_edges(nhp):
    """M = 0, M = 1, a node without events, N = 1, and a state with ρv exactly 0 and 1 and a row of mv with an exact 0: nothing
    is NaN, and 0·ln 0 = 0 in both entropies (the pieces equal the restatement's)."""
    q = Q_BLOCK
    for N, K, times, nodes in ((3, 2, [], []), (3, 2, [4.0], [2]), (4, 3, np.linspace(0.5, 9.5, 40), np.tile([1, 2, 4], 14)[:40]), (1, 2, [1.0, 2.0, 2.5], [1, 1, 1])):
        data = (np.asarray(times, float), np.asarray(nodes, np.int64), 10.0)
        proc = _block_process(nhp, random_case(N, 5, 10.0, "exponential", 1.5, seed=1, nhp=nhp)["proc"], K, q)
        nhp.invalidate_device_datasets()
        res = nhp.vb_(proc, data, max_steps=4, f_abstol=0.0)
        for v in (res.S, res.R, res.Q, res.B, res.trace):
            assert np.all(np.isfinite(v)), (N, len(times))
        assert np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo)) and np.all(np.abs(res.mv.sum(axis=1) - 1.0) <= 1e-12)
    N, K, kind, dt_max = 5, 2, "exponential", 1.5
    case = random_case(N, 400, 40.0, kind, dt_max, seed=3, nhp=nhp)
    state = cb.random_state(N, K, kind, 1)
    state["rho"][0, 1], state["rho"][2, 2], state["rho"][3, 0] = 0.0, 1.0, 1.0
    m = state["blk"][0].copy()
    m[1] = [0.0, 1.0]
    m[2] = [0.5, 0.5]                                                 # a tie: labels() takes the lowest index
    state["blk"] = (m,) + state["blk"][1:]
    proc = _block_process(nhp, case["proc"], K, q, blk=state["blk"])
    obj = _state_object(nhp, state, kind, N, K, q)
    assert obj.labels()[2] == 0 and obj.labels()[1] == 1
    nhp.invalidate_device_datasets()
    got = nhp.update_(proc, case["data"], init=obj, recursive=False)
    assert all(np.all(np.isfinite(v)) for v in (got.S, got.R, got.Q, got.B)) and np.isfinite(got.elbo)
    _check_network_pieces(got.pieces["network_before"], got.pieces["before"][4], state["blk"], state["rho"], q["bpri"], "edges before")
    pr = er.Pairs(case["times"], case["nodes"], case["T"], N, dt_max)
    want, _, _ = cb.step(cr.surrogate(state, dt_max), pr, q, state["blk"], True)
    _check_state(got, want, "edges")


@pytest.mark.parametrize("kind,recursive", [("exponential", False), ("exponential", True), ("logitnormal", False)])
def test_three_trials_are_the_sum_of_their_statistics(nhp, kind, recursive):
    """tests/test_cont_netvb_gpu.py's three trials under the block network: the restated update on the summed statistics."""
    N, K, dt_max, q = 4, 2, 1.5, Q_BLOCK
    trials = []
    for s, (M, T) in enumerate(((300, 30.0), (180, 25.0), (40, 12.0))):
        c = random_case(N, M, T, kind, dt_max, seed=20 + s, nhp=nhp)
        trials.append((c["times"] + (0.0 if not recursive else 1e-3), c["nodes"], T + 1.0))
    state = cb.random_state(N, K, kind, 6)
    proc = _block_process(nhp, random_case(N, 10, 10.0, kind, dt_max, seed=1, nhp=nhp)["proc"], K, q, blk=state["blk"])
    model = cr.surrogate(state, dt_max)
    parts = [(er.statistics(model, p), p) for p in (er.Pairs(t, n, T, N, dt_max, recursive=recursive) for t, n, T in trials)]
    summed = [sum(s[i] for s, _ in parts) if parts[0][0][i] is not None else None for i in range(5)]
    cnt, T = sum(p.cnt for _, p in parts), sum(p.T for _, p in parts)
    want = cb.update(model, summed, cnt, T, q, state["blk"], True)
    nhp.invalidate_device_datasets()
    got = nhp.update_(proc, trials, init=_state_object(nhp, state, kind, N, K, q), recursive=recursive)
    _check_state(got, want, f"{kind} trials rec={recursive}")
    assert np.all(got.beta == q["beta0"] + T)
    _check_first_four(got.pieces["after"][:4], want, cnt, T, q, f"{kind} trials")
    _check_network_pieces(got.pieces["network_after"], got.pieces["after"][4], want["blk"], want["rho"], q["bpri"], f"{kind} trials")
    _check_link_layer(got, state["blk"], q, f"{kind} trials")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_a_step_on_device_planes_is_the_step_on_host_planes(nhp, kind):
    """output_on_device = 1: S, R, Q and B are device pointers, read and overwritten; the same numbers as through host arrays
    (within the factor bound: this dataset's route adds with LDS atomics), the same 21 scalars likewise."""
    import torch
    from nhp_amd import _lib, inference
    N, K, q = 5, 3, Q_BLOCK
    case = random_case(N, 600, 60.0, kind, 1.0, seed=8, nhp=nhp)
    st = cb.random_state(N, K, kind, 3)
    proc = _block_process(nhp, case["proc"], K, q, blk=st["blk"])
    state = _state_object(nhp, st, kind, N, K, q)
    nhp.invalidate_device_datasets()
    host = nhp.update_(proc, case["data"], init=state, recursive=False)
    ctx = nhp.default_context()
    dev = torch.device("cuda", ctx.device)
    dS, dR, dQ, dB = (torch.as_tensor(v).to(dev) for v in (state.S, state.R, state.Q, state.B))
    torch.cuda.current_stream(dev).synchronize()
    stats = np.empty(21)
    pr, netp, _ = inference._netvb_check(proc, case["data"], "update!")
    sbm = np.array(q["bpri"], dtype=np.float64)
    ds, model = nhp.device_dataset(proc, case["data"], ctx), proc.device_model(ctx)
    _lib.check(_lib.lib().nhp_cont_sbmvb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), _lib.dptr(netp), _lib.dptr(sbm), K, 1, 0, dS.data_ptr(),
                                              dR.data_ptr(), len(state.S), dQ.data_ptr(), dB.data_ptr(), 1, _lib.dptr(stats)), ctx.h)
    for g, w in ((dS.cpu().numpy(), host.S), (dR.cpu().numpy(), host.R), (dQ.cpu().numpy(), host.Q), (dB.cpu().numpy(), host.B)):
        assert tn._ratio(g, w) <= 1.0
    want = np.array([host.pieces["loglam"], *host.pieces["before"], *host.pieces["after"], *host.pieces["network_before"],
                     *host.pieces["network_after"]])
    assert np.array_equal(stats[1:6], want[1:6]) and np.array_equal(stats[11:16], want[11:16])      # the state stepped from: no statistics in them
    assert np.max(np.abs(stats - want) / np.maximum(1.0, np.abs(want))) <= 1e-10


def test_refusals_of_the_device_entry_points(nhp):
    """nhp_cont_sbmvb_step / _run themselves: NHP_ENOTIMPL (6) for a model without A, an LGCP baseline, a latent distance network
    and a sweep that does not fit in LDS; NHP_EINVAL (1) for K outside 1..64, labels_every < 1, priors, tables or rows of m that
    cannot be, the dense flag and the state's checks -- and nothing written."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    good = lambda: _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)          # noqa: E731
    N, K = 3, 2
    NN = N * N

    def calls(proc, data, pr=None, net=(0.3, 30.0), sbm=(1.5, 2.5, 1.2), K=K, every=1, flags=0, edit=None, n=N, ds_h=None):
        model = proc.device_model(ctx)
        ds = nhp.device_dataset(proc, data, ctx) if ds_h is None else None
        ds_h = ds.h if ds_h is None else ds_h
        P = n + 2 * n * n
        S, R, x, stats = np.full(P, 7.0), np.full(P, 7.0), np.full(P, 0.5), np.full(21, 7.0)
        Q = np.concatenate([np.full(2 * n * n, 7.0), np.full(n * n, 0.5)])
        Kb = min(max(K, 1), 64)
        B = np.concatenate([np.full(2 * Kb * Kb + Kb, 2.0), np.full(n * Kb, 1.0 / Kb)])
        if edit:
            edit(S, R, Q, B)
        keep = [v.copy() for v in (S, R, Q, B, x, stats)]
        pr = good() if pr is None else pr
        netp, sbmp = np.array(net, dtype=np.float64), np.array(sbm, dtype=np.float64)
        e, st, cv = C.c_double(), C.c_int32(), C.c_int32()
        rc = (lib.nhp_cont_sbmvb_step(ctx.h, ds_h, model.h, flags, C.byref(pr), _lib.dptr(netp), _lib.dptr(sbmp), K, every, 0, S.ctypes.data,
                                      R.ctypes.data, P, Q.ctypes.data, B.ctypes.data, 0, _lib.dptr(stats)),
              lib.nhp_cont_sbmvb_run(ctx.h, ds_h, model.h, flags | 256, C.byref(pr), _lib.dptr(netp), _lib.dptr(sbmp), K, every, 0, 1e-6, 5,
                                     _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P, _lib.dptr(Q), _lib.dptr(B), C.byref(e), C.byref(st),
                                     C.byref(cv), None))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, (S, R, Q, B, x, stats)))
        return rc
    std = random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    net = tn._network(nhp, random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    data = std["data"]
    lgcp = random_case(N, 50, 10.0, "exponential", 1.0, lgcp=True, seed=1, nhp=nhp)
    lgcp_net = nhp.ContinuousNetworkHawkesProcess(lgcp["proc"].baseline, lgcp["proc"].impulses, net.weights, np.ones((N, N)), net.network)
    assert calls(std["proc"], data) == (6, 6) and calls(lgcp_net, lgcp["data"]) == (6, 6)
    lat = tn._network(nhp, random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    _lib.check(lib.nhp_cont_model_set_latent(ctx.h, lat.device_model(ctx).h, 2, _lib.dptr(_lib.colmajor(np.zeros((N, 2)))), 0.1, 1.0, 0.0, 1.0),
               ctx.h)
    assert calls(lat, data) == (6, 6)
    big = 400                                                         # 8·(400·64 + ...) bytes of LDS: more than a CU has
    wide = tn._network(nhp, random_case(big, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)["proc"])
    assert calls(wide, random_case(big, 50, 10.0, "exponential", 1.0, seed=1)["data"], K=64, n=big) == (6, 6)
    for bad_K in (0, -1, 65):
        assert calls(net, data, K=bad_K) == (1, 1)
    assert calls(net, data, every=0) == (1, 1) and calls(net, data, flags=1024) == (1, 1)
    for bad in (0.0, -1.0, np.nan, np.inf):
        for j in range(3):
            s = [1.5, 2.5, 1.2]
            s[j] = bad
            assert calls(net, data, sbm=s) == (1, 1), (j, bad)
        for j in range(2):
            s = [0.3, 30.0]
            s[j] = bad
            assert calls(net, data, net=s) == (1, 1), (j, bad)

        def put(plane, at, v):
            def edit(S, R, Q, B):
                {"S": S, "R": R, "Q": Q, "B": B}[plane][at] = v
            return edit
        for plane, at in (("B", 0), ("B", 2 * K * K - 1), ("B", 2 * K * K), ("Q", 0), ("Q", 2 * NN - 1), ("S", N + NN), ("R", N + 2 * NN - 1)):
            assert calls(net, data, edit=put(plane, at, bad)) == (1, 1), (plane, at, bad)
    assert calls(net, data, edit=put("B", 2 * K * K + K, 0.5 + 1e-9)) == (1, 1)       # a row of m off the simplex
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


def test_a_refused_step_leaves_the_host_planes_alone(nhp):
    """nhp_cont_sbmvb_step itself on host planes, N = 2 and three events, from a state whose baseline shapes are 1e-300: the
    surrogate λ̃0 = exp(ψ(α') - log β') underflows to zero, the first event has no parent, so its intensity is zero:
    NHP_EDOMAIN (2), and S, R, Q, B are byte for byte what was passed in."""
    from nhp_amd import _lib
    lib, ctx = _lib.lib(), nhp.default_context()
    N, K = 2, 2
    NN = N * N
    case = random_case(N, 3, 2.0, "exponential", 1.0, seed=1, nhp=nhp)
    proc = tn._network(nhp, case["proc"])
    P = N + 2 * NN
    S, R, stats = np.full(P, 2.0), np.full(P, 1.5), np.full(21, 7.0)
    Q = np.concatenate([np.full(NN, 0.5), np.full(NN, 20.0), np.full(NN, 0.5)])
    B = np.concatenate([np.full(2 * K * K + K, 2.0), np.full(N * K, 1.0 / K)])
    S[:N] = 1e-300
    keep = S.tobytes(), R.tobytes(), Q.tobytes(), B.tobytes()
    pr = _lib.GibbsPriors(2.0, 1.5, 1.5, 2.0, 2.0, 0.7, 0.0, 1.0)
    netp, sbmp = np.array([0.3, 30.0]), np.array([1.5, 2.5, 1.2])
    ds, model = nhp.device_dataset(proc, case["data"], ctx), proc.device_model(ctx)
    rc = lib.nhp_cont_sbmvb_step(ctx.h, ds.h, model.h, 0, C.byref(pr), _lib.dptr(netp), _lib.dptr(sbmp), K, 1, 0, S.ctypes.data, R.ctypes.data, P,
                                 Q.ctypes.data, B.ctypes.data, 0, _lib.dptr(stats))
    assert rc == 2
    assert (S.tobytes(), R.tobytes(), Q.tobytes(), B.tobytes()) == keep


def test_the_planted_partition_is_recovered(nhp):
    """csbmvb_ref.RECOVERY (N = 12, K = 2, dense within, sparse across; the restatement meets the same assertions on the CPU):
    labels() is the planted partition up to relabelling, ρv > ½ on more than 90 % of the planted links and < ½ on more than
    90 % of the absent ones."""
    r = cb.RECOVERY
    times, nodes, T, A, z = cb.recovery_problem()
    N, q = r["N"], cb.priors(r["bpri"], r["spike"])
    std = random_case(N, 5, T, "exponential", r["dt_max"], seed=1, nhp=nhp)["proc"]
    proc = _block_process(nhp, std, 2, q, blk=cb.recovery_start(), labels_every=r["labels_every"])
    nhp.invalidate_device_datasets()
    res = nhp.vb_(proc, (times, nodes, T), max_steps=r["steps"], f_abstol=0.0, guess=cb.recovery_guess(), recursive=False)
    same, present, absent = cb.recovered(res.mv, res.rho, A, z)
    print(f"{len(times)} events, {res.steps} steps: labels {res.labels()}; rho_v > 1/2 on {present:.3f} of the planted links, < 1/2 on {absent:.3f} of the absent")
    assert np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo))
    assert same and present > 0.9 and absent > 0.9
    assert np.array_equal(proc.network.z, res.labels())


def test_the_example_runs():
    z, A, res = importlib.import_module("continuous_exponential_block_network_hawkes_vb").main()
    assert np.all(np.isfinite(res.trace)) and np.all(np.diff(res.trace) >= -1e-11 * abs(res.elbo))
    labels = res.labels()
    assert np.array_equal(labels, z) or np.array_equal(1 - labels, z)
    assert np.mean(res.rho[A == 1.0] > 0.5) > 0.9 and np.mean(res.rho[A == 0.0] < 0.5) > 0.9
