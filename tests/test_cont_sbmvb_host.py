"""CPU tests of the continuous block-network variational fit: the restatement (tests/csbmvb_ref.py) against brute-force
p, c, k, l loops and its 50-digit twins, its trace, the K = 1 reduction to the Bernoulli restatement, the Python refusals
(before any device work), the result class, the planted-partition inputs of the GPU recovery test and the restatement's
own piece error."""
import math

import numpy as np
import pytest

import cnetvb_ref as cr
import csbmvb_ref as cb
import disc_sbmvb_ref as sb
import em_ref as er
from helpers import random_case


def test_the_restatement_against_brute_force_loops():
    """N = 4, K = 2: the logit's network term, the tables, the sweep's scores and the network pieces against explicit loops; the
    pieces against their 50-digit twin; links + labels - KL_Dir - ΣKL_Beta is disc_sbmvb_ref.network_bound."""
    N, K = 4, 2
    state, pr, new, _, _ = cb.parity_problem(N, 200, 20.0, K, "exponential", 1.5)
    q = cb.priors()
    m, av, bv, gv = state["blk"]
    assert np.allclose(sb.net_term(m, av, bv), sb.net_term_brute(m, av, bv), rtol=0, atol=1e-13)
    assert np.max(np.abs(cb.logit(new, state["blk"], q) - cb.logit_mp(new, state["blk"], q))) <= 1e-13
    nm, nav, nbv, ngv = new["blk"]
    bav, bbv, bgv = sb.tables_brute(q["bpri"], m, new["rho"])
    assert np.allclose(nav, bav, rtol=1e-13) and np.allclose(nbv, bbv, rtol=1e-13) and np.allclose(ngv, bgv, rtol=1e-13)
    cur = m.copy()
    for n in range(N):                                                # the sweep: each node reads the current m of the others
        s = sb.node_score_brute(n, cur, new["rho"], nav, nbv, ngv)
        cur[n] = sb.softmax(s)
    assert np.allclose(cur, nm, rtol=0, atol=1e-13)
    for st in (state, new):
        got = cb.network_pieces(st["blk"], st["rho"], q["bpri"])
        assert np.allclose(got, cb.network_pieces_mp(st["blk"], st["rho"], q["bpri"]), rtol=1e-13, atol=1e-13)
        bound = got[1] + got[2] - got[3] - got[4]
        assert abs(bound - sb.network_bound_brute(st["blk"], st["rho"], q["bpri"])) <= 1e-12 * max(1.0, abs(bound))
        assert abs(bound - sb.network_bound(st["blk"], st["rho"], q["bpri"])) <= 1e-12 * max(1.0, abs(bound))
        assert cb.pieces(st, pr.cnt, pr.T, q)[4] == got[0] - bound
    # 0·ln 0 = 0 in both entropies
    rho = new["rho"].copy()
    rho[0, 1], rho[2, 2] = 0.0, 1.0
    m0 = nm.copy()
    m0[1] = [0.0, 1.0]
    assert all(math.isfinite(v) for v in cb.network_pieces((m0, nav, nbv, ngv), rho, q["bpri"]))


@pytest.mark.parametrize("labels_every", [1, 3])
def test_the_restated_trace_never_falls(labels_every):
    N, K, q = 7, 2, cb.priors()
    c = random_case(N, 600, 60.0, "exponential", 1.5, seed=3)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, 1.5)
    guess = er.Model(np.full(N, 1.0), np.full((N, N), 0.1), 1.5, theta=np.full((N, N), 2.0))
    start = sb.init_blocks(np.arange(N) % 2, K, q["bpri"], 0.3, 2)
    state, trace = cb.run(guess, pr, q, 30, start, labels_every, exact=False)
    assert len(trace) == 30 and np.all(np.isfinite(trace)) and np.diff(trace).min() >= -1e-11 * abs(trace[-1])
    assert np.all(np.abs(state["blk"][0].sum(axis=1) - 1.0) <= 1e-12)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_one_block_is_the_bernoulli_restatement(kind):
    """K = 1: m ≡ 1, Eπ = 0, KL_Dir = 0 -- state and trace of five steps equal cnetvb_ref.run within 1e-12."""
    N, steps = 5, 5
    c = random_case(N, 400, 40.0, kind, 1.5, seed=3)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, 1.5)
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(0.5, 1.5, N)] + ([rng.uniform(1.0, 3.0, N * N)] if kind == "exponential"
                                                     else [rng.normal(0.0, 1.0, N * N), rng.uniform(0.5, 2.0, N * N)])
                       + [rng.uniform(0.05, 0.3, N * N)])
    a, b, g = cb.BPRI
    start = (np.ones((N, 1)), np.full((1, 1), a), np.full((1, 1), b), np.full(1, g))
    got, tg = cb.run(er.from_vector(x, N, kind, 1.5), pr, cb.priors(), steps, start, exact=False)
    want, tw = cr.run(er.from_vector(x, N, kind, 1.5), pr, cr.priors(net=(a, b)), steps, a, b, exact=False)
    assert np.max(np.abs(tg - tw) / np.abs(tw)) <= 1e-12
    for key in ("alpha", "beta", "kappa", "nu", "kappa0", "nu0", "rho", "a", "b"):
        assert np.allclose(got[key], want[key], rtol=1e-12, atol=0), key
    m, av, bv, gv = got["blk"]
    assert np.all(m == 1.0) and abs(av[0, 0] - want["na"]) <= 1e-12 * want["na"] and abs(bv[0, 0] - want["nb"]) <= 1e-12 * want["nb"]
    assert gv[0] == g + N


def test_the_restatement_recovers_the_planted_partition():
    """The condition on the inputs of the GPU recovery test: the restatement alone meets its assertions."""
    times, nodes, T, A, z, state = cb.recovery_reference()
    same, present, absent = cb.recovered(state["blk"][0], state["rho"], A, z)
    print(f"{len(times)} events; labels recovered {same}; rho_v > 1/2 on {present:.3f} of the planted links, < 1/2 on {absent:.3f} of the absent ones")
    assert same and present > 0.9 and absent > 0.9


def test_the_restatement_own_piece_error_is_far_below_the_piece_bound():
    """The five network pieces against their 50-digit twin on the GPU shapes: at most a tenth of TOL_PIECE = 1e-11 (relative to
    max(1, |piece|)), so the bound the GPU tests hold the device to is not spent on the reference."""
    err = cb.measured_piece_errors()
    print("own error of (entropy, links, labels, KL_Dir, KL_Beta):", err)
    assert np.all(err <= 1e-12)


def _process(nhp, network, N=3):
    std = random_case(N, 50, 10.0, "exponential", 1.0, seed=1, nhp=nhp)
    w = nhp.SparseWeightModel(std["proc"].weights.W, 0.3, 30.0, 1.5, 2.0)
    return nhp.ContinuousNetworkHawkesProcess(std["proc"].baseline, std["proc"].impulses, w, np.ones((N, N)), network), std["data"]


def test_python_refusals_are_raised_before_any_device_work(nhp):
    N = 3
    for fn in (nhp.vb_, nhp.update_):
        with pytest.raises(NotImplementedError, match=r"StochasticBlockNetworkModel.*variational_init_\(\)"):
            fn(*_process(nhp, nhp.StochasticBlockNetworkModel(N, 2)))
        for name in ("α", "β", "γ"):
            for bad in (0.0, -1.0, np.nan, np.inf):
                net = nhp.StochasticBlockNetworkModel(N, 2).variational_init_(seed=1)
                setattr(net, name, bad)
                with pytest.raises(ValueError, match="network"):
                    fn(*_process(nhp, net))
        net = nhp.StochasticBlockNetworkModel(N, 2).variational_init_(seed=1)
        net.mv = net.mv[:2]
        with pytest.raises(ValueError, match="mv"):
            fn(*_process(nhp, net))
        net = nhp.StochasticBlockNetworkModel(N, 2).variational_init_(seed=1)
        proc, data = _process(nhp, net)
        with pytest.raises(TypeError, match="ContinuousBlockNetworkVariational"):
            fn(proc, data, init=object())
        with pytest.raises(NotImplementedError, match="shard"):
            fn(proc, object.__new__(nhp.ShardedDataset))


def test_the_result_class(nhp):
    N, K, kind = 4, 3, "exponential"
    state = cb.random_state(N, K, kind, 1)
    m = state["blk"][0].copy()
    m[2] = [0.4, 0.4, 0.2]                                            # a tie: the lowest index
    state["blk"] = (m,) + state["blk"][1:]
    S, R, Q, B = cb.planes(state)
    res = nhp.ContinuousBlockNetworkVariational(kind, N, S, R, Q, B, K, prior_kappa=1.5, vb_step=7, labels_every=3)
    assert isinstance(res, nhp.ContinuousNetworkVariational) and res.vb_step == 7 and res.labels_every == 3 and res.nblocks == K
    assert np.array_equal(res.mv, m) and np.array_equal(res.alpha_v, state["blk"][1]) and np.array_equal(res.beta_v, state["blk"][2])
    assert np.array_equal(res.gamma_v, state["blk"][3]) and np.array_equal(res.rho, state["rho"]) and np.array_equal(res.kappa0, state["kappa0"])
    assert np.array_equal(res.link_probability(), state["rho"]) and res.labels()[2] == 0 and res.labels().dtype == np.int32
    assert np.array_equal(res.labels(), np.argmax(m, axis=1))
    assert np.array_equal(res.block_link_probability(), state["blk"][1] / (state["blk"][1] + state["blk"][2]))
    assert res.net_alpha is None and res.net_beta is None and res.pieces is None
    net = nhp.StochasticBlockNetworkModel(N, K)
    net.mv, net.αv, net.βv, net.γv = state["blk"]
    assert np.array_equal(net.variational_params(), B)
    with pytest.raises(ValueError, match="3·N²"):
        nhp.ContinuousBlockNetworkVariational(kind, N, S, R, np.concatenate([Q, [1.0, 1.0]]), B, K)
    with pytest.raises(ValueError, match="2·K²"):
        nhp.ContinuousBlockNetworkVariational(kind, N, S, R, Q, B[:-1], K)
