"""VB / SVI for the stochastic block network without a GPU: the reference (tests/disc_sbmvb_ref.py) against
its brute-force twin, its limits (K = 1 is the Bernoulli step, the closed form of Σω), the monotonicity of the network
part of the bound under coordinate ascent with the margin measured against 50-digit arithmetic, the input on which a
simultaneous update lowers it, saturated inputs, what the package refuses before any device work, and recovery of a
planted two-block network."""
import numpy as np
import pytest

import disc_netvb_ref as nr
import disc_sbmvb_ref as br
import disc_svi_ref as sr


def state(N=7, K=3, seed=0):
    return br.random_blocks(N, K), np.random.default_rng(seed).uniform(0.05, 0.95, (N, N))


def test_the_reference_against_its_brute_force_twin():
    """Loops over p, c, k, l with the literal formulas; rtol 1e-12, the bound of the netvb twins."""
    for N, K in ((4, 1), (5, 2), (7, 3)):
        (m, av, bv, gv), rho = state(N, K)
        assert np.allclose(br.net_term(m, av, bv), br.net_term_brute(m, av, bv), rtol=1e-12, atol=1e-14)
        for got, want in zip(br.tables(br.BPRI, m, rho), br.tables_brute(br.BPRI, m, rho)):
            assert np.allclose(got, want, rtol=1e-12, atol=0.0)
        E = br.expectations(av, bv, gv)
        for n in range(N):
            assert np.allclose(br.node_score(n, m, rho, *E), br.node_score_brute(n, m, rho, av, bv, gv), rtol=1e-12, atol=0.0)
        assert np.isclose(br.network_bound((m, av, bv, gv), rho, br.BPRI), br.network_bound_brute((m, av, bv, gv), rho, br.BPRI),
                          rtol=1e-12, atol=0.0)


def test_one_block_is_the_bernoulli_step():
    N, T, B, L = 5, 700, 3, 7
    data, conv, start = nr.parity_problem(N, T, B, L)
    a, b = 1.7, 2.3
    blk = (np.ones((N, 1)), np.array([[a]]), np.array([[b]]), np.array([1.4]))
    bpri = (nr.PARITY_NET[0], nr.PARITY_NET[1], 0.8)
    want = nr.netvb_step(data, conv, 1.0, nr.PARITY_PRIORS, nr.PARITY_NET, start[:8] + (a, b))
    got, nb = br.sbmvb_step(data, conv, 1.0, nr.PARITY_PRIORS, bpri, start[:8], blk)
    for g, w in zip(got, want[:8]):
        assert np.allclose(g, w, rtol=1e-13, atol=0.0)
    assert np.isclose(nb[1][0, 0], want[8], rtol=1e-13) and np.isclose(nb[2][0, 0], want[9], rtol=1e-13)
    assert np.all(nb[0] == 1.0) and np.isclose(nb[3][0], 0.8 + N, rtol=1e-15)


def test_the_pair_weights_sum_as_in_closed_form():
    """αv + βv - α - β = Σ_pc ω = S_k S_l - Σ_p m[p,k] m[p,l] + δ_kl S_k with S = Σ_n m."""
    (m, _, _, _), rho = state(9, 4)
    av, bv, gv = br.tables(br.BPRI, m, rho)
    S = m.sum(axis=0)
    want = np.outer(S, S) - m.T @ m + np.diag(S)
    assert np.allclose(av + bv - br.BPRI[0] - br.BPRI[1], want, rtol=1e-12, atol=0.0)
    assert np.isclose(want.sum(), 9 * 9, rtol=1e-13)                    # every link carries weight 1


def test_coordinate_ascent_never_lowers_the_network_bound():
    """Random start, N = 7, K = 3: the Beta update, the Dirichlet update and each node's update in turn.  "Does not fall":
    by no more than 4 x the reference's own rounding error in network_bound against 50-digit arithmetic at the states
    compared (1.5e-14 where this was written, the largest over the ten states, on values between -59 and -40; the smallest
    rise was 2.8e-2)."""
    blk, rho = state()
    m, av, bv, gv = blk
    bpri = br.BPRI
    av2, bv2, gv2 = br.tables(bpri, m, rho)
    chain = [(m, av, bv, gv), (m, av2, bv2, gv), (m, av2, bv2, gv2)]
    E = br.expectations(av2, bv2, gv2)
    cur = m.copy()
    for n in range(m.shape[0]):
        cur = cur.copy()
        cur[n] = br.node_update(n, cur, rho, *E)
        chain.append((cur, av2, bv2, gv2))
    vals = [br.network_bound(s, rho, bpri) for s in chain]
    err = max(br.measured_bound_error(s, rho, bpri) for s in chain)
    steps = np.diff(vals)
    print(f"network_bound's own error against 50 digits: {err:.2e}; smallest step {steps.min():.3e}, values {vals[0]:.6f} .. {vals[-1]:.6f}")
    assert err < 1e-12
    assert np.all(steps >= -4 * err)
    assert np.all(steps > 1e-6)                                          # from a random start every update gains


def test_a_simultaneous_update_lowers_the_bound():
    """The check that the monotonicity test can see the difference.  A bipartite ρv (links only across two groups of four),
    tables that favour links inside a block, and a start in which each group leans to its own label: updated all at once
    from the old m every node jumps to its neighbours' label, the two groups swap and the bound FALLS (by 70.8 at the
    first step, measured), then the swap repeats; node after node the same start only rises."""
    N = 8
    g = np.arange(N) % 2
    rho = np.where(g[:, None] != g[None, :], 0.95, 0.05)
    m = np.where(g[:, None] == np.arange(2)[None, :], 0.6, 0.4)
    av, bv, gv = np.array([[9.0, 1.0], [1.0, 9.0]]), np.array([[1.0, 9.0], [9.0, 1.0]]), np.array([5.0, 5.0])
    bpri = (1.0, 1.0, 1.0)
    bound = lambda x: br.network_bound((x, av, bv, gv), rho, bpri)       # noqa: E731
    both = br.simultaneous(m, rho, av, bv, gv)
    print(f"simultaneous: {bound(both) - bound(m):.4f}; sequential: {bound(br.sweep(m, rho, av, bv, gv)) - bound(m):.4f}")
    assert bound(both) < bound(m) - 1.0
    assert bound(br.sweep(m, rho, av, bv, gv)) > bound(m)
    assert np.array_equal(np.argmax(both, axis=1), 1 - g) and np.array_equal(np.argmax(br.simultaneous(both, rho, av, bv, gv), axis=1), g)


def test_saturated_inputs_stay_finite():
    """A one-hot m and a ρv of exact 0s and 1s; scores further than 745 apart give an exact 0 and no NaN."""
    N, K = 6, 3
    m = np.eye(K)[np.arange(N) % K]
    rho = (np.arange(N * N).reshape(N, N) % 2).astype(np.float64)
    mh, av, bv, gv = br.network_update(br.BPRI, (m, None, None, None), rho)
    for x in (mh, av, bv, gv, br.net_term(m, av, bv)):
        assert np.all(np.isfinite(x))
    assert np.allclose(mh.sum(axis=1), 1.0, rtol=0, atol=1e-15) and np.isfinite(br.network_bound((mh, av, bv, gv), rho, br.BPRI))
    out = br.softmax(np.array([0.0, -746.0, -2000.0]))
    assert out[0] == 1.0 and out[1] == 0.0 and out[2] == 0.0
    big = (np.eye(2)[np.arange(40) % 2], np.array([[400.0, 1e-3], [1e-3, 400.0]]), np.array([[1e-3, 400.0], [400.0, 1e-3]]), np.ones(2))
    r40 = np.where((np.arange(40) % 2)[:, None] == (np.arange(40) % 2)[None, :], 1.0, 0.0)
    got = br.sweep(big[0], r40, *big[1:])
    assert np.all(np.isfinite(got)) and np.any(got == 0.0) and np.all(got.sum(axis=1) == 1.0)


def test_a_fresh_block_model_has_no_variational_state(nhp):
    N, B, L = 3, 2, 4
    data = nr.counts(N, 60, 1)
    proc = br.make_process(nhp, N, B, L, 2)
    net = proc.network
    assert net.mv is None and net.αv is None and net.βv is None and net.γv is None
    for call in (lambda: nhp.update_(proc, data, None), lambda: nhp.svi_(proc, data, nsteps=2, batch_bins=32),
                 lambda: nhp.vb_(proc, data, max_steps=1)):
        with pytest.raises(NotImplementedError, match="network.*variational_init_"):
            call()
    n_before = len(proc.variational_params())
    with pytest.raises(ValueError, match="sharpness"):
        net.variational_init_(sharpness=0.0)
    assert net.mv is None
    net.variational_init_()
    assert np.array_equal(net.mv, 0.5 * np.eye(2)[net.z] + 0.25) and np.all(net.αv == net.α) and np.all(net.γv == net.γ)
    assert len(proc.variational_params()) == n_before + 4 + 4 + 2 + N * 2
    j = nhp.StochasticBlockNetworkModel(5, 3).variational_init_(seed=4, sharpness=0.8)
    assert np.allclose(j.mv.sum(axis=1), 1.0, rtol=0, atol=1e-15) and np.array_equal(np.argmax(j.mv, axis=1), j.z)
    lat = nhp.DiscreteNetworkHawkesProcess(proc.baseline, proc.impulses, proc.weights, np.ones((N, N)),
                                           nhp.LatentDistanceNetworkModel(N, 2), 1.0)
    with pytest.raises(NotImplementedError, match="network"):
        nhp.update_(lat, data, None)


def test_recovery_of_a_planted_two_block_network():
    """N = 12, T = 2e4, B = 3, two planted blocks (links with probability 0.9 inside, 0.05 across), start labels that
    alternate, 100 steps with the sweep at every 10th: argmax mv is the planted partition for ALL nodes up to the swap of
    the two labels.  Smallest margin max_k m - 1/2 over the nodes: 0.453 (measured); 142 of 144 links classified."""
    data, A, z, start, params, blk = br.recovery_reference()
    margin = float(np.min(np.max(blk[0], axis=1) - 0.5))
    print(f"smallest margin {margin:.3f}; links classified as planted {int(np.sum((params[7] > 0.5) == (A > 0.5)))} of {A.size}")
    assert not br.same_partition(np.argmax(start[0], axis=1), z)
    assert br.same_partition(np.argmax(blk[0], axis=1), z)
    assert margin > 0.25
    fit = blk[1] / (blk[1] + blk[2])
    print(np.round(fit, 3))
    assert min(fit[0, 0], fit[1, 1]) > max(fit[0, 1], fit[1, 0])         # links are likelier inside a block than across
