"""Network VB / SVI without a GPU: the exports and the errors raised before any device work, the vectorised
reference (tests/disc_netvb_ref.py) against its brute-force twin and against the oracle's dense step, the limits of the
update in the reference itself, the reference's own rounding error in the logit against 50-digit arithmetic (four times
it is the bound of the device logit in tests/test_disc_netvb_gpu.py), and recovery of a sparse truth."""
import numpy as np
import pytest
from scipy.special import digamma

import disc_netvb_ref as nr
import disc_svi_ref as sr


def close(got, want, rtol):
    for g, w in zip(got, want):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape and np.allclose(g, w, rtol=rtol, atol=0.0)


def test_the_exports_exist(nhp):
    from nhp_amd import _lib
    assert callable(nhp.variational_mean_)
    assert hasattr(_lib.lib(), "nhp_disc_netvb_run") and hasattr(_lib.lib(), "nhp_disc_netsvi_run")
    W = np.zeros((3, 3))
    assert nhp.SparseWeightModel(W).ρv is None
    net = nhp.BernoulliNetworkModel(0.3, 3)
    assert (net.αv, net.βv) == (1.0, 1.0)
    p = nr.make_process(nhp, 3, 2, 4, nr.PARITY_PRIORS, nr.PARITY_NET)
    v = p.variational_params()
    assert len(v) == 2 * 3 + 4 * 9 + 9 * 2 + 9 + 2 and np.all(v[-11:-2] == 0.5) and np.all(v[-2:] == 1.0)   # ρv = None: ρ
    d = nr.make_process(nhp, 3, 2, 4, nr.PARITY_PRIORS, None)
    assert len(d.variational_params()) == len(v) - 2 and np.all(d.variational_params()[-9:] == 1.0)


def test_what_is_not_built_says_which_part(nhp):
    N, B, L = 3, 2, 4
    data = nr.counts(N, 60, 1)
    ok = nr.make_process(nhp, N, B, L, nr.PARITY_PRIORS, nr.PARITY_NET)
    dense_w = nhp.DiscreteNetworkHawkesProcess(ok.baseline, ok.impulses, nhp.DenseWeightModel(ok.weights.W), np.ones((N, N)),
                                               ok.network, 1.0)
    G = 5
    lg = nhp.DiscreteLogGaussianCoxProcess(np.linspace(0.0, 60.0, G), np.ones((G, N)), None, 0.0, 1.0)
    lgcp = nhp.DiscreteNetworkHawkesProcess(lg, ok.impulses, ok.weights, np.ones((N, N)), ok.network, 1.0)
    block = nhp.DiscreteNetworkHawkesProcess(ok.baseline, ok.impulses, ok.weights, np.ones((N, N)),
                                             nhp.StochasticBlockNetworkModel(N, 2), 1.0)
    sparse_std = nhp.DiscreteStandardHawkesProcess(ok.baseline, ok.impulses, ok.weights, 1.0)
    for proc, part in ((dense_w, "weights"), (lgcp, "baseline"), (block, "network"), (sparse_std, "standard process")):
        with pytest.raises(NotImplementedError, match=part):
            nhp.update_(proc, data, None)
        with pytest.raises(NotImplementedError, match=part):
            nhp.svi_(proc, data, nsteps=2, batch_bins=32)
        with pytest.raises(NotImplementedError, match=part):
            nhp.vb_(proc, data, max_steps=1)


def test_the_reference_against_its_brute_force_twin():
    N, T, B, L, Tb = 3, 37, 2, 3, 16                                     # three blocks, the last of 5 bins
    data = nr.counts(N, T, 11, rate=0.6)
    dt, priors = 0.5, (1.5, 2.0, 0.4, 9.0, 1.75, 1.25, 0.5)
    conv = nr.convolve(data, sr.basis_brute(L, B, dt))
    assert np.allclose(conv, sr.convolve_brute(data, sr.basis_brute(L, B, dt)), rtol=1e-15, atol=0.0)
    start = nr.random_start(N, B)
    for net in ((1.5, 0.5), None):
        close(nr.netvb_step(data, conv, dt, priors, net, start), nr.netvb_step_brute(data, L, dt, priors, net, start), 1e-12)
        for j, i in ((0, 1), (1, 4), (2, 9)):
            close(nr.netsvi_step(data, conv, dt, priors, net, start, j, Tb, i, 1.0, 0.7),
                  nr.netsvi_step_brute(data, L, dt, priors, net, start, j, Tb, i, 1.0, 0.7), 1e-12)


def test_the_limits_in_the_reference(orc):
    N, T, B, L = 3, 50, 2, 4
    data = nr.counts(N, T, 4)
    conv = orc.disc_convolve(data, orc.disc_basis(L, B, 1.0))
    assert np.allclose(conv, nr.convolve(data, sr.basis_brute(L, B, 1.0)), rtol=1e-13, atol=1e-300)
    s = nr.random_start(N, B)
    # dense network, slab prior = the dense prior: the oracle's dense step on (αv, βv, κv1, νv1, γv), ρv ≡ 1
    priors = (1.0, 1.0, 0.3, 7.0, 1.25, 0.75, 1.0)
    got = nr.netvb_step(data, conv, 1.0, priors, None, s[:7] + (np.ones((N, N)),) + s[8:])
    want = orc.disc_vb_step(data, conv, 1.0, 1.0, 1.0, 1.25, 0.75, 1.0, s[0], s[1], s[4], s[5], s[6])
    close((got[0], got[1], got[4], got[5], got[6]), want, 1e-12)
    assert np.all(got[7] == 1.0) and got[8:] == s[8:]
    # symmetric priors: every ρv is sigmoid(ψ(αv) - ψ(βv)) of the OLD network parameters; α = β and αv = βv give 1/2
    sym = (1.0, 1.0, 0.8, 2.0, 0.8, 2.0, 1.0)
    got = nr.netvb_step(data, conv, 1.0, sym, (2.0, 3.0), s)
    assert np.allclose(got[7], nr.sigmoid(digamma(s[8]) - digamma(s[9])), rtol=1e-14, atol=0.0)
    assert np.isclose(got[8], 2.0 + got[7].sum(), rtol=1e-15) and np.isclose(got[9], 3.0 + (1.0 - got[7]).sum(), rtol=1e-15)
    got = nr.netvb_step(data, conv, 1.0, sym, (2.0, 2.0), s[:8] + (1.7, 1.7))
    assert np.all(got[7] == 0.5)
    # a parent without events: its rows stay at the priors and its logit is the network term alone
    quiet = data.copy()
    quiet[1] = 0
    qconv = orc.disc_convolve(quiet, orc.disc_basis(L, B, 1.0))
    got = nr.netvb_step(quiet, qconv, 1.0, priors, (2.0, 3.0), s)
    assert np.all(got[2][1] == 0.3) and np.all(got[4][1] == 1.25) and np.all(got[3][1] == 7.0) and np.all(got[5][1] == 0.75)
    assert np.allclose(got[7][1], nr.sigmoid(digamma(s[8]) - digamma(s[9])), rtol=1e-13, atol=0.0)
    assert all(np.all(np.isfinite(np.asarray(g))) for g in got)
    # ρv of exact 0s and 1s, and a logit far past saturation: exactly 0 or 1, never NaN
    hard = s[:7] + ((np.arange(N * N).reshape(N, N) % 2).astype(np.float64),) + s[8:]
    assert all(np.all(np.isfinite(np.asarray(g))) for g in nr.netvb_step(data, conv, 1.0, priors, (2.0, 3.0), hard))
    assert np.array_equal(nr.sigmoid(np.array([-800.0, 800.0, 0.0])), [0.0, 1.0, 0.5])
    # one block, delay 0, forgetting 1, step 1 is one update!
    close(nr.netsvi_step(data, conv, 1.0, priors, (2.0, 3.0), s, 0, T, 1, 0.0, 1.0),
          nr.netvb_step(data, conv, 1.0, priors, (2.0, 3.0), s), 1e-14)


def test_the_lgamma_difference_does_not_cancel():
    """At κv ≈ 1e6 the two lgammas are 1.3e7 each and their library difference carries 1e-9 of rounding; the form inside
    Stirling's formula stays at the 1e-15 of its result, on both sides of the switch at 16."""
    import mpmath as mp
    mp.mp.dps = 50
    for x, d in ((1.0e6 + 0.37, 1.5), (16.0, 1.5), (15.99, 1.5), (40.0, -23.5), (3.0e4, 700.25), (0.3, 0.2)):
        want = float(mp.loggamma(mp.mpf(x) + mp.mpf(d)) - mp.loggamma(mp.mpf(x)))
        got = float(nr.lgamma_diff(np.array([x]), d)[0])
        print(f"x = {x}, d = {d}: error {abs(got - want):.2e} of {want:.6g}")
        assert abs(got - want) <= 4e-15 * max(1.0, abs(want)) + 64 * 2.2e-16     # 64 ulp of 1: two library lgammas near 28


def test_the_rounding_error_of_the_reference_logit():
    """max |logit - 50-digit logit| over all links of the parity shapes, after the first and the sixth step.  Measured
    8.9e-15 (at (5, 700, 3, 7), where κv0 reaches 63 and the logit's terms 60); the terms are at most a few hundred and
    each carries a few ulp, so anything above 1e-12 would mean the formula cancels after all."""
    err = nr.measured_logit_error()
    print(f"reference logit: largest error against 50 digits {err:.3e}; device bound 4x = {4 * err:.3e}, ρv bound {err:.3e}")
    assert 0.0 < err < 1e-12


def test_recovery_of_a_sparse_truth():
    """With the spike Gamma(1, 50) (mean 0.02), the slab Gamma(2, 4) and 30 steps from the all-ones start the reference
    puts ρv > 0.5 on each of the 8 true links (W from 0.12 to 0.28) and ρv < 0.5 on each of the 8 absent ones: 16 of 16."""
    r = nr.RECOVERY
    data, A, W = nr.simulate_sparse(r["N"], r["T"], r["B"], r["L"], r["seed"])
    assert 0 < A.sum() < A.size and W[A > 0].min() >= 0.1 and np.all(W[A == 0] == 0.0)
    conv = nr.convolve(data, sr.basis_brute(r["L"], r["B"], 1.0))
    got = nr.netvb_run(data, conv, 1.0, r["priors"], r["net"], nr.ones_start(r["N"], r["B"]), r["steps"])
    rho = got[7]
    print(np.round(rho, 3), A, f"smallest |ρv - 1/2| = {np.min(np.abs(rho - 0.5)):.3f}", sep="\n")
    assert np.array_equal(rho > 0.5, A > 0.5)
    assert np.isclose(got[8], 1.0 + rho.sum()) and np.isclose(got[9], 1.0 + (1.0 - rho).sum())
