"""Network VB / SVI on the GPU (nhp_disc_netvb_run, nhp_disc_netsvi_run) against tests/disc_netvb_ref.py.

Bounds.  The tables the step inherits from the dense one (αv, βv, κv0, νv0, κv1, νv1, γv) are held to what
tests/test_disc_svi_gpu.py holds a dense step to: rtol 1e-10 / atol 1e-12 after one step, rtol 1e-9 after six.  The logit
is held to 4 x the reference's own rounding error against 50-digit arithmetic (nr.measured_logit_error(), 8.9e-15 where
it was written) and ρv to 0.25 x that, at the SAME inputs: the reference logit is evaluated at the κv0, νv0, νv1 the device
wrote and at the network parameters the device read, so the comparison sees the per-link layer alone.  The network's
αv, βv are held to N² x the ρv bound against α + Σρv of the device's own ρv.  Against the reference's whole trajectory ρv
inherits the tables' bound through the logit's slope: |Δlogit| <= |ψ(κv1) - ψ(κv0) - log(νv1/νv0)| |Δκv0| +
ψ'(αv)|Δαv| + ψ'(βv)|Δβv| with the Δ's at the tables' rtol, plus the logit bound; `rho_bound` writes that out."""
import importlib
import os
import sys

import numpy as np
import pytest
from scipy.special import digamma, polygamma

import disc_netvb_ref as nr
import disc_svi_ref as sr

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

PRI, NET, WP = nr.PARITY_PRIORS, nr.PARITY_NET, nr.PARITY_PRIORS[2:6]
TABLES = slice(0, 7)


def problem(nhp, N, T, B, L, net=NET, priors=PRI):
    data, conv, start = nr.parity_problem(N, T, B, L)
    proc = nr.make_process(nhp, N, B, L, priors, net, seed=N)
    return proc, data, conv, start


def copy_of(params):
    return tuple(np.array(p, dtype=np.float64, copy=True) if np.ndim(p) else float(p) for p in params)


def worst(got, want):
    return max(float(np.max(np.abs(np.asarray(g) - np.asarray(w)) / np.abs(np.asarray(w)))) for g, w in zip(got, want))


def rho_bound(new, old_net, eps, atol, logit_tol):
    """The bound on |Δρv| against the reference's trajectory (module docstring); `new` the reference's new parameters,
    old_net the network parameters its last step read, eps / atol the tables' bound."""
    k0, n0, k1, n1 = new[2], new[3], new[4], new[5]
    slope = np.abs(digamma(k1) - digamma(k0) - np.log(n1 / n0))
    dnet = (polygamma(1, old_net[0]) * old_net[0] + polygamma(1, old_net[1]) * old_net[1]) * eps
    return 0.25 * (slope * (eps * k0 + atol) + dnet + logit_tol)


def check_link_layer(got, net_read, label):
    """ρv and the network parameters of the device against the reference logit at the device's own tables."""
    err = nr.measured_logit_error()
    want = nr.sigmoid(nr.logit(float(digamma(net_read[0]) - digamma(net_read[1])), WP, got[2], got[3], got[5]))
    d = float(np.max(np.abs(got[7] - want)))
    N2 = got[7].size
    da = abs(got[8] - (NET[0] + float(np.sum(got[7])))), abs(got[9] - (NET[1] + float(np.sum(1.0 - got[7]))))
    print(f"{label}: max |Δρv| {d:.2e} (bound {err:.2e}, logit bound {4 * err:.2e}); network |Δαv| {da[0]:.2e} |Δβv| {da[1]:.2e} "
          f"(bound {N2 * err:.2e})")
    assert d <= err
    inner = (got[7] > 1e-3) & (got[7] < 1.0 - 1e-3)                         # where ρv still determines its logit
    if inner.any():
        lo_got = np.log(got[7][inner] / (1.0 - got[7][inner]))
        lo_want = nr.logit(float(digamma(net_read[0]) - digamma(net_read[1])), WP, got[2], got[3], got[5])[inner]
        back = 4 * 2.2e-16 / (got[7][inner] * (1.0 - got[7][inner]))         # rounding ρv to a double, seen through the inverse
        dl = np.abs(lo_got - lo_want)
        print(f"{label}: max |Δlogit| where 1e-3 < ρv < 1 - 1e-3: {float(dl.max()):.2e}")
        assert np.all(dl <= 4 * err + back)
    assert max(da) <= N2 * err


_REF = {}


def reference(key, data, conv, start):
    if key not in _REF:
        one = nr.netvb_step(data, conv, 1.0, PRI, NET, start)
        five = nr.netvb_run(data, conv, 1.0, PRI, NET, one, 4)
        _REF[key] = (one, five, nr.netvb_step(data, conv, 1.0, PRI, NET, five))
    return _REF[key]


@pytest.mark.parametrize("N,T,B,L", nr.PARITY)
def test_parity_with_the_reference(nhp, N, T, B, L):
    """(3, 50, 2, 4); (5, 700, 3, 7): N² is less than one workgroup; (130, 300, 2, 3): N crosses the 128-column tile and the
    ρv partials span 67 workgroups.  Measured maxima over the three shapes: tables 1.2e-15 (one step) and 3.7e-15 (six steps)
    relative; |Δρv| at the device's own tables 4.7e-16 against the bound 8.9e-15; |Δlogit| 6.2e-15 against 3.6e-14."""
    proc, data, conv, start = problem(nhp, N, T, B, L)
    ds = nhp.convolve(proc, data)
    want1, want5, want6 = reference((N, T, B, L), data, conv, start)
    err = nr.measured_logit_error()
    nr.put(proc, start)
    v = nhp.update_(proc, data, ds)
    got = copy_of(nr.get(proc))
    assert len(v) == 2 * N + 4 * N * N + N * N * B + N * N + 2 and np.array_equal(v[-2:], [got[8], got[9]])
    print(f"one step: largest relative difference of the tables {worst(got[TABLES], want1[TABLES]):.2e}")
    for g, w in zip(got[TABLES], want1[TABLES]):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)
    check_link_layer(got, start[8:], "one step")
    b = rho_bound(want1, start[8:], 1e-10, 1e-12, 4 * err)
    print(f"one step: max |Δρv| against the trajectory {float(np.max(np.abs(got[7] - want1[7]))):.2e} (bound up to {float(b.max()):.2e})")
    assert np.all(np.abs(got[7] - want1[7]) <= b)
    assert abs(got[8] - want1[8]) <= b.sum() and abs(got[9] - want1[9]) <= b.sum()
    # six chained steps: five resident ones, then the sixth from the state the device holds
    nr.put(proc, start)
    nhp.update_(proc, data, ds, n_steps=5)
    got5 = copy_of(nr.get(proc))
    nhp.update_(proc, data, ds)
    got6 = copy_of(nr.get(proc))
    print(f"six steps: largest relative difference of the tables {worst(got6[TABLES], want6[TABLES]):.2e}")
    for g, w in zip(got6[TABLES], want6[TABLES]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    check_link_layer(got6, got5[8:], "sixth step")
    b = rho_bound(want6, want5[8:], 1e-9, 0.0, 4 * err)
    print(f"six steps: max |Δρv| against the trajectory {float(np.max(np.abs(got6[7] - want6[7]))):.2e} (bound up to {float(b.max()):.2e})")
    assert np.all(np.abs(got6[7] - want6[7]) <= b)
    assert abs(got6[8] - want6[8]) <= b.sum() and abs(got6[9] - want6[9]) <= b.sum()


@pytest.mark.parametrize("N,T,B,L", [(5, 700, 3, 7), (130, 300, 2, 3)])
def test_the_dense_limit_is_the_dense_step(nhp, N, T, B, L):
    """DenseNetworkModel and (κ1, ν1) = (κ, ν): ρv ≡ 1 exactly and (αv, βv, κv1, νv1, γv) are update_ on the standard process."""
    proc, data, conv, start = problem(nhp, N, T, B, L, net=None)
    std = nr.make_process(nhp, N, B, L, PRI, None, seed=N, standard=True)
    ds = nhp.convolve(proc, data)
    for steps in (1, 3):
        nr.put(proc, start)
        std.baseline.αv, std.baseline.βv, std.weights.κv, std.weights.νv, std.impulses.γv = copy_of((start[0], start[1], start[4], start[5], start[6]))
        v = nhp.update_(proc, data, ds, n_steps=steps)
        nhp.update_(std, data, ds, n_steps=steps)
        got = nr.get(proc)
        want = (std.baseline.αv, std.baseline.βv, std.weights.κv, std.weights.νv, std.impulses.γv)
        mine = (got[0], got[1], got[4], got[5], got[6])
        print(f"{steps} step(s): bits equal: {all(np.array_equal(g, w) for g, w in zip(mine, want))}; largest relative difference {worst(mine, want):.2e}")
        for g, w in zip(mine, want):
            assert np.allclose(g, w, rtol=1e-13, atol=0.0)
        assert np.all(got[7] == 1.0) and len(v) == 2 * N + 4 * N * N + N * N * B + N * N
        assert np.allclose(got[2], PRI[2] + (got[4] - PRI[4]), rtol=1e-12) and np.allclose(got[3], PRI[3] + (got[5] - PRI[5]), rtol=1e-12)


@pytest.mark.parametrize("N,T,B,L,Tb", [(5, 700, 3, 7, 128), (130, 300, 2, 3, 112)])
def test_the_dense_limit_is_the_dense_step_under_svi(nhp, N, T, B, L, Tb):
    """The same limit through svi_: three blended steps (first block, the short last block, the second), resident and
    streamed, leave ρv ≡ 1 and (αv, βv, κv1, νv1, γv) those of svi_ on the standard process, to the rounding of the blend
    (the compiler fuses the two finish kernels' blends kernel by kernel: not the same bits, where the VB twin above has them)."""
    proc, data, conv, start = problem(nhp, N, T, B, L, net=None)
    std = nr.make_process(nhp, N, B, L, PRI, None, seed=N, standard=True)
    nb = sr.n_blocks(T, Tb)
    assert T % Tb != 0
    kw = dict(nsteps=3, blocks=np.array([0, nb - 1, min(1, nb - 1)], dtype=np.int32), batch_bins=Tb, delay=1.0, forgetting=0.6)
    for streamed, arg in ((False, nhp.convolve(proc, data)), (True, data)):
        nr.put(proc, start)
        std.baseline.αv, std.baseline.βv, std.weights.κv, std.weights.νv, std.impulses.γv = copy_of((start[0], start[1], start[4], start[5], start[6]))
        nhp.svi_(proc, arg, streamed=streamed, **kw)
        nhp.svi_(std, arg, streamed=streamed, **kw)
        got = nr.get(proc)
        want = (std.baseline.αv, std.baseline.βv, std.weights.κv, std.weights.νv, std.impulses.γv)
        mine = (got[0], got[1], got[4], got[5], got[6])
        print(f"streamed={streamed}: bits equal: {all(np.array_equal(g, w) for g, w in zip(mine, want))}; largest relative difference {worst(mine, want):.2e}")
        for g, w in zip(mine, want):
            assert np.allclose(g, w, rtol=1e-13, atol=0.0)
        assert np.all(got[7] == 1.0)


def test_symmetric_priors(nhp):
    N, T, B, L = 5, 700, 3, 7
    sym = (1.0, 1.0, 0.8, 2.0, 0.8, 2.0, 1.0)
    proc, data, conv, start = problem(nhp, N, T, B, L, priors=sym)
    ds = nhp.convolve(proc, data)
    nr.put(proc, start)
    nhp.update_(proc, data, ds)
    got = nr.get(proc)
    assert np.allclose(got[7], nr.sigmoid(digamma(start[8]) - digamma(start[9])), rtol=1e-12, atol=0.0)
    assert np.array_equal(got[2], got[4]) and np.array_equal(got[3], got[5])
    proc = nr.make_process(nhp, N, B, L, sym, (2.0, 2.0), seed=N)
    nr.put(proc, start[:8] + (1.7, 1.7))
    nhp.update_(proc, data, ds)
    assert np.all(nr.get(proc)[7] == 0.5)
    assert nr.get(proc)[8] == 2.0 + 0.5 * N * N and nr.get(proc)[9] == 2.0 + 0.5 * N * N


def test_a_parent_without_events_and_saturated_starts(nhp):
    N, T, B, L = 5, 700, 3, 7
    proc, data, conv, start = problem(nhp, N, T, B, L)
    data = data.copy()
    data[1] = 0
    ds = nhp.convolve(proc, data)
    nr.put(proc, start)
    nhp.update_(proc, data, ds)
    got = copy_of(nr.get(proc))
    assert all(np.all(np.isfinite(np.asarray(g))) for g in got)
    assert np.all(got[2][1] == PRI[2]) and np.all(got[4][1] == PRI[4]) and np.all(got[3][1] == PRI[3]) and np.all(got[5][1] == PRI[5])
    # the prior terms of the logit cancel in exact arithmetic: the row is the symmetric-prior value, to the logit's bound
    err = nr.measured_logit_error()
    assert np.all(np.abs(got[7][1] - nr.sigmoid(digamma(start[8]) - digamma(start[9]))) <= err)
    check_link_layer(got, start[8:], "quiet parent")
    # a start whose ρv holds exact 0s and 1s
    hard = start[:7] + ((np.arange(N * N).reshape(N, N) % 2).astype(np.float64),) + start[8:]
    nr.put(proc, hard)
    nhp.update_(proc, data, ds, n_steps=2)
    got = copy_of(nr.get(proc))
    assert all(np.all(np.isfinite(np.asarray(g))) for g in got) and np.all((got[7] >= 0.0) & (got[7] <= 1.0))
    want = nr.netvb_run(data, nr.convolve(data, sr.basis_brute(L, B, 1.0)), 1.0, PRI, NET, hard, 2)
    for g, w in zip(got[TABLES], want[TABLES]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    # priors under which every link of a parent with events saturates: exactly 0 (logit near -1e4) or 1, nothing NaN
    for priors, value in (((1.0, 1.0, 1.0, 1e6, 2000.0, 1.0, 1.0), 0.0), ((1.0, 1.0, 2000.0, 1.0, 1.0, 1e6, 1.0), 1.0)):
        proc = nr.make_process(nhp, N, B, L, priors, NET, seed=N)
        nr.put(proc, start)
        nhp.update_(proc, data, ds)
        got = nr.get(proc)
        assert all(np.all(np.isfinite(np.asarray(g))) for g in got)
        assert np.all(np.delete(got[7], 1, axis=0) == value) and np.all((got[7][1] > 0.0) & (got[7][1] < 1.0))
    with pytest.raises(Exception, match="rho_v|ρv"):
        nr.put(proc, start[:7] + (np.full((N, N), 1.5),) + start[8:])
        nhp.update_(proc, data, ds)


def test_reproducible_and_resident(nhp):
    N, T, B, L = 130, 300, 2, 3
    proc, data, conv, start = problem(nhp, N, T, B, L)
    ds = nhp.convolve(proc, data)
    runs = []
    for _ in range(2):
        nr.put(proc, start)
        nhp.update_(proc, data, ds, n_steps=5)
        runs.append(copy_of(nr.get(proc)))
    nr.put(proc, start)
    for _ in range(5):
        nhp.update_(proc, data, ds)
    runs.append(copy_of(nr.get(proc)))
    for other in runs[1:]:
        for g, w in zip(other, runs[0]):
            assert np.array_equal(g, w)


def six_blocks(nb):
    return np.array([0, nb - 1, min(1, nb - 1), nb - 1, 0, 0], dtype=np.int32)


@pytest.mark.parametrize("N,T,B,L", [(5, 700, 3, 7), (130, 300, 2, 3)])
def test_svi_one_block_and_no_delay_is_update(nhp, N, T, B, L):
    proc, data, conv, start = problem(nhp, N, T, B, L)
    ds = nhp.convolve(proc, data)
    nr.put(proc, start)
    nhp.update_(proc, data, ds)
    want = copy_of(nr.get(proc))
    nr.put(proc, start)
    res = nhp.svi_(proc, ds, nsteps=1, batch_bins=T, delay=0.0, forgetting=1.0)
    assert res.step == 1 and len(res.trace) == 1 and len(res.trace[0]) == 2 * N + 4 * N * N + N * N * B + N * N + 2
    for g, w in zip(nr.get(proc), want):
        assert np.allclose(g, w, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("N,T,B,L,Tb", [(5, 700, 3, 7, 128), (130, 300, 2, 3, 112)])
def test_svi_parity_streamed_and_resume(nhp, N, T, B, L, Tb):
    """Six steps against the reference: the tables at rtol 1e-9, ρv and the network through `rho_bound` (one SVI step
    blends, so the bound of the un-blended step covers it).  Streamed equals resident to rtol 1e-12; a run cut at step 2
    and resumed with step0 is bit-equal to the whole run."""
    proc, data, conv, start = problem(nhp, N, T, B, L)
    nb = sr.n_blocks(T, Tb)
    blocks = six_blocks(nb)
    ds = nhp.convolve(proc, data)
    kw = dict(batch_bins=Tb, delay=1.0, forgetting=0.6)
    nr.put(proc, start)
    res = nhp.svi_(proc, ds, nsteps=6, blocks=blocks, **kw)
    got = copy_of(nr.get(proc))
    want5 = nr.netsvi_run(data, conv, 1.0, PRI, NET, start, blocks[:5], Tb, 1.0, 0.6)
    want = nr.netsvi_run(data, conv, 1.0, PRI, NET, want5, blocks[5:], Tb, 1.0, 0.6, step0=5)
    assert res.step == 6
    print(f"six SVI steps: largest relative difference of the tables {worst(got[TABLES], want[TABLES]):.2e}")
    for g, w in zip(got[TABLES], want[TABLES]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    err = nr.measured_logit_error()
    hat = nr.netsvi_step(data, conv, 1.0, PRI, NET, want5, int(blocks[5]), Tb, 1, 0.0, 1.0)      # the sixth step's hats (r = 1)
    b = rho_bound(hat, want5[8:], 1e-9, 0.0, 4 * err) + 1e-9 * want[7]
    print(f"six SVI steps: max |Δρv| {float(np.max(np.abs(got[7] - want[7]))):.2e} (bound up to {float(b.max()):.2e})")
    assert np.all(np.abs(got[7] - want[7]) <= b)
    assert abs(got[8] - want[8]) <= b.sum() + 1e-9 * want[8] and abs(got[9] - want[9]) <= b.sum() + 1e-9 * want[9]
    nr.put(proc, start)
    nhp.svi_(proc, data, nsteps=6, blocks=blocks, streamed=True, **kw)
    for g, w in zip(nr.get(proc), got):
        assert np.allclose(g, w, rtol=1e-12, atol=0.0)
    nr.put(proc, start)
    first = nhp.svi_(proc, ds, nsteps=2, seed=3, **kw)
    nhp.svi_(proc, ds, nsteps=4, seed=3, step0=first.step, trace_every=2, **kw)
    cut = copy_of(nr.get(proc))
    nr.put(proc, start)
    nhp.svi_(proc, ds, nsteps=6, seed=3, **kw)
    for g, w in zip(nr.get(proc), cut):
        assert np.array_equal(g, w)


def test_recovery_classifies_the_links_as_the_reference_does(nhp):
    r = nr.RECOVERY
    data, A, W = nr.simulate_sparse(r["N"], r["T"], r["B"], r["L"], r["seed"])
    conv = nr.convolve(data, sr.basis_brute(r["L"], r["B"], 1.0))
    want = nr.netvb_run(data, conv, 1.0, r["priors"], r["net"], nr.ones_start(r["N"], r["B"]), r["steps"])
    proc = nr.make_process(nhp, r["N"], r["B"], r["L"], r["priors"], r["net"], seed=1)
    nr.put(proc, nr.ones_start(r["N"], r["B"]))
    before = proc.adjacency_matrix.copy()
    res = nhp.vb_(proc, data, max_steps=r["steps"], keep_trace=False)
    rho = proc.weights.ρv
    print(np.round(rho, 3), A, sep="\n")
    assert res.step == r["steps"] and np.array_equal(proc.adjacency_matrix, before)         # VB leaves A alone
    assert np.array_equal(rho > 0.5, want[7] > 0.5) and np.array_equal(rho > 0.5, A > 0.5)   # the reference reaches 16 of 16
    nhp.variational_mean_(proc)
    assert np.array_equal(proc.adjacency_matrix, A) and np.isclose(proc.network.ρ, proc.network.αv / (proc.network.αv + proc.network.βv))
    assert np.allclose(proc.weights.W, proc.weights.κv1 / proc.weights.νv1) and np.allclose(proc.impulses.θ.sum(axis=2), 1.0)
    ll = nhp.loglikelihood(proc, data)
    assert np.isfinite(ll)
    resid = nhp.disc_residuals(proc, data)
    assert np.all(np.isfinite(resid.chi2))


def test_the_example_runs(capsys):
    ex = importlib.import_module("discrete_gaussian_network_hawkes_vb")
    ex.main(steps=4000, max_steps=20)
    out = capsys.readouterr().out
    assert "ρv | A" in out and "links classified as in the truth" in out
