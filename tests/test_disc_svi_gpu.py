"""svi_ on the GPU (nhp_disc_svi_run) against the numpy reference tests/disc_svi_ref.py: parity per step and
over a chain at the shapes where the block GEMMs take another path, a block without events, the one-block limit against
update_, chunking and seeds, the streamed mode against the resident one, the property that gives SVI its name, and the
example."""
import importlib
import os
import sys

import numpy as np
import pytest

import disc_svi_ref as sr

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

PRIORS = (1.0, 1.0, 1.0, 1.0, 1.0)


def make(nhp, N, T, B, L, seed=0, dt=1.0, rate=0.3):
    """The models and counts of tests/test_discrete_gpu.py (a copy of its `make`, standard process only)."""
    rng = np.random.default_rng(seed)
    data = rng.poisson(rate, (N, T)).astype(np.int64)
    W = rng.uniform(0.05, 0.3, (N, N)) / max(1, N // 4)
    th = rng.dirichlet(np.ones(B), (N, N))
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    th = np.where(th.sum(axis=2, keepdims=True) == 1.0, th, th)
    lam0 = rng.uniform(0.2, 1.0, N)
    rng.uniform(size=(N, N))                                        # (the adjacency draw of the original: same stream)
    base = nhp.DiscreteHomogeneousProcess(lam0, dt)
    imp = nhp.DiscreteGaussianImpulseResponse.__new__(nhp.DiscreteGaussianImpulseResponse)
    imp.θ, imp.γ, imp.γv, imp.nlags, imp.dt, imp.ϕ = th, 1.0, np.ones_like(th), L, dt, None
    return nhp.DiscreteStandardHawkesProcess(base, imp, nhp.DenseWeightModel(W), dt), data


def random_start(N, B, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 3, N), rng.uniform(0.5, 3, N), rng.uniform(0.5, 3, (N, N)), rng.uniform(0.5, 3, (N, N)),
            rng.uniform(0.5, 3, (N, N, B)))


def put(proc, params):
    av, bv, kv, nv, gv = (np.array(p, dtype=np.float64) for p in params)
    proc.baseline.αv, proc.baseline.βv, proc.weights.κv, proc.weights.νv, proc.impulses.γv = av, bv, kv, nv, gv
    return proc


def get(proc):
    return proc.baseline.αv, proc.baseline.βv, proc.weights.κv, proc.weights.νv, proc.impulses.γv


def worst(got, want):
    return max(float(np.max(np.abs(g - w) / np.abs(w))) for g, w in zip(got, want))


_REF = {}


def reference(orc, key, data, conv, start, blocks, Tb):
    """The reference after one and after six steps, computed once per shape (the two tile heights share it)."""
    if key not in _REF:
        one = sr.svi_run(orc, data, conv, 1.0, PRIORS, start, blocks[:1], Tb, 1.0, 0.6)
        _REF[key] = (one, sr.svi_run(orc, data, conv, 1.0, PRIORS, one, blocks[1:], Tb, 1.0, 0.6, step0=1))
    return _REF[key]


def six_blocks(nb):
    return np.array([0, nb - 1, min(1, nb - 1), nb - 1, 0, 0], dtype=np.int32)      # block 0, the last block, repeats


SHAPES = [(3, 50, 2, 4, 16, None),            # last block of 2 bins, shorter than L
          (5, 700, 3, 7, 128, None),          # last block of 60 bins
          (130, 300, 2, 3, 112, None),        # N crosses the 128-column tile; Tb a multiple of 16 but not of the tile height
          (128, 2560, 2, 4, 1280, "128"),     # whole tiles at 128 rows: the branch-free main loop
          (128, 2560, 2, 4, 1280, "160")]     # ... and at 160 rows


@pytest.mark.parametrize("N,T,B,L,Tb,bm", SHAPES)
def test_parity_with_the_reference(nhp, orc, monkeypatch, N, T, B, L, Tb, bm):
    """One step to rtol 1e-10 / atol 1e-12 (the bound test_vb_step holds a VB step to), six chained steps to rtol 1e-9.
    Measured maxima of the relative difference over the five cases: one step 2.2e-15, six steps 3.8e-15 (both at N = 128)."""
    if bm:
        monkeypatch.setenv("NHP_GEMM_BM", bm)
    proc, data = make(nhp, N, T, B, L, seed=7 * N)
    conv = orc.disc_convolve(data, orc.disc_basis(L, B, 1.0))
    start = random_start(N, B)
    nb = sr.n_blocks(T, Tb)
    blocks = six_blocks(nb)
    ds = nhp.convolve(proc, data)
    put(proc, start)
    res = nhp.svi_(proc, ds, nsteps=1, batch_bins=Tb, delay=1.0, forgetting=0.6, blocks=blocks[:1])
    want1, want6 = reference(orc, (N, T, B, L, Tb), data, conv, start, blocks, Tb)
    print(f"one step: largest relative difference {worst(get(proc), want1):.2e}")
    for g, w in zip(get(proc), want1):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)
    assert res.step == 1 and len(res.trace) == 1 and len(res.trace[0]) == 2 * N + N * N * B + 2 * N * N
    put(proc, start)
    res = nhp.svi_(proc, ds, nsteps=6, batch_bins=Tb, delay=1.0, forgetting=0.6, blocks=blocks)
    print(f"six steps: largest relative difference {worst(get(proc), want6):.2e}")
    for g, w in zip(get(proc), want6):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    assert res.step == 6


def test_a_block_without_events(nhp, orc):
    N, T, B, L, Tb = 5, 700, 3, 7, 128
    proc, data = make(nhp, N, T, B, L, seed=35)
    data[:, 128:256] = 0
    conv = orc.disc_convolve(data, orc.disc_basis(L, B, 1.0))
    assert conv[128:128 + L].max() > 0.0                           # the lags still reach back into block 0
    start = random_start(N, B)
    put(proc, start)
    nhp.svi_(proc, data, nsteps=1, batch_bins=Tb, delay=1.0, forgetting=0.6, blocks=[1])
    got = get(proc)
    assert all(np.all(np.isfinite(g)) and np.all(g > 0.0) for g in got)
    r = sr.rho(1, 1.0, 0.6)
    for g, s in ((got[0], start[0]), (got[2], start[2]), (got[4], start[4])):      # α̂, κ̂, γ̂ are the priors
        assert np.allclose(g, (1.0 - r) * s + r * 1.0, rtol=1e-14, atol=0.0)
    want = sr.svi_run(orc, data, conv, 1.0, PRIORS, start, [1], Tb, 1.0, 0.6)
    for g, w in zip(got, want):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("N,T,B,L", [(5, 700, 3, 7), (130, 300, 2, 3)])
def test_one_block_and_no_delay_is_update(nhp, N, T, B, L):
    proc, data = make(nhp, N, T, B, L, seed=7 * N)
    ds = nhp.convolve(proc, data)
    start = random_start(N, B)
    put(proc, start)
    nhp.update_(proc, data, ds)
    want = [g.copy() for g in get(proc)]
    for Tb in (T, 4096):
        put(proc, start)
        nhp.svi_(proc, ds, nsteps=1, batch_bins=Tb, delay=0.0, forgetting=0.6)
        for g, w in zip(get(proc), want):
            assert np.allclose(g, w, rtol=1e-12, atol=0.0)


def test_chunking_and_seeds(nhp):
    N, T, B, L, Tb = 5, 700, 3, 7, 128
    proc, data = make(nhp, N, T, B, L, seed=35)
    ds = nhp.convolve(proc, data)
    start = random_start(N, B)

    def run(**kw):
        put(proc, start)
        res = nhp.svi_(proc, ds, batch_bins=Tb, delay=1.0, forgetting=0.6, **kw)
        return res, [g.copy() for g in get(proc)]

    res, plain = run(nsteps=6, seed=3)
    assert res.step == 6 and len(res.trace) == 1
    put(proc, start)
    first = nhp.svi_(proc, ds, nsteps=3, batch_bins=Tb, delay=1.0, forgetting=0.6, seed=3)
    second = nhp.svi_(proc, ds, nsteps=3, batch_bins=Tb, delay=1.0, forgetting=0.6, seed=3, step0=first.step)
    assert first.step == 3 and second.step == 6
    assert all(np.array_equal(g, w) for g, w in zip(get(proc), plain))            # 3 + 3 with step0 = 3
    _, again = run(nsteps=6, seed=3)
    assert all(np.array_equal(g, w) for g, w in zip(again, plain))
    _, other = run(nsteps=6, seed=4)
    assert not np.array_equal(other[4], plain[4])
    blocks = nhp.svi_blocks(3, 0, 6, sr.n_blocks(T, Tb))
    _, given = run(nsteps=6, seed=99, blocks=blocks)                              # the library's own sequence, passed back
    assert all(np.array_equal(g, w) for g, w in zip(given, plain))
    res, traced = run(nsteps=6, seed=3, trace_every=2)
    assert res.step == 6 and len(res.trace) == 3
    assert all(np.array_equal(g, w) for g, w in zip(traced, plain)) and np.array_equal(res.trace[-1], proc.variational_params())
    assert not np.array_equal(res.trace[0], res.trace[1])


@pytest.mark.parametrize("N,T,B,L,Tb,rate", [(5, 700, 3, 7, 128, 0.3), (5, 700, 3, 7, 128, 0.05), (130, 300, 2, 3, 112, 0.3)])
def test_streamed_equals_resident(nhp, N, T, B, L, Tb, rate):
    """A block convolved on the fly is the resident Ŝ's rows (rate 0.3: the resident convolution took its dense kernel, 0.05:
    the sparse one), so the steps agree -- to rtol 1e-12 here; the bits came out equal at every case (printed)."""
    proc, data = make(nhp, N, T, B, L, seed=7 * N, rate=rate)
    start = random_start(N, B)
    blocks = six_blocks(sr.n_blocks(T, Tb))
    put(proc, start)
    nhp.svi_(proc, data, nsteps=6, batch_bins=Tb, blocks=blocks)
    want = [g.copy() for g in get(proc)]
    fresh = nhp.DiscreteDataset(nhp.default_context(), data)                      # never convolved
    put(proc, start)
    nhp.svi_(proc, fresh, nsteps=6, batch_bins=Tb, blocks=blocks, streamed=True)
    got = get(proc)
    print(f"streamed against resident: bits equal {all(np.array_equal(g, w) for g, w in zip(got, want))}, "
          f"largest relative difference {worst(got, want):.2e}")
    for g, w in zip(got, want):
        assert np.allclose(g, w, rtol=1e-12, atol=0.0)
    assert fresh.B == 0
    with pytest.raises(nhp.NhpError, match="convolve"):                           # still no resident Ŝ behind the handle
        nhp.update_(proc, data, fresh)


# the bound of the log-likelihood comparison below: 100 times the deviation measured once (1.12e-16 relative: one unit in
# the last place of -32 604.5), which is far inside the project's fp64 contract of 1e-6.  It is a tight bound for 395 chained
# steps against a CPU oracle: a compiler or runtime update that reorders a sum in the GEMMs or in libm can move the device's
# value by more than 1.1e-14 with no bug behind it.  When this assertion fails while test_parity_with_the_reference still
# passes, run this test with -s, read the printed relative deviation, and if it is far below 1e-6 put it here in place of
# 1.12e-16 (the rule -- 100 times the deviation measured once, never more than 1e-6 -- stays).
LL_RTOL = min(100 * 1.12e-16, 1e-6)


def test_svi_earns_its_name_on_the_device(nhp, orc):
    e = sr.EARNS
    N, T, B, L, Tb = e["N"], e["T"], e["B"], e["L"], e["Tb"]
    data = sr.simulate(N, T, B, L)
    conv = orc.disc_convolve(data, orc.disc_basis(L, B, 1.0))
    start = sr.ones_start(N, B)
    th = np.full((N, N, B), 1.0 / B)
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)

    def fresh():
        return put(nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.ones(N), 1.0),
                                                     nhp.DiscreteGaussianImpulseResponse(th, L, 1.0),
                                                     nhp.DenseWeightModel(np.full((N, N), 0.1)), 1.0), start)

    ds = nhp.convolve(fresh(), data)
    blocks = sr.earns_blocks(0)
    assert len(blocks) == 395
    proc = fresh()
    nhp.svi_(proc, ds, nsteps=len(blocks), batch_bins=Tb, delay=e["delay"], forgetting=e["forgetting"], blocks=blocks)
    got = sr.loglik_at_means(orc, data, conv, get(proc), 1.0)
    want = sr.loglik_at_means(orc, data, conv, sr.svi_run(orc, data, conv, 1.0, PRIORS, start, blocks, Tb, e["delay"],
                                                          e["forgetting"]), 1.0)
    print(f"log-likelihood at the means after 395 steps: device {got:.6f}, reference {want:.6f}, "
          f"relative deviation {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= LL_RTOL * abs(want)
    vbp = fresh()
    nhp.vb_(vbp, ds, max_steps=e["passes"], keep_trace=False)
    vb = sr.loglik_at_means(orc, data, conv, get(vbp), 1.0)
    for seed in (0, 1, 2):
        proc = fresh()
        res = nhp.svi_(proc, ds, nsteps=395, batch_bins=Tb, delay=e["delay"], forgetting=e["forgetting"], seed=seed)
        svi = sr.loglik_at_means(orc, data, conv, get(proc), 1.0)
        print(f"seed {seed}: SVI {svi:.3f}  VB after {e['passes']} passes {vb:.3f}  margin {svi - vb:.3f}")
        assert res.step == 395 and svi > vb


def test_the_example():
    svi, vb, ll_svi, ll_vb = importlib.import_module("discrete_gaussian_standard_hawkes_svi").main(duration=3000, batch_bins=256)
    assert np.all(np.isfinite(svi.variational_params())) and np.all(svi.variational_params() > 0.0)
    assert np.all(np.isfinite(vb.variational_params())) and np.isfinite(ll_svi) and np.isfinite(ll_vb)
