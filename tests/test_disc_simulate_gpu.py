"""disc_rand(process, steps): the GPU generator nhp_disc_simulate (csrc/disc_simulate.hip).

Contract of the output, determinism, the exact numpy restatement of the documented counter scheme
(tests/disc_simulate_ref.py, written from include/nhp.h), more than one chunk of cells and of child slots, the edges, the
immigrant law, consistency with the library's own intensity (normalised martingale sums), agreement with the host
simulator and the config-4 shape end to end.

Statistical bounds are |z| <= 5 throughout: every statistic is a normalised sum over more than 10^3 expected events, the
two-sided normal tail at 5 is 5.7e-7, and the file holds fewer than 10^3 such statistics (about 220 on the small shapes, 512
node totals at the large one), so a correct sampler fails a given set of seeds with probability below 1e-3 -- and the
seeds are fixed and pre-checked on the restatement by tests/test_disc_simulate_host.py."""
import ctypes as C
import time

import numpy as np
import pytest

import disc_simulate_ref as dr

pytestmark = pytest.mark.gpu


def raw(nhp, process, T, seed, max_events=50_000_000, device=False, background=True):
    """nhp_disc_simulate through the C ABI -> (counts [N, T], background | None, n_events); device=True: torch tensors."""
    from nhp_amd import _lib
    ctx = nhp.default_context()
    base, W, th, A, phi, dt = dr.lower(process, T)
    N, (L, B) = W.shape[0], phi.shape
    homogeneous = not hasattr(process.baseline, "x")
    l0 = _lib.f64(process.baseline.λ) if homogeneous else None
    bs = None if homogeneous else np.asfortranarray(base).ravel(order="K")
    Wc, thc, Ac, ph = _lib.colmajor(W), _lib.colmajor(th), _lib.colmajor(A), np.asfortranarray(phi).ravel(order="K")
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        out = torch.full((T, N), -1, dtype=torch.int64, device=dev)
        bg = torch.full((T, N), -1, dtype=torch.int64, device=dev) if background else None
        torch.cuda.synchronize(dev)
        po, pb = out.data_ptr(), (bg.data_ptr() if background else None)
    else:
        out = np.full((T, N), -1, dtype=np.int64)
        bg = np.full((T, N), -1, dtype=np.int64) if background else None
        po, pb = out.ctypes.data, (bg.ctypes.data if background else None)
    n = C.c_int64(-1)
    _lib.check(_lib.lib().nhp_disc_simulate(ctx.h, _lib.dptr(l0), _lib.dptr(bs), _lib.dptr(Wc), _lib.dptr(thc), _lib.dptr(Ac),
                                            _lib.dptr(ph), L, B, dt, N, T, seed, max_events, int(device), po, pb, C.byref(n), None), ctx.h)
    tr = (lambda x: x.t()) if device else (lambda x: x.T)
    return tr(out), (tr(bg) if background else None), n.value


def invariants(s, bg, n, N, T):
    assert s.shape == bg.shape == (N, T) and s.dtype == bg.dtype == np.int64
    assert s.min() >= 0 and bg.min() >= 0 and np.all(s - bg >= 0)
    assert n == s.sum()


# ---- 1. contract --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,network", [(3, False), (5, True)])
def test_output_contract_and_determinism(nhp, N, network):
    import torch
    ctx = nhp.default_context()
    T = dr.T_SMALL
    p = dr.make(nhp, N, seed=N, network=network)
    s, bg, n = raw(nhp, p, T, 7)
    invariants(s, bg, n, N, T)
    assert n > 150 and (s - bg).sum() > 30
    # the Python entry: host arrays, device tensors, with and without the background -- the same sample
    assert np.array_equal(nhp.disc_rand(p, T, seed=7), s)
    hs, hb = nhp.disc_rand(p, T, seed=7, return_background=True)
    assert hs.dtype == hb.dtype == np.int64 and np.array_equal(hs, s) and np.array_equal(hb, bg)
    ds, db = nhp.disc_rand(p, T, seed=7, return_background=True, device=True)
    for x in (ds, db, nhp.disc_rand(p, T, seed=7, device=True)):
        assert x.dtype == torch.int64 and x.device.type == "cuda" and x.device.index == ctx.device and tuple(x.shape) == (N, T)
    assert np.array_equal(ds.cpu().numpy(), s) and np.array_equal(db.cpu().numpy(), bg)
    assert np.array_equal(nhp.disc_rand(p, T, seed=7, device=True).cpu().numpy(), s)
    # another seed: another sample; max_events at 2x and 20x the events: the same sample
    assert not np.array_equal(nhp.disc_rand(p, T, seed=8), s)
    for f in (2, 20):
        s2, bg2, n2 = raw(nhp, p, T, 7, max_events=f * n)
        assert n2 == n and np.array_equal(s2, s) and np.array_equal(bg2, bg)
    # the sample is what DiscreteDataset reads
    assert nhp.DiscreteDataset(ctx, hs).node_counts.sum() == n


# ---- 2. the exact restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(dr.RESTATE_CASES))
def test_restatement_reproduces_the_sample_exactly(nhp, name):
    kw, T, seed = dr.RESTATE_CASES[name]
    p = dr.make(nhp, **kw)
    s, bg = nhp.disc_rand(p, T, seed=seed, return_background=True)
    want, want_bg = dr.simulate(p, T, seed)
    assert want.sum() > want_bg.sum() > 0
    assert np.array_equal(bg, want_bg)
    assert np.array_equal(s, want)


# ---- 3. more than one chunk -------------------------------------------------------------------------------------------------------

def test_several_chunks_of_cells(nhp):
    """N = 8, T = 20000: generation 1 has more than 4096 slots, and with max_events at twice the events the 160000 cells go
    through several chunks; the restatement finishes in a second at this size, so the comparison is exact."""
    N, T = 8, 20000
    p = dr.make(nhp, N, seed=12, rate=0.06, scale=0.6)
    s, bg, n = raw(nhp, p, T, 21)
    invariants(s, bg, n, N, T)
    info = {}
    want, want_bg = dr.simulate(p, T, 21, info)
    assert info["per_generation"][0] > 4096 and N * T > 2 * 2 * n
    assert np.array_equal(s, want) and np.array_equal(bg, want_bg)
    for f in (2, 20):
        s2, bg2, n2 = raw(nhp, p, T, 21, max_events=f * n)
        assert n2 == n and np.array_equal(s2, s) and np.array_equal(bg2, bg)


def test_several_chunks_of_child_slots(nhp):
    """A generation's slots pass max_events (so its chunk) only when most children fall past the last bin: immigrants in bin
    T - 1 alone (an LGCP table), ten children per event, three lags of four past the end."""
    N, T = 8, 20000
    p = dr.make(nhp, N, seed=13, scale=10.0, lgcp_T=T)
    lam = np.zeros((4, N))
    lam[2] = 125.0
    p.baseline = nhp.DiscreteLogGaussianCoxProcess(np.array([0.0, T - 2.0, T - 1.0, float(T)]), lam, None, 0.0, 1.0)
    s, bg, n = raw(nhp, p, T, 22)
    invariants(s, bg, n, N, T)
    info = {}
    want, want_bg = dr.simulate(p, T, 22, info)
    assert np.array_equal(s, want) and np.array_equal(bg, want_bg)
    cap = 2 * n
    assert cap >= 4096 and info["per_generation"][0] > cap and info["per_generation"][1] > 2 * cap and info["kept"] > 1000
    s2, bg2, n2 = raw(nhp, p, T, 22, max_events=cap)
    assert n2 == n and np.array_equal(s2, s) and np.array_equal(bg2, bg)


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------

def test_edges(nhp):
    p = dr.make(nhp, 3, seed=2, rate=2.0)
    s, bg = nhp.disc_rand(p, 1, seed=1, return_background=True)             # T = 1: nothing can have a child
    assert s.shape == (3, 1) and np.array_equal(s, bg) and s.sum() > 0
    q = dr.make(nhp, 3, L=7, seed=2, rate=4.0, scale=2.0)                             # L > T
    s, bg = nhp.disc_rand(q, 3, seed=1, return_background=True)
    want, want_bg = dr.simulate(q, 3, 1)
    assert np.array_equal(s, want) and np.array_equal(bg, want_bg) and (s - bg).sum() > 0
    still = dr.make(nhp, 3, seed=2, scale=0.0)                              # W = 0
    s, bg = nhp.disc_rand(still, dr.T_SMALL, seed=1, return_background=True)
    assert np.array_equal(s, bg) and s.sum() > 100
    quiet = dr.make(nhp, 3, seed=2, rate=0.0)                               # λ0 = 0
    s, bg, n = raw(nhp, quiet, dr.T_SMALL, 1)
    assert n == 0 and not s.any() and not bg.any()
    s, bg, n = raw(nhp, quiet, dr.T_SMALL, 1, max_events=0)
    assert n == 0 and not s.any()


def test_explosion_is_an_error_and_the_context_survives(nhp):
    wild = dr.make(nhp, 3, seed=2, scale=3.0)
    with pytest.raises(RuntimeError, match="exploded"):
        nhp.disc_rand(wild, dr.T_SMALL, seed=1, max_events=20000)
    with pytest.raises(RuntimeError, match="exploded"):                      # the immigrants alone pass the cap
        nhp.disc_rand(wild, dr.T_SMALL, seed=1, max_events=10)
    p = dr.make(nhp, 3, seed=2)
    assert np.array_equal(nhp.disc_rand(p, dr.T_SMALL, seed=1), dr.simulate(p, dr.T_SMALL, 1)[0])


def test_parameters_no_process_has(nhp):
    p = dr.make(nhp, 3, seed=2)
    p.weights.W = p.weights.W.copy()
    p.weights.W[1, 2] = -0.1
    with pytest.raises(nhp.DomainError):
        nhp.disc_rand(p, 50)
    p = dr.make(nhp, 3, seed=2)
    p.impulses.θ[0, 1, 0] = np.nan
    with pytest.raises(nhp.DomainError):
        nhp.disc_rand(p, 50)
    p = dr.make(nhp, 3, seed=2)
    p.baseline.λ[2] = np.inf
    with pytest.raises(nhp.DomainError):
        nhp.disc_rand(p, 50)
    assert nhp.disc_rand(dr.make(nhp, 3, seed=2), 50).shape == (3, 50)


# ---- 5. immigrants ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mean", dr.IMMIGRANT_MEANS)
def test_immigrants_are_poisson(nhp, mean):
    s, bg = nhp.disc_rand(dr.immigrant_process(nhp, mean), dr.IMMIGRANT_T, seed=dr.IMMIGRANT_SEED, return_background=True)
    assert np.array_equal(s, bg)
    z, chi2 = dr.immigrant_checks(s, mean)
    print(f"mean {mean}: z of the node totals {z}")
    assert np.all(np.abs(z) <= 5.0) and chi2


# ---- 6. consistency with the library's own intensity ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(dr.MARTINGALE_CASES))
def test_martingale_sums_against_disc_intensity(nhp, name):
    import copy
    p = dr.make(nhp, **dr.MARTINGALE_CASES[name])
    s = nhp.disc_rand(p, dr.MARTINGALE_T, seed=dr.MARTINGALE_SEED)
    assert s.sum(axis=1).min() > 1000
    lam = nhp.intensity(p, s)
    late = copy.deepcopy(p)
    shifted = dr.shifted_basis(p)
    late.impulses.basis = lambda: shifted
    dr.assert_martingale(p, s, lam, nhp.intensity(late, s))


# ---- 7. agreement with the host simulator -------------------------------------------------------------------------------------------

def test_agreement_with_the_host_simulator(nhp):
    kw, T, S = dr.AGREEMENT
    p = dr.make(nhp, **kw)
    dr.assert_agreement([nhp.disc_rand(p, T, seed=seed) for seed in range(S)], [nhp.rand(p, T, seed=1000 + seed) for seed in range(S)])


# ---- 8. the config-4 shape ------------------------------------------------------------------------------------------------------

def test_config4_shape_end_to_end(nhp):
    """N = 512, B = 8, L = 32, T = 1e5 on the device.  Per-node totals over the bins after a start-up of 20·L bins against
    the stationary expectation m = (I - Gᵀ)⁻¹·λ0·dt per bin, with the asymptotic variance of a Hawkes count,
    T'·[(I - Gᵀ)⁻¹ diag(m) (I - G)⁻¹]_cc (Hawkes 1971); what the window's two edges add or lose is of the order of L·m·ΣG
    events per node, below a hundredth of a standard deviation here."""
    import torch
    N, B, L, T = 512, 8, 32, 100_000
    rng = np.random.default_rng(7)
    lam0 = rng.uniform(0.02, 0.08, N)
    W = rng.uniform(0, 1, (N, N)) / N
    p = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(lam0, 1.0),
                                          nhp.DiscreteGaussianImpulseResponse(np.full((N, N, B), 1.0 / B), L, 1.0),
                                          nhp.DenseWeightModel(W), 1.0)
    t0 = time.perf_counter()
    s, bg, n = raw(nhp, p, T, 3, max_events=20_000_000, device=True)
    torch.cuda.synchronize()
    print(f"config 4: {n} events in {1e3 * (time.perf_counter() - t0):.1f} ms (uploads and allocation included)")
    assert tuple(s.shape) == tuple(bg.shape) == (N, T) and s.dtype == bg.dtype == torch.int64
    assert int(s.min()) >= 0 and int(bg.min()) >= 0 and int((s - bg).min()) >= 0
    assert int(s.sum()) == n
    G = dr.link_mass(p)
    M = np.linalg.inv(np.eye(N) - G.T)
    m = M @ lam0
    burn = 20 * L
    tot = s[:, burn:].sum(dim=1).cpu().numpy()
    sd = np.sqrt((T - burn) * ((M ** 2) @ m))
    z = (tot - (T - burn) * m) / sd
    print(f"node totals: max |z| = {np.abs(z).max():.2f}, rms z = {np.sqrt(np.mean(z ** 2)):.2f}")
    assert np.all(np.abs(z) <= 5.0)
    assert abs(np.sqrt(np.mean(z ** 2)) - 1.0) < 0.16       # the spread is the stated one: the rms of 512 values has σ = 1/√1024, 5 of them
    zb = (int(bg.sum()) - T * lam0.sum()) / np.sqrt(T * lam0.sum())
    print(f"immigrants in all: z = {zb:.2f}")
    assert abs(zb) <= 5.0
