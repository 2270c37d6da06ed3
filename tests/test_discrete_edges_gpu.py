"""The discrete inference kernels (csrc/disc.hip, csrc/disc_gibbs.hip) against an exact reference at their edges.

C1  intensity, log-likelihood and gradient against tests/disc_grad_ref.py (long double) where the GEMMs, the slab split of
    GEMM-2 (disc_grad_sizes) and k_disc_grad_finish change path:
      one_element       N=1   T=1    B=1 L=2   one element, T < L
      k_below_bk        N=3   T=17   B=2 L=5   K = 6 < BK; T one over a BK slab
      fd_shape          N=3   T=400  B=2 L=5   the finite-difference shape of test_discrete_gpu.py, now exact
      ragged            N=17  T=129  B=5 L=9   K = 85, ragged everything
      two_column_tiles  N=130 T=997  B=2 L=3   two column tiles, three GEMM-2 row tiles, ragged last slab
      whole_tiles       N=128 T=1280 B=2 L=4   whole tiles: the WHOLE loop, with NHP_GEMM_BM 128 / 160 and NHP_GEMM_PLAIN
      one_column_over   N=129 T=65   B=2 L=3   second column tile of one column, T one over a tile row
      lgcp              N=64  T=2000 B=4 L=8   LGCP baseline, G = 9 grid points
    λ to 1e-12 and ll to 1e-11 relative (the suite's figures for these kernels); every gradient entry within
    (N·B + T + 16)·2⁻⁵³·S of the reference, S the sum of the absolute values of the entry's terms
    (disc_grad_ref.gradient_bound has the derivation; tests/test_disc_grad_host.py shows a float64 numpy evaluation of the
    same inputs inside it).
C2  the log-queue of the EPI_LOGLIK / EPI_GRAD epilogue at its occupancy edges (N=5, T=300, B=3, L=7): no bin occupied
    (never flushes), one bin (flushes at the end only), about half, every bin (flushes on every push).
C3  count ranges (N=2, T=192, B=2, L=4, Poisson(0.5) with planted bins): maximum exactly 255 (the byte plane), a 256 (no
    byte plane), and 70 000 / 65 535 / 65 536 / 1 200 000 (past the 16-bit packing of the lane exchange, draw index
    (bin << 20) | j with j >= 2^20): convolution, ll / gradient, VB step and Gibbs parent counts.  Poisson(0.5) is dense
    enough that nhp_disc_convolve takes its dense kernel whatever the switch says, so the same planted bins on a
    Poisson(0.05) matrix walk the sparse kernel with and without the byte plane as well.
C4  Gibbs parent counts where k_disc_resample_parents leaves its usual path: a tile with more than XSIDE bins that keep
    several events for walk 2 (the lane exchange gives up), a count past 65 535 in the two-slot kernel (it gives up as
    well), a tile with more occupied bins than threads under the one-slot kernel (second round), and N=129, T=65.
C5  the device optimizer on a shape with several tiles.
D   nhp_disc_dataset_create's own refusal of a single negative count (DiscreteDataset refuses before calling it).

Which route a case takes is read from the launchers' arithmetic (asserted on the data here where it is a property of the
data), not observed on the device.

Largest |g - g_ref| / bound observed on an MI355X, per case:
    one_element 0        k_below_bk 0.026     fd_shape 0.0025   ragged 0.0075     two_column_tiles 0.0023
    whole_tiles 0.0019 (default, NHP_GEMM_BM 128 / 160, NHP_GEMM_PLAIN: all alike)      one_column_over 0.0079
    lgcp 0.0014          all_zero 0           one_bin 0.0015    half 0.0043       every_bin 0.0054
    max_255 0.0062       with_256 0.0058      huge 0.0076
(a float64 numpy evaluation of the same inputs: 0.001 to 0.03); λ within 1.3e-15, ll within 4.5e-16 relative, the two ll entry
points equal; the device optimizer's value equals the reference's to every printed digit.
"""
import copy

import numpy as np
import pytest

import disc_edge_cases as cases
import disc_grad_ref as ref

pytestmark = pytest.mark.gpu


def process(nhp, c):
    """The package's process object for a case's arrays."""
    dt, L = c["dt"], c["phi"].shape[0]
    if "lam0" in c:
        base = nhp.DiscreteHomogeneousProcess(c["lam0"].copy(), dt)
    else:
        base = nhp.DiscreteLogGaussianCoxProcess(c["grid_x"].copy(), c["lam_grid"].copy(), None, -1.0, dt)
    proc = nhp.DiscreteStandardHawkesProcess(base, nhp.DiscreteGaussianImpulseResponse(c["theta"].copy(), L, dt),
                                             nhp.DenseWeightModel(c["W"].copy()), dt)
    assert np.array_equal(proc.impulses.basis(), c["phi"])
    return proc


def held_to_the_reference(nhp, name, c, r, proc=None):
    """λ, ll (both entry points) and the gradient of case `c` against the reference `r`; prints the gradient's error / bound."""
    proc = proc or process(nhp, c)
    data = c["data"]
    N, T = data.shape
    B = c["phi"].shape[1]
    ds = nhp.convolve(proc, data)
    lam = nhp.intensity(proc, ds)
    assert lam.shape == (T, N)
    lam_err = float(np.max(np.abs(lam - r.lam) / r.lam))
    ll = nhp.loglikelihood(proc, data, convolved=ds)
    ll2, g = nhp.loglikelihood_gradient(proc, data, convolved=ds)
    ref_ll = float(r.ll)
    bound = ref.gradient_bound(N, T, B, r.scale)
    err = np.abs(g - r.grad)
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    print(f"[{name}] lambda rel {lam_err:.3g}  ll rel {abs(ll - ref_ll) / abs(ref_ll):.3g} / {abs(ll2 - ref_ll) / abs(ref_ll):.3g}"
          f"  gradient error / bound {ratio:.3g}  (bound / scale {(N * B + T + 16) * 2.0 ** -53:.3g})")
    assert lam_err < 1e-12
    assert abs(ll - ref_ll) < 1e-11 * abs(ref_ll) and abs(ll2 - ref_ll) < 1e-11 * abs(ref_ll)
    assert abs(ll - ll2) <= 1e-12 * abs(ref_ll)
    assert g.shape == r.grad.shape
    worst = int(np.argmax(np.where(pos, err / np.where(pos, bound, 1), np.where(err > 0, np.inf, 0.0))))
    assert np.all(err <= bound), (worst, float(g[worst]), float(r.grad[worst]), float(err[worst]), float(bound[worst]))
    return ds


C1_RUNS = [(name, None, False) for name in cases.C1] + [("whole_tiles", bm, plain) for bm in ("128", "160") for plain in (False, True)]


@pytest.mark.parametrize("name,bm,plain", C1_RUNS)
def test_intensity_loglik_and_gradient_equal_the_reference(nhp, orc, monkeypatch, name, bm, plain):
    if bm:
        monkeypatch.setenv("NHP_GEMM_BM", bm)
    if plain:
        monkeypatch.setenv("NHP_GEMM_PLAIN", "1")
    c, r = cases.case(orc, name), cases.reference(orc, name)
    held_to_the_reference(nhp, name + (f"/bm{bm}" + ("/plain" if plain else "") if bm else ""), c, r)


@pytest.mark.parametrize("name", cases.C2)
def test_log_queue_occupancy_edges(nhp, orc, name):
    c, r = cases.case(orc, name), cases.reference(orc, name)
    occupied = int(np.count_nonzero(c["data"]))
    assert {"all_zero": occupied == 0, "one_bin": occupied == 1, "half": 0.4 < occupied / c["data"].size < 0.6,
            "every_bin": occupied == c["data"].size}[name]
    held_to_the_reference(nhp, name, c, r)
    if name == "all_zero":
        proc = process(nhp, c)
        ll = nhp.loglikelihood(proc, c["data"])
        assert abs(ll + float(r.lam.sum())) < 1e-11 * float(r.lam.sum())          # ll = -Σλ


def planted(data, rate, seed):
    """The planted bins of a C3 matrix on a Poisson(rate) background."""
    thin = np.random.default_rng(seed).poisson(rate, data.shape).astype(np.int64)
    big = data >= 255
    thin[big] = data[big]
    return thin


@pytest.mark.parametrize("name", cases.C3)
def test_count_ranges_through_the_pipeline(nhp, orc, monkeypatch, name):
    c, r = cases.case(orc, name), cases.reference(orc, name)
    data = c["data"]
    N, T = data.shape
    B = c["phi"].shape[1]
    assert int(data.max()) == {"max_255": 255, "with_256": 256, "huge": 1_200_000}[name]
    if name == "huge":
        assert sorted(data[0][data[0] > 255].tolist()) == [65_535, 65_536, 70_000] and data[1].max() >= 1 << 20
    proc = process(nhp, c)
    # convolution, bit for bit, both kernels; the thin matrix takes the sparse walk (fewer than 1 bin in 8 occupied)
    thin = planted(data, 0.05, 7)
    assert np.count_nonzero(thin) < 0.125 * thin.size <= np.count_nonzero(data)
    for d in (data, thin):
        want = orc.disc_convolve(d, c["phi"])
        monkeypatch.delenv("NHP_CONV_DENSE", raising=False)
        _, conv = nhp.convolve(proc, d, fetch=True)
        assert np.array_equal(conv, want)
        monkeypatch.setenv("NHP_CONV_DENSE", "1")
        _, conv = nhp.convolve(proc, d, fetch=True)
        assert np.array_equal(conv, want)
    monkeypatch.delenv("NHP_CONV_DENSE", raising=False)
    # log-likelihood and gradient
    ds = held_to_the_reference(nhp, name, c, r, proc)
    conv = orc.disc_convolve(data, c["phi"])
    # Gibbs parent counts: integer work, equal to the oracle's; every event gets exactly one parent
    got = nhp.resample_parent_counts(proc, convolved=ds, seed=5, step=2)
    want = orc.disc_resample_parents(data, conv, c["lam0"], c["W"], c["theta"], c["dt"], seed=5, step=2)
    assert np.array_equal(got.sum(axis=1), data.sum(axis=1))
    assert np.array_equal(want.sum(axis=1), data.sum(axis=1))
    assert np.array_equal(got, want)
    # one VB step
    rng = np.random.default_rng(5)
    b, w, imp = proc.baseline, proc.weights, proc.impulses
    b.αv, b.βv = rng.uniform(0.5, 3, N), rng.uniform(0.5, 3, N)
    w.κv, w.νv = rng.uniform(0.5, 3, (N, N)), rng.uniform(0.5, 3, (N, N))
    imp.γv = rng.uniform(0.5, 3, (N, N, B))
    want = orc.disc_vb_step(data, conv, c["dt"], b.α0, b.β0, w.κ, w.ν, imp.γ, b.αv, b.βv, w.κv, w.νv, imp.γv)
    nhp.update_(proc, data, ds)
    for g, v in zip((b.αv, b.βv, w.κv, w.νv, imp.γv), want):
        assert np.allclose(g, v, rtol=1e-10, atol=1e-12)


def gibbs_case(nhp, N, T, B, L, data, lam0, seed):
    rng = np.random.default_rng(seed)
    proc = nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(np.asarray(lam0, dtype=np.float64), 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(cases._theta(rng, N, B), L, 1.0),
                                             nhp.DenseWeightModel(rng.uniform(0.0, 0.5, (N, N)) / N), 1.0)
    return proc, data.astype(np.int64)


def slots_of_the_launch(data, tile_bins=64, tile_nodes=128, threads=256):
    """disc_parent_counts' choice (small tile): one occupied bin per thread unless the mean tile, plus three standard
    deviations, holds more than the workgroup has threads."""
    N, T = data.shape
    mean = np.count_nonzero(data) * (tile_bins * tile_nodes) / (T * max(N, tile_nodes))
    return 1 if mean + 3.0 * np.sqrt(mean) <= threads else 2


def gibbs_data(kind):
    rng = np.random.default_rng(9)
    if kind == "dense_tile":                       # > XSIDE = 256 bins of a tile keep several events for walk 2
        N, T, B, L = 8, 128, 2, 4
        data = rng.poisson(6.0, (N, T))
        lam0 = np.full(N, 1e-3)                    # next to nothing is placed in the baseline category
        assert slots_of_the_launch(data) == 2 and min(np.count_nonzero(data[:, a:a + 64] >= 2) for a in (0, 64)) > 256 + N
    elif kind == "past_16_bits":                   # two slots, few bins with several events, one of them with n > 65 535
        N, T, B, L = 8, 128, 2, 4
        data = rng.poisson(0.7, (N, T))
        data[3, 90] = 70_000
        lam0 = np.full(N, 0.2)                     # (a baseline this small leaves nearly all of them for walk 2)
        assert slots_of_the_launch(data) == 2 and max(np.count_nonzero(data[:, a:a + 64] >= 2) for a in (0, 64)) < 256
    elif kind == "uneven":                         # one slot by the global mean, yet the first tile holds ~490 bins for 256 threads
        N, T, B, L = 8, 6400, 2, 4
        data = np.zeros((N, T), dtype=np.int64)
        data[:, :64] = rng.poisson(3.0, (N, 64))
        lam0 = np.full(N, 0.2)
        assert slots_of_the_launch(data) == 1 and np.count_nonzero(data[:, :64]) > 256
    else:                                          # a second node tile of one column, a second bin tile of one bin
        N, T, B, L = 129, 65, 2, 3
        data = rng.poisson(0.3, (N, T))
        lam0 = rng.uniform(0.05, 0.3, N)
        assert data[128].any() and data[:, 64].any()
    return N, T, B, L, data, lam0


@pytest.mark.parametrize("kind", ["dense_tile", "past_16_bits", "uneven", "second_tiles"])
def test_parent_counts_on_the_untested_routes(nhp, orc, kind):
    N, T, B, L, data, lam0 = gibbs_data(kind)
    proc, data = gibbs_case(nhp, N, T, B, L, data, lam0, seed=N + T)
    ds, conv = nhp.convolve(proc, data, fetch=True)
    got = nhp.resample_parent_counts(proc, convolved=ds, seed=11, step=4)
    want = orc.disc_resample_parents(data, conv, proc.baseline.λ, proc.weights.W, proc.impulses.θ, proc.dt, seed=11, step=4)
    assert got.shape == (N, 1 + N * B)
    assert np.array_equal(got.sum(axis=1), data.sum(axis=1))
    assert np.array_equal(got, want)
    again = nhp.resample_parent_counts(proc, convolved=ds, seed=11, step=4)
    assert np.array_equal(got, again)                                   # the same call, the same seed: the same counts
    if kind == "dense_tile":
        assert got[:, 0].sum() < 0.02 * data.sum()                      # the baseline took next to nothing


def test_device_mle_on_several_tiles(nhp, orc):
    """nhp_disc_mle_run at N=130, T=997, B=2: two column tiles, three GEMM-2 row tiles, a ragged last slab in every
    objective call.  Five steps from the case's own parameters: the value it reports is the reference's log-likelihood of
    the parameters the process then holds, and more than the reference's of the start."""
    c = cases.case(orc, "two_column_tiles")
    data = c["data"]
    N, T = data.shape
    B = c["phi"].shape[1]
    proc = process(nhp, c)
    x0 = np.clip(proc.params(), 1e-6, 10.0)
    eta0 = x0[N:].reshape((N, N, B), order="F")
    start = ref.evaluate(data, c["phi"], eta0.sum(axis=2), eta0 / eta0.sum(axis=2)[:, :, None], c["dt"], lam0=x0[:N])
    res = nhp.mle_(proc, data, guess=x0, optimizer="device", max_steps=5)
    assert res.steps <= 5
    assert np.array_equal(proc.params(), nhp.discrete.disc_params_(copy.deepcopy(proc), res.maximizer))
    now = ref.evaluate(data, c["phi"], proc.weights.W, proc.impulses.θ, c["dt"], lam0=proc.baseline.λ)
    print(f"[device mle] start {float(start.ll):.6f}  reported {res.maximum:.6f}  reference {float(now.ll):.6f}  "
          f"rel {abs(res.maximum - float(now.ll)) / abs(float(now.ll)):.3g}")
    assert abs(res.maximum - float(now.ll)) < 1e-9 * abs(float(now.ll))
    assert res.maximum > float(start.ll) and float(now.ll) > float(start.ll)


def test_the_library_refuses_a_single_negative_count(nhp):
    """nhp_disc_dataset_create itself (DiscreteDataset refuses before calling it): a row [-1, 0, 5, ...] with a positive
    total is NHP_EDOMAIN, no handle comes back, and the context goes on working."""
    import ctypes as C
    from nhp_amd import _lib
    ctx = _lib.default_context()
    data = np.zeros((3, 40), dtype=np.int64)
    data[1, :3] = [-1, 0, 5]
    assert data[1].sum() > 0
    d = np.asfortranarray(data).ravel(order="K")
    h = C.c_void_p()
    rc = _lib.lib().nhp_disc_dataset_create(ctx.h, _lib.iptr(d), 3, 40, C.byref(h))
    assert rc == _lib.EDOMAIN and not h.value
    with pytest.raises(nhp.DomainError, match="counts must be non-negative"):
        _lib.check(rc, ctx.h)
    with pytest.raises(nhp.DomainError, match="counts must be non-negative"):
        nhp.convolve(gibbs_case(nhp, 3, 40, 2, 4, data, np.full(3, 0.2), seed=1)[0], data)
    data[1, 0] = 1
    assert nhp.DiscreteDataset(ctx, data).T == 40
