"""Independent trials, the host side: stack_trials and its refusals, the refusals a trial list meets before any device work,
and proof that the inputs of tests/test_disc_trials_gpu.py can see a leak: on every shape that file convolves, the per-trial
reference differs from the oracle's convolution of the naive concatenation in the first bins of every trial after the
first, and nowhere else."""
import numpy as np
import pytest

import disc_trials_ref as tr


def counts(N, T, seed=0):
    return np.random.default_rng(seed).poisson(0.5, (N, T)).astype(np.int64)


def test_stack_trials_stacks_along_time(nhp):
    trials = [counts(3, 5, 1), counts(3, 1, 2), counts(3, 9, 3).astype(np.int32)]
    data, off = nhp.stack_trials(trials)
    assert data.dtype == np.int64 and off.dtype == np.int64
    assert np.array_equal(off, [0, 5, 6, 15]) and data.shape == (3, 15)
    for r, x in enumerate(trials):
        assert np.array_equal(data[:, off[r]:off[r + 1]], x)
    want, woff = tr.stack(trials)
    assert np.array_equal(data, want) and np.array_equal(off, woff)
    one, off1 = nhp.stack_trials((counts(2, 4),))                       # a tuple, one trial
    assert np.array_equal(off1, [0, 4]) and one.shape == (2, 4)


@pytest.mark.parametrize("bad", [[], (), [np.zeros((3, 4), dtype=np.int64), np.zeros((2, 4), dtype=np.int64)],
                                 [np.zeros((3, 4), dtype=np.int64), np.zeros((3, 0), dtype=np.int64)],
                                 [np.zeros((3, 4), dtype=np.int64), np.zeros(4, dtype=np.int64)],
                                 [np.zeros((3, 4, 1), dtype=np.int64)], np.zeros((3, 4), dtype=np.int64)],
                         ids=["empty list", "empty tuple", "differing N", "zero bins", "1-D entry", "3-D entry", "not a list"])
def test_stack_trials_value_errors(nhp, bad):
    with pytest.raises(ValueError) as e:
        nhp.stack_trials(bad)
    assert not isinstance(e.value, nhp.DomainError)


def test_stack_trials_negative_count(nhp):
    x = counts(3, 6)
    y = x.copy()
    y[1, 2] = -1
    with pytest.raises(nhp.DomainError, match="trial 1"):
        nhp.stack_trials([x, y])


def small_process(nhp, N=3, B=2, L=4, lgcp=False):
    th = np.full((N, N, B), 1.0 / B)
    if lgcp:
        x = np.linspace(0.0, 40.0, 5)
        base = nhp.DiscreteLogGaussianCoxProcess(x, np.full((5, N), 0.3), None, -1.0, 1.0)
    else:
        base = nhp.DiscreteHomogeneousProcess(np.full(N, 0.3), 1.0)
    return nhp.DiscreteStandardHawkesProcess(base, nhp.DiscreteGaussianImpulseResponse(th, L, 1.0),
                                             nhp.DenseWeightModel(np.full((N, N), 0.1)), 1.0)


def no_context(nhp, monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    from nhp_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was reached before the refusal")
    monkeypatch.setattr(_lib, "default_context", boom)


def test_trials_refused_with_an_lgcp_baseline_before_device_work(nhp, monkeypatch):
    no_context(nhp, monkeypatch)
    proc = small_process(nhp, lgcp=True)
    trials = [counts(3, 10, 1), counts(3, 12, 2)]
    for call in (lambda: nhp.convolve(proc, trials), lambda: nhp.loglikelihood(proc, trials), lambda: nhp.intensity(proc, tuple(trials)),
                 lambda: nhp.mle_(proc, trials), lambda: nhp.mcmc_(proc, trials, nsteps=1), lambda: nhp.disc_residuals(proc, trials)):
        with pytest.raises(NotImplementedError, match="trials"):
            call()


def test_streamed_svi_refuses_trials_before_device_work(nhp, monkeypatch):
    no_context(nhp, monkeypatch)
    proc = small_process(nhp)
    with pytest.raises(NotImplementedError, match="trials"):
        nhp.svi_(proc, [counts(3, 32, 1), counts(3, 32, 2)], nsteps=1, batch_bins=16, streamed=True)


def test_forecast_refuses_a_list_of_trials(nhp, monkeypatch):
    no_context(nhp, monkeypatch)
    proc = small_process(nhp)
    with pytest.raises(NotImplementedError, match="matrix of the trial to continue"):
        nhp.disc_forecast(proc, [counts(3, 10, 1), counts(3, 12, 2)], 5, nsamples=2)


def test_entry_checks_see_the_stacked_matrix(nhp, monkeypatch):
    """The shape and sufficient-statistics readers get the stacked matrix, not a ragged list; a bad trial list is refused at
    the entry of a call, before the device."""
    no_context(nhp, monkeypatch)
    from nhp_amd import discrete
    trials = [counts(3, 10, 1), counts(3, 7, 2)]
    stacked = tr.stack(trials)[0]
    tot, T = small_process(nhp).baseline.sufficient_statistics(trials)
    assert T == 17 and np.array_equal(tot, stacked.sum(axis=1))
    assert tuple(discrete._data_shape(trials)) == (3, 17) and tuple(discrete._data_shape(tuple(trials))) == (3, 17)
    proc = small_process(nhp)
    with pytest.raises(ValueError, match="nodes"):
        nhp.loglikelihood(proc, [counts(3, 10), counts(2, 10)])
    with pytest.raises(nhp.DomainError):
        nhp.mle_(proc, [counts(3, 10), -counts(3, 10) - 1])
    with pytest.raises(ValueError, match="batch_bins"):                 # svi_'s own check, on ΣT = 17 bins
        nhp.svi_(proc, trials, nsteps=1, batch_bins=10)
    plan = discrete._score_plan(proc, discrete._trials(trials), True, (trials, (10, 17)), 1, 0)
    assert plan[0][2] == (0, 17) and plan[1][2] == (10, 17)
    plan = discrete._score_plan(proc, discrete._trials(trials), False, tuple(trials), 1, 0)      # a tuple of two trials is data
    assert plan[0][2] == (0, 17)


@pytest.mark.parametrize("name", list(tr.CONV_CASES))
def test_the_gpu_shapes_can_see_a_leak(nhp, orc, name):
    N, lengths, B, L, rate, zero, big = tr.CONV_CASES[name]
    proc, trials = tr.conv_case(nhp, name)
    stacked, off = tr.stack(trials)
    assert [x.shape for x in trials] == [(N, T) for T in lengths]
    for r, x in enumerate(trials):
        assert (x.max() == 0) if r in zero else (x[:, -1].max() > 0), r   # a count in every trial's last bin
    if big is not None:
        assert stacked.max() > 255
    if L <= 64:                                                           # the bitmap kernel's rule: under one bin in eight occupied
        assert np.count_nonzero(stacked) < 0.125 * stacked.size
    phi = orc.disc_basis(L, B, 1.0)
    ref, naive = tr.convolve(orc, trials, phi), tr.convolve_naive(orc, trials, phi)
    assert ref.shape == naive.shape == (sum(lengths), N, B)
    same = np.ones(sum(lengths), dtype=bool)
    for first, reach in tr.leak_rows(lengths, L):
        assert np.all(ref[first] == 0.0)                                  # a trial's first bin has no history
        assert not np.array_equal(ref[first:first + reach], naive[first:first + reach]), first
        assert np.any(naive[first] > 0.0), first                          # the very first bin shows it
        same[first:first + reach] = False
    assert np.array_equal(ref[same], naive[same])
    if len(lengths) == 1:
        assert np.array_equal(ref, naive)
    # the dyadic basis of the column-sum check: every order of summation gives the same bits
    dy = tr.dyadic_basis(L, B)
    conv = tr.convolve(orc, trials, dy)
    assert np.array_equal(conv * 64.0, np.round(conv * 64.0)) and conv.sum() * 64.0 < 2.0 ** 50
    assert np.array_equal(conv.sum(axis=0), conv[::-1].sum(axis=0))
