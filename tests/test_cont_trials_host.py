"""Several trials of a continuous process, the part that needs no GPU: stack_event_trials and its checks, how a list is told
from a triple, the integer restatements of tests/cont_trials_ref.py against a brute-force loop, and the LEAK CHECK -- for
every input of tests/test_cont_trials_gpu.py the reference's value on the naive concatenation differs from the per-trial sum
by at least 10³ times the tolerance the GPU test holds, so a library that lets windows cross the seams cannot pass there."""
import numpy as np
import pytest

import cont_trials_ref as tr


def _trials():
    return [(np.array([0.0, 0.5, 1.0]), np.array([1, 2, 1]), 1.0), (np.zeros(0), np.zeros(0, dtype=np.int64), 0.5),
            (np.array([0.0, 0.25]), np.array([2, 2]), 2.0)]


def test_stack_event_trials_matches_the_restatement(nhp):
    st = nhp.stack_event_trials(_trials())
    t, nd, f, o = tr.stack(_trials())
    assert isinstance(st, nhp.StackedEvents) and st.ntrials == 3
    assert np.array_equal(st.events, t) and np.array_equal(st.nodes, nd)
    assert np.array_equal(st.event_offsets, f) and np.array_equal(st.time_offsets, o)
    assert st.events.dtype == np.float64 and st.nodes.dtype == np.int64 and st.duration == 3.5
    assert list(st.events) == [0.0, 0.5, 1.0, 1.5, 1.75]               # T_0's last event and trial 2's first keep their order
    e, n, T = st                                                        # unpacks like a triple
    assert e is st.events and n is st.nodes and T == 3.5 and st[2] == 3.5
    assert nhp.stack_event_trials(st) is st


def test_stack_event_trials_checks(nhp):
    ok = _trials()
    with pytest.raises(ValueError, match="non-empty list"):
        nhp.stack_event_trials([])
    with pytest.raises(ValueError, match="trial 1 is not"):
        nhp.stack_event_trials([ok[0], (np.zeros(1), 1.0)])
    with pytest.raises(ValueError, match="trial 0: events must be sorted"):
        nhp.stack_event_trials([(np.array([0.5, 0.25]), np.array([1, 1]), 1.0)])
    with pytest.raises(nhp.DomainError, match=r"trial 1: events must lie in \[0, 1.0\]"):
        nhp.stack_event_trials([ok[0], (np.array([0.5, 1.5]), np.array([1, 1]), 1.0)])
    with pytest.raises(nhp.DomainError, match="trial 0: events must lie"):
        nhp.stack_event_trials([(np.array([-0.5, 0.5]), np.array([1, 1]), 1.0)])
    with pytest.raises(nhp.DomainError, match="trial 0: events must lie"):
        nhp.stack_event_trials([(np.array([0.5, np.nan]), np.array([1, 1]), 1.0)])
    for T in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(nhp.DomainError, match="trial 2: duration"):
            nhp.stack_event_trials([ok[0], ok[1], (np.zeros(0), np.zeros(0, dtype=np.int64), T)])
    with pytest.raises(ValueError, match="trial 0: events and nodes must be 1-D and of the same length"):
        nhp.stack_event_trials([(np.array([0.5]), np.array([1, 1]), 1.0)])


def test_a_list_of_tuples_is_trials_and_a_triple_one_recording(nhp):
    from nhp_amd.continuous import _is_trial_list, as_data
    ok = _trials()
    assert _is_trial_list(ok) and _is_trial_list(ok[:1])
    assert not _is_trial_list(ok[0])                                    # a 3-tuple: one recording
    assert not _is_trial_list(tuple(ok))                                # a tuple of three tuples is still (events, nodes, duration)-shaped
    assert not _is_trial_list([ok[0][0], ok[0][1], 1.0])                # the triple written as a list: one recording, as ever
    assert not _is_trial_list([])
    from nhp_amd.continuous import ntrials_of
    one = ok[0]
    assert as_data(one) is one and ntrials_of(one) == 1 and ntrials_of([one]) == 1 and ntrials_of(ok) == 3
    st = as_data(ok)
    assert isinstance(st, nhp.StackedEvents) and as_data(st) is st and ntrials_of(st) == 3
    ok[2] = (np.array([0.0, 0.5]), np.array([2, 2]), 2.0)
    assert as_data(ok).events[-1] == 2.0                                # nothing is kept: a changed list is stacked as it is now
    with pytest.raises(NotImplementedError, match="several trials"):
        nhp.ShardedDataset(None, ok)
    with pytest.raises(NotImplementedError, match="several trials"):
        nhp.ShardedDataset(None, st)


@pytest.mark.parametrize("name", ["counts", "ties", "wide", "inf", "empty-ends"])
def test_integer_restatements_against_a_loop(name):
    c = tr.case(name)
    t, nd, f, o = tr.stack(c["trials"])
    M = len(t)
    assert np.all(np.diff(t) >= 0) and f[-1] == M
    assert np.all(t * 2.0 ** 20 == np.round(t * 2.0 ** 20)) and o[-1] <= 2.0 ** 10
    first = tr.window_starts(t, f, c["dt_max"])
    g = tr.first_positive(t, f, o)
    rs = tr.recursive_starts(t, f, g, 1.5)
    rinf = tr.recursive_starts(t, f, g, np.inf)
    for r in range(len(f) - 1):
        for i in range(f[r], f[r + 1]):
            want = [j for j in range(f[r], i) if t[j] > t[i] - c["dt_max"]]
            assert first[i] == (want[0] if want else i), (name, i)
            local = [j for j in range(f[r], i) if t[j] > o[r]]
            assert rinf[i] == (local[0] if local else i)
            cutw = [j for j in local if t[j] > t[i] - 1.5]
            assert rs[i] == (cutw[0] if cutw else i)
        assert all(t[j] == o[r] for j in range(f[r], g[r])) and (g[r] == f[r + 1] or t[g[r]] != o[r])
    if name == "ties":                                                  # equal stacked times on the two sides of a seam
        assert all(t[f[r] - 1] == t[f[r]] == o[r] for r in (1, 2)) and np.array_equal(g, f[:-1] + 2)
    if name in ("wide", "inf"):                                         # every earlier event of the trial is a parent
        assert np.array_equal(first, f[tr.trial_of(f, M)])
    near = [(t[f[r]] - o[r] < c["dt_max"], o[r] - t[f[r] - 1] < c["dt_max"]) for r in range(1, len(f) - 1) if f[r] - f[r - 1] >= 2 and f[r + 1] - f[r] >= 2]
    assert near and all(a and b for a, b in near)                       # events within Δtmax on both sides of the seams
                                                                        # between trials of two or more events


@pytest.mark.parametrize("name", tr.LL_CASES)
def test_leak_check_windowed(name):
    c, m, res, tail = tr.prepared(name)
    ll = float(res.ll)
    leak = abs(tr.naive_ll(m, c["trials"]) - ll)
    assert leak >= 1e3 * tr.REL_LL * abs(ll), (name, leak)


@pytest.mark.parametrize("name", tr.REC_CASES + ("slow",))      # ("silent" has W = 0: no excitation, nothing to leak; see its case)
def test_leak_check_recursive(name):
    c, m, res, tail = tr.prepared(name, True)
    ll = float(res.ll)
    leak = abs(tr.naive_ll(m, c["trials"], recursive=True) - ll)
    assert leak >= 1e3 * tr.REL_LL * abs(ll), (name, leak)


@pytest.mark.parametrize("name", tr.COMP_SMALL + tr.COMP_EDGES)
def test_leak_check_compensator(name):
    c = tr.case(name)
    m = tr.gr.model_of(c)
    want = tr.compensator(m, c["trials"])
    leak = np.abs(tr.naive_total(m, c["trials"]) - np.asarray(want.total.value, dtype=np.float64))
    assert np.all(leak >= 1e3 * want.total.bound), (name, leak, want.total.bound)


def test_refusals_come_before_any_device_work(nhp, monkeypatch):
    """intensity at query times and forecast on several trials raise before a context is made or a dataset stacked or built: the
    builder is replaced by a tripwire, and there is no GPU here for a context anyway.  (The LGCP refusal sits in device_dataset,
    behind the context its caller made and before stacking and upload: tests/test_cont_trials_gpu.py.)"""
    from nhp_amd import continuous
    import cont_grad_ref as gr

    def tripwire(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(continuous, "DeviceDataset", type("Tripwire", (), {"__init__": tripwire}))
    monkeypatch.setattr(continuous, "stack_event_trials", tripwire)
    c = tr.case("ties")
    proc = gr.process_of(nhp, c)
    st = tr.stack(c["trials"])
    stacked = nhp.StackedEvents(st[0], st[1], st[3][-1], st[2], st[3])
    for data in (c["trials"], stacked):
        with pytest.raises(NotImplementedError, match="intensity at query times is not available on several trials"):
            nhp.intensity(proc, data, 0.5)
        with pytest.raises(NotImplementedError, match="forecast is not available on several trials"):
            nhp.forecast(proc, data, 1.0, nsamples=2)


def test_per_trial_sum_of_one_trial_is_the_plain_reference():
    c = tr.case("ties")
    m = tr.gr.model_of(c)
    one = c["trials"][:1]
    res, tail = tr.evaluate(m, one)
    e, n, T = one[0]
    plain = tr.gr.evaluate(m, e, n, T)
    assert float(res.ll) == float(plain.ll) and np.array_equal(np.asarray(res.grad, dtype=np.float64), np.asarray(plain.grad, dtype=np.float64))
    comp = tr.compensator(m, one)
    ref = tr.ce.evaluate(m, e, n, T)
    assert np.array_equal(np.asarray(comp.at_events.value, dtype=np.float64), np.asarray(ref.at_events.value, dtype=np.float64))
    assert np.array_equal(comp.at_events.bound, ref.at_events.bound)   # one trial: no prefix is subtracted, no extra allowance
