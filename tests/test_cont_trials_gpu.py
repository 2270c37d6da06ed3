"""Several independent trials of a continuous process as one dataset (nhp_cont_dataset_create_trials), against
tests/cont_trials_ref.py: the definition restated trial by trial on the unshifted times.  Every input has times and durations
on the grid 2⁻¹⁰ with ΣT_r <= 2¹⁰, so the stacking is exact; tests/test_cont_trials_host.py shows for every input that a
library whose windows crossed the seams would be off by more than 10³ tolerances.

    layout        window starts, pair offsets, scalars and the three tables against the integer restatement; host-built =
                  device-built (host pointers and device tensors) byte for byte; one trial = the plain builders; every
                  validation error on both routes; a list of device tensors is stacked on the device
    windowed      log-likelihood (1e-11, the suites' tolerance), gradient (every entry inside cont_grad_ref's bound + the final
                  additions), total_intensity (compensator_exact_ref's λ bound), on a dataset that keeps its child slices
                  (NHP_CHUNK=4096, sl_rows > 0) and on one that does not (NHP_SLICES=0 and the exact records, sl_rows = 0);
                  enqueue (single and the pass of two), batch
    recursive     log-likelihood and gradient with a usable cut, without one (θmin = 1e-6; W = 0 under derivatives), each with
                  LL_RECURSIVE alone and with LL_FULL_RECURSION through nhp_cont_loglik and nhp_cont_loglik_grad; the route by
                  nhp_probe_recursive_window, the exported starts by the restatement
    information   nhp_cont_information and nhp_cont_hessian_vec (flags 0, 1 and 3) and the package's calls, entry by entry
                  against information_ref on each trial alone, added
    sampler       resample_parents on a fixed uniform stream = the oracle on each trial alone, sliced and unsliced; the Gibbs
                  statistics; the adjacency sweep against adjacency_ref fed the clipped windows
    others        expected_statistics against em_ref on each trial alone, one em_ step, map_parents / cascades, one device and
                  one host mle_ run, a short chain with each network model
    compensator   at_events, residuals, total inside compensator_exact_ref's bound + the prefix subtraction's allowance: trial
                  starts at 127 / 128 / 129, on either side of 8192, trials shorter than a chunk, a node absent from a trial,
                  empty trials, Δtmax = ∞, both impulses
    refusals      intensity at times, forecast, an LGCP baseline, lgcp_loglik, ShardedDataset: status and message on several
                  trials, accepted on one recording
"""
import ctypes as C

import numpy as np
import pytest

import adjacency_ref as ar
import compensator_exact_ref as ce
import cont_grad_ref as gr
import cont_trials_ref as tr
import em_ref as er
import information_ref as ir
from helpers import window_routes

pytestmark = pytest.mark.gpu

ROUTE_ENV = ("NHP_GRAD_SLICES", "NHP_PLIST", "NHP_EV8", "NHP_GROUP", "NHP_CHUNK", "NHP_SLICES", "NHP_SAMPLER_SLICES")
UNSLICED = {"NHP_SLICES": "0", "NHP_GRAD_SLICES": "0", "NHP_PLIST": "0", "NHP_EV8": "0"}     # the exact 16-byte records: δ = 0
SLICED = {"NHP_CHUNK": "4096"}


@pytest.fixture
def route(monkeypatch, nhp):
    def use(env):
        for k in ROUTE_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        nhp.invalidate_device_datasets()
    yield use
    for k in ROUTE_ENV:
        monkeypatch.delenv(k, raising=False)
    nhp.invalidate_device_datasets()


def dataset(nhp, c, build="host", device_tensors=False):
    from nhp_amd import continuous
    st = nhp.stack_event_trials(c["trials"])
    data = st
    if device_tensors:
        import torch
        dev = torch.device("cuda", nhp.default_context().device)
        data = nhp.StackedEvents(torch.as_tensor(st.events, device=dev), torch.as_tensor(st.nodes, device=dev), st.duration,
                                 st.event_offsets, st.time_offsets)
    return continuous.DeviceDataset(nhp.default_context(), data, c["N"], c["dt_max"], build=build)


def same_layout(a, b):
    la, lb = a.layout(), b.layout()
    assert la["scalars"] == lb["scalars"]
    for k in la["arrays"]:
        assert la["arrays"][k].tobytes() == lb["arrays"][k].tobytes(), k
    for x, y in zip(a.trials(), b.trials()):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("name", ["counts", "empty-ends", "ties", "wide", "inf", "dense"])
def test_layout_against_the_restatement_and_between_the_builds(nhp, route, name):
    route({})
    c = tr.case(name)
    t, nd, f, o = tr.stack(c["trials"])
    M, N = len(t), c["N"]
    ds = dataset(nhp, c)
    lay = ds.layout()
    child, sc = lay["arrays"]["child"], lay["scalars"]
    first = tr.window_starts(t, f, c["dt_max"])
    assert np.array_equal(np.sort(child["idx"]), np.arange(M)) and np.array_equal(child["t"], t[child["idx"]])
    assert np.array_equal(child["first"], first[child["idx"]])
    cw = lay["arrays"]["child_w"]
    assert np.array_equal(cw["first"], first[cw["idx"]])
    assert np.array_equal(lay["arrays"]["pair_off"], tr.pair_offsets(first, nd - 1, N))
    assert np.array_equal(lay["arrays"]["times"], t) and np.array_equal(lay["arrays"]["nodes"], nd - 1)
    pairs = int((np.arange(M) - first).sum())
    assert sc["M"] == M and sc["N"] == N and sc["pairs"] == pairs == ds.pairs
    assert sc["max_window"] == int((np.arange(M) - first).max())
    assert sc["n_zero_time"] == int((t[:f[1]] == 0.0).sum())            # trial 0's value
    assert sc["t_last"] == int(np.float64(t[-1]).view(np.int64))        # on the stacked clock
    if len(lay["arrays"]["poff"]):
        assert np.array_equal(lay["arrays"]["poff"], np.concatenate([[0], np.cumsum(cw["idx"] - cw["first"])]).astype(np.uint32))
    gf, go, gg = ds.trials()
    assert np.array_equal(gf, f) and np.array_equal(go, o) and np.array_equal(gg, tr.first_positive(t, f, o))
    assert ds.ntrials == len(c["trials"]) and ds.duration == o[-1]
    assert ds.trial_events(1) == (int(f[1]), int(f[2])) and ds.trial_interval(1) == (float(o[1]), float(o[2]))
    same_layout(ds, dataset(nhp, c, build="device"))
    same_layout(ds, dataset(nhp, c, device_tensors=True))


def test_one_trial_is_the_plain_dataset(nhp, route):
    from nhp_amd import continuous
    route({})
    c = tr.case("dense")
    e, n, T = c["trials"][0]
    ctx = nhp.default_context()
    for build in ("host", "device"):
        plain = continuous.DeviceDataset(ctx, (e, n, T), c["N"], c["dt_max"], build=build)
        one = continuous.DeviceDataset(ctx, (e, n, T), c["N"], c["dt_max"], build=build, trial_offsets=([0, len(e)], [0.0, T]))
        same_layout(plain, one)
        assert one.ntrials == 1 and plain.ntrials == 1 and one.duration == T
    proc = gr.process_of(nhp, c)
    assert nhp.loglikelihood(proc, [(e, n, T)], recursive=False) == nhp.loglikelihood(proc, (e, n, T), recursive=False)


def test_trials_given_as_device_tensors_are_stacked_on_the_device(nhp, route):
    import torch
    route({})
    c, m, res, tail = tr.prepared("ties")
    dev = torch.device("cuda", nhp.default_context().device)
    trials = [(torch.as_tensor(e, device=dev), torch.as_tensor(n, device=dev), T) for e, n, T in c["trials"]]
    st = nhp.stack_event_trials(trials)
    t, nd, f, o = tr.stack(c["trials"])
    assert st.events.device == dev and st.nodes.device == dev
    assert np.array_equal(st.events.cpu().numpy(), t) and np.array_equal(st.nodes.cpu().numpy(), nd)
    assert np.array_equal(st.event_offsets, f) and np.array_equal(st.time_offsets, o)
    proc = gr.process_of(nhp, c)
    assert abs(nhp.loglikelihood(proc, trials, recursive=False) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))
    with pytest.raises(nhp.DomainError, match="trial 1: events must lie"):
        nhp.stack_event_trials([trials[0], (trials[1][0] + 100.0, trials[1][1], 8.0)])


def test_every_validation_error_on_both_routes(nhp):
    from nhp_amd import continuous
    ctx = nhp.default_context()
    t = np.array([0.5, 1.0, 1.0, 1.5, 2.5])
    nd = np.array([1, 2, 1, 2, 1], dtype=np.int64)
    good = ([0, 3, 3, 5], [0.0, 1.0, 1.25, 3.0])
    cases = [
        (([1, 3, 3, 5], good[1]), nhp.NhpError, r"trial_event_offsets\[0\] = 1 must be 0"),
        (([0, 3, 2, 5], good[1]), nhp.NhpError, r"trial_event_offsets\[2\] = 2 is below trial_event_offsets\[1\] = 3"),
        (([0, 3, 3, 4], good[1]), nhp.NhpError, r"trial_event_offsets\[3\] = 4 must be n_events = 5"),
        ((good[0], [0.5, 1.0, 1.25, 3.0]), nhp.DomainError, r"trial_time_offsets\[0\] = 0.5 must be 0"),
        ((good[0], [0.0, 1.0, 1.0, 3.0]), nhp.DomainError, r"trial_time_offsets\[2\] = 1 must be finite and above trial_time_offsets\[1\] = 1"),
        ((good[0], [0.0, 1.0, 1.25, np.inf]), nhp.DomainError, r"trial_time_offsets\[3\] = inf must be finite"),
        (([0, 2, 2, 5], good[1]), nhp.DomainError, r"event 3 at 1 lies outside trial 3 = \[1.25, 3\]"),
        (([0, 4, 4, 5], good[1]), nhp.DomainError, r"event 4 at 1.5 lies outside trial 1 = \[0, 1\]"),
        ((good[0], [0.0, 1.0, 1.25, 2.0]), nhp.DomainError, r"event 5 at 2.5 lies outside trial 3 = \[1.25, 2\]"),
    ]
    for build in ("host", "device"):
        ds = continuous.DeviceDataset(ctx, (t, nd, 3.0), 2, 1.0, build=build, trial_offsets=good)
        assert ds.ntrials == 3 and ds.pairs == 1 + 2                    # (0.5 -> 1.0 twice and the tie; 1.5 -> 2.5 is exactly Δtmax: no pair)
        for offs, err, msg in cases:
            with pytest.raises(err, match=msg):
                continuous.DeviceDataset(ctx, (t, nd, 3.0), 2, 1.0, build=build, trial_offsets=offs)
        # two faults: the first failing event decides on both routes (event 3 outside its trial, before the bad node of event 5)
        with pytest.raises(nhp.DomainError, match=r"event 3 at 1 lies outside trial 3"):
            continuous.DeviceDataset(ctx, (t, np.array([1, 2, 1, 2, 7]), 3.0), 2, 1.0, build=build, trial_offsets=([0, 2, 2, 5], good[1]))
        with pytest.raises(nhp.DomainError, match="node id 3 at event 2"):       # the plain builders' errors stay
            continuous.DeviceDataset(ctx, (t, np.array([1, 3, 1, 2, 1]), 3.0), 2, 1.0, build=build, trial_offsets=good)
        with pytest.raises(nhp.NhpError, match=r"events must be sorted \(event 3\)"):
            continuous.DeviceDataset(ctx, (np.array([0.5, 1.0, 0.75, 1.5, 2.5]), nd, 3.0), 2, 1.0, build=build, trial_offsets=good)
    with pytest.raises(NotImplementedError, match="whole dataset"):
        continuous.DeviceDataset(ctx, (t, nd, 3.0), 2, 1.0, columns=(0, 1), trial_offsets=good)


# ---------------------------------------------------------------------------------------------------------------- windowed
def grad_of(nhp, proc, ds, flags=0):
    from nhp_amd import _lib
    ctx = nhp.default_context()
    model = proc.device_model(ctx)
    from nhp_amd.continuous import gradient_length
    P = gradient_length(proc)
    g, ll = np.full(P, np.nan), C.c_double()
    _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, flags, C.byref(ll), _lib.dptr(g), P), ctx.h)
    return ll.value, g


def loglik_flags(nhp, proc, ds, flags):
    """nhp_cont_loglik with the flags given (the package passes LL_RECURSIVE alone)."""
    from nhp_amd import _lib
    ctx = nhp.default_context()
    ll = C.c_double(np.nan)
    _lib.check(_lib.lib().nhp_cont_loglik(ctx.h, ds.h, proc.device_model(ctx).h, flags, C.byref(ll)), ctx.h)
    return ll.value


def hold(label, ll, g, res, N, delta=0.0, tail=None):
    want = float(res.ll)
    print(f"{label}: ll {ll!r} want {want!r} rel {abs(ll - want) / abs(want):.3g}")
    assert abs(ll - want) <= tr.REL_LL * abs(want), (label, ll, want)
    ratio, bad, err, B = gr.check(g, res, delta, tail)
    print(f"{label}: gradient error/bound {ratio:.3g}, {int((B == 0).sum())} entries equal to their constant")
    assert len(bad) == 0, f"{label}: {len(bad)} entries outside the bound\n" + gr.explain(g, res, N, bad, err, B)


def bit_length(v):
    return int(v).bit_length()


def event_intensity_ref(m, trials):
    parts = [ce.event_intensity(m, np.asarray(e, dtype=np.float64), n) for e, n, T in trials if len(e)]
    return ce.Lam(*[np.concatenate([getattr(p, k) for p in parts]) for k in ce.Lam._fields])


@pytest.mark.parametrize("name", tr.LL_CASES)
def test_windowed_loglikelihood_gradient_intensity(nhp, route, name):
    c, m, res, tail = tr.prepared(name)
    proc = gr.process_of(nhp, c)
    expo = c["kind"] == "exponential"
    routes = [("exact records", UNSLICED)]
    if name.startswith("dense"):
        routes.append(("slices", SLICED))
    for label, env in routes:
        route(env)
        ds = dataset(nhp, c)
        sc = ds.scalars()
        delta = 0.0
        if env is SLICED:
            assert sc["sl_rows"] > 0 and sc["n_items"] == c["N"], sc
            if expo:                                                     # the 6-byte records' delay step (test_cont_grad_edges_gpu.py)
                delta = c["dt_max"] * 2.0 ** -(48 - max(sc["sl_nb"], bit_length(sc["max_item"])))
        else:
            assert sc["sl_rows"] == 0, sc
        assert abs(nhp.loglikelihood(proc, ds, recursive=False) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))
        ll, g = grad_of(nhp, proc, ds)
        hold(f"{name} {label}", ll, g, res, c["N"], delta=delta, tail=tail)
        lam = nhp.total_intensity(proc, ds)
        want = event_intensity_ref(m, c["trials"])
        ratio, bad = ce.check_intensity(lam, want, delta=delta)[:2]
        print(f"{name} {label}: total_intensity error/bound {ratio:.3g}")
        assert len(bad) == 0, (name, label, bad[:5])
    # the list itself, through device_dataset
    route({})
    assert abs(nhp.loglikelihood(proc, c["trials"], recursive=False) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))


@pytest.mark.parametrize("env", [SLICED, UNSLICED], ids=["slices", "exact"])
def test_enqueue_and_batch_forms(nhp, route, env):
    from nhp_amd import _lib
    c, m, res, tail = tr.prepared("dense")
    c2 = dict(c, W=c["W"] * 0.5, theta=c["theta"] * 1.25)
    res2, _ = tr.evaluate(gr.model_of(c2), c["trials"])
    route(env)
    ctx = nhp.default_context()
    ds = dataset(nhp, c)
    assert (ds.scalars()["sl_rows"] > 0) == (env is SLICED)
    procs = [gr.process_of(nhp, c), gr.process_of(nhp, c2)]
    models = [p.device_model(ctx) for p in procs]
    want = np.array([float(res.ll), float(res2.ll)])
    lib = _lib.lib()
    for k in (0, 1):                                                    # a streak of two: one pass over the records where sliced
        _lib.check(lib.nhp_cont_loglik_enqueue(ctx.h, ds.h, models[k].h, 0, 4 + k), ctx.h)
    got = ctx.fetch(4, 2)
    assert np.all(np.abs(got - want) <= tr.REL_LL * np.abs(want)), (got, want)
    _lib.check(lib.nhp_cont_loglik_enqueue(ctx.h, ds.h, models[1].h, 0, 9), ctx.h)
    assert abs(ctx.fetch(9, 1)[0] - want[1]) <= tr.REL_LL * abs(want[1])
    out = np.full(2, np.nan)
    hs = (C.c_void_p * 2)(models[0].h, models[1].h)
    _lib.check(lib.nhp_cont_loglik_batch(ctx.h, ds.h, hs, 2, 0, _lib.dptr(out)), ctx.h)
    assert np.all(np.abs(out - want) <= tr.REL_LL * np.abs(want)), (out, want)


# --------------------------------------------------------------------------------------------------------------- recursive
def probe(nhp, proc, ds, cost):
    from nhp_amd import _lib
    ctx = nhp.default_context()
    out = np.full(4, np.nan)
    _lib.check(_lib.lib().nhp_probe_recursive_window(ctx.h, ds.h, proc.device_model(ctx).h, cost, _lib.dptr(out)), ctx.h)
    return out


def hold_starts(label, ds, c, cut):
    t, nd, f, o = tr.stack(c["trials"])
    want = tr.recursive_starts(t, f, tr.first_positive(t, f, o), cut)
    cc = ds.array("child_cut")
    assert len(cc) == len(t), label
    bad = np.nonzero(cc["first"] != want[cc["idx"]])[0]
    assert len(bad) == 0, (label, cut, cc[bad[:5]], want[cc["idx"][bad[:5]]])
    return int((np.arange(len(t)) - want).sum())


@pytest.mark.parametrize("name", tr.REC_CASES)
def test_recursive_route_with_a_usable_cut_or_from_the_trial_start(nhp, route, name):
    route({})
    c, m, res, tail = tr.prepared(name, True)
    proc = gr.process_of(nhp, c)
    ds = dataset(nhp, c)
    assert window_routes(nhp, proc, ds) == [1, 1, 1]                    # several trials: always the window
    out = probe(nhp, proc, ds, 1.2)
    M, span = len(ds), ds.duration
    t = tr.stack(c["trials"])[0]
    usable = out[0] > 1e-300 and out[0] * M / t[-1] <= 8192.0
    assert usable, (name, out)                                          # (test_recursive_route_without_a_cut has the others)
    cut = out[0]
    pairs = hold_starts(name, ds, c, cut)
    assert out[3] == pairs
    if name.startswith("cut"):                                           # clipped at g_r AND at the cut: neither alone gives these starts;
        assert cut < 8.0                                                 # the other cases' cut is longer than a trial: they start at g_r
        f, o = ds.trials()[:2]
        g_only = tr.recursive_starts(t, f, tr.first_positive(t, f, o), np.inf)
        cut_only = np.minimum(np.searchsorted(t, t - cut, side="right"), np.arange(M))
        want = tr.recursive_starts(t, f, tr.first_positive(t, f, o), cut)
        assert (want != g_only).any() and (want != cut_only).any()
    wt = tr.window_tail(res, m, c["trials"]) + tail
    for flags in (1, 3):                                                 # LL_RECURSIVE, + LL_FULL_RECURSION: the same window
        ll, g = grad_of(nhp, proc, ds, flags)
        hold(f"{name} flags {flags}", ll, g, res, c["N"], tail=wt)
        # the log-likelihood's own caller (nhp_launch_recursive_flags): with LL_FULL_RECURSION too it is the window sum -- the
        # recursion kernels would carry their state across the seams and return the concatenation's value (the host leak check)
        assert abs(loglik_flags(nhp, proc, ds, flags) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll)), (name, flags)
    assert abs(nhp.loglikelihood(proc, c["trials"], recursive=True) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))


@pytest.mark.parametrize("name", tr.REC_NO_CUT)
def test_recursive_route_without_a_cut(nhp, route, name):
    """θmin = 1e-6 puts the cut's expected window far above 8192 parents; W = 0 gives the empty cut, which no derivative may use:
    both walk from g_r.  The data hold an event at exactly local time 0 in trials 1 and 2 and one at exactly T_r in the trials
    before them."""
    route({})
    c, m, res, tail = tr.prepared(name, True)
    proc = gr.process_of(nhp, c)
    ds = dataset(nhp, c)
    assert window_routes(nhp, proc, ds) == [1, 1, 1]
    out = probe(nhp, proc, ds, 1.2)
    if name == "slow":
        assert out[0] * len(ds) / ds.duration > 8192.0
    else:
        assert out[0] == 1e-300
    hold_starts(name, ds, c, np.inf)
    for flags in (1, 3):
        ll, g = grad_of(nhp, proc, ds, flags)
        hold(f"{name} flags {flags}", ll, g, res, c["N"], tail=tail)
    assert abs(loglik_flags(nhp, proc, ds, 3) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))
    if name == "silent":                                                 # the log-likelihood alone may take the empty window
        assert abs(nhp.loglikelihood(proc, ds, recursive=True) - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))
        assert np.array_equal(ds.array("child_cut")["first"], ds.array("child_cut")["idx"])


INFO_CASES = [("ties", 0), ("ties-logit", 0), ("ties-net", 0), ("cut", 1), ("cut", 3), ("cut-net", 1), ("ties", 1), ("ties", 3), ("slow", 1)]


@pytest.mark.parametrize("name,flags", INFO_CASES)
def test_observed_information_and_hessian_vector_product(nhp, route, name, flags):
    """nhp_cont_information and nhp_cont_hessian_vec on the stacked dataset against information_ref evaluated on each trial alone
    and added (its bounds added, + the final additions, + the truncated window's tail for the recursive objective), entry by
    entry; flags = 3 (LL_FULL_RECURSION) is the same window sum on several trials, where one recording refuses it."""
    from nhp_amd import _lib
    route({})
    c = tr.case(name)
    m, rec = gr.model_of(c), flags != 0
    res, tails = tr.information(m, c["trials"], recursive=rec)
    proc = gr.process_of(nhp, c)
    ctx, N = nhp.default_context(), c["N"]
    ds = dataset(nhp, c)
    model = proc.device_model(ctx)
    D = 1 + res.kinds * N
    cols = np.arange(N, dtype=np.int32)
    out, ll = np.full((N, D, D), np.nan), C.c_double(np.nan)
    _lib.check(_lib.lib().nhp_cont_information(ctx.h, ds.h, model.h, flags, cols.ctypes.data_as(C.POINTER(C.c_int32)), N, 0, 0, C.byref(ll),
                                               out.ctypes.data), ctx.h)
    assert abs(ll.value - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))
    if rec:
        tails = [tails[k] + tr.information_window_tail(res, k, m, c["trials"]) for k in range(N)]
    def hold_blocks(label, blocks):
        worst = 0.0
        for k in range(N):
            got = np.asarray(blocks[k])
            assert np.array_equal(got, got.T)
            ratio, bad, err, B = ir.check(got, res, k, tails[k])
            assert len(bad) == 0, f"{label}: {len(bad)} entries outside the bound\n" + ir.explain(got, res, k, bad, err, B)
            worst = max(worst, ratio)
        print(f"{label}: information error/bound {worst:.3g}")

    hold_blocks(f"{name} flags {flags}", out.transpose(0, 2, 1))
    if flags in (0, 1):                                                  # the package's call, on the list itself (the sums go through LDS
        info = nhp.observed_information(proc, c["trials"], recursive=rec)   # adds in any order: two calls need not agree in the last bits)
        assert abs(info.ll - float(res.ll)) <= tr.REL_LL * abs(float(res.ll))
        hold_blocks(f"{name} recursive={rec}, package", info.blocks)
        se = nhp.standard_errors(proc, c["trials"], recursive=rec)
        assert np.all(np.isfinite(se.se) | np.isnan(se.se))
    P = N + res.kinds * N * N
    v = np.random.default_rng(5).normal(size=P)
    hv = np.full(P, np.nan)
    _lib.check(_lib.lib().nhp_cont_hessian_vec(ctx.h, ds.h, model.h, flags, 0, v.ctypes.data, hv.ctypes.data, P), ctx.h)
    want, B = ir.hvp(res, v, N)
    kinds = res.kinds
    for k in range(N):
        idx = ir.block_index(N, kinds, k)
        B[idx] = B[idx] + np.where(res.S[k] @ np.abs(v[idx]) > 0, tails[k] @ np.abs(v[idx]), 0.0)
    results = [hv] + ([nhp.hessian_vector_product(proc, c["trials"], v, recursive=rec)] if flags in (0, 1) else [])
    for got in results:
        err = np.abs(got - np.asarray(want, dtype=np.float64))
        assert np.all(np.where(B > 0, err <= B, got == 0.0)), (name, flags, float((err / np.where(B > 0, B, 1.0)).max()))


# ------------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("name", ["dense", "dense-logit", "ties", "ties-net"])
def test_parents_equal_the_oracle_on_each_trial_alone(nhp, orc, route, name):
    c = tr.case(name)
    om = gr.oracle_model(orc, c)
    proc = gr.process_of(nhp, c)
    t, nd, f, o = tr.stack(c["trials"])
    M = len(t)
    u = np.random.default_rng(7).uniform(size=M)
    want_p, want_n = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for r, (e, n, T) in enumerate(c["trials"]):
        if len(e):
            p, pn = orc.resample_parents(om, e, n, u[f[r]:f[r + 1]], flags=orc.MATH_DET)
            want_p[f[r]:f[r + 1]] = np.where(p > 0, p + f[r], 0)
            want_n[f[r]:f[r + 1]] = pn
    for env in ([SLICED, UNSLICED] if name.startswith("dense") else [UNSLICED]):
        route(env)
        ds = dataset(nhp, c)
        assert (ds.scalars()["sl_rows"] > 0) == (env is SLICED)
        got_p, got_n, st = nhp.resample_parents(proc, ds, u=u, with_stats=True)
        assert np.array_equal(got_p, want_p) and np.array_equal(got_n, want_n)
        assert np.all((got_p == 0) | (got_p > f[tr.trial_of(f, M)]))    # no parent before the trial's first event
        N = c["N"]
        assert np.array_equal(st["Mn"], nhp.node_counts(nd, N))
        assert np.array_equal(st["Mnm"].reshape((N, N), order="F"), nhp.parent_counts(nd, want_n, N))
        assert np.array_equal(st["cnt0"], np.bincount(nd[want_n == 0] - 1, minlength=N).astype(np.float64))


def test_adjacency_sweep_against_the_reference_fed_the_clipped_windows(nhp, route, monkeypatch):
    route({})
    c = tr.case("dense-net")
    t, nd, f, o = tr.stack(c["trials"])
    M, N = len(t), c["N"]
    first = tr.window_starts(t, f, c["dt_max"])

    def clipped(times, dt_max):
        cnt = np.arange(M) - first
        k = np.repeat(np.arange(M), cnt)
        return k, np.arange(len(k)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(first, cnt)
    monkeypatch.setattr(ar, "window_pairs", clipped)
    model = ar.Model(c["lam0"], c["W"], theta=c["theta"], dt_max=c["dt_max"])
    u = np.random.default_rng(3).uniform(size=(N, N))
    A0 = c["A"]
    want, d, B = ar.sweep(model, t, nd, o[-1], 0.5, u, A0)
    proc = gr.process_of(nhp, c)
    links = nhp.resample_adjacency_matrix_(proc, c["trials"], u=u)
    with np.errstate(divide="ignore"):
        margin = np.abs(np.asarray(d, dtype=np.float64) - np.log(u / (1.0 - u)))
    decided = margin > 4.0 * B + 1e-12                                  # entries whose decision no rounding can flip
    assert decided.sum() >= N * N - 1
    assert np.array_equal(proc.adjacency_matrix[decided], want[decided]) and links == proc.adjacency_matrix.sum()


# ------------------------------------------------------------------------------------------------------- other entry points
def test_expected_statistics_em_map_parents_cascades_and_mle(nhp, route):
    route({})
    c = tr.case("dense")
    trials = c["trials"]
    t, nd, f, o = tr.stack(trials)
    M, N = len(t), c["N"]
    proc = gr.process_of(nhp, c)
    # against tests/em_ref.py on each trial alone, added; test_em_gpu.py's tolerance.  (em_ref's recursive pairs take every
    # earlier event, so the recursive leg runs on "counts", whose trials have no event at local time 0.)
    for cc, rec in ((c, False), (tr.case("counts"), True), (tr.case("counts-logit"), False)):
        pc = gr.process_of(nhp, cc)
        em_model = er.Model.of(pc)
        whole = nhp.expected_statistics(pc, cc["trials"], recursive=rec)
        assert all((e > 0.0).all() for e, n, T in cc["trials"]) or not rec
        parts = [er.statistics(em_model, er.Pairs(e, n, T, cc["N"], cc["dt_max"], recursive=rec)) for e, n, T in cc["trials"] if len(e)]
        for i, k in ((1, "bg"), (2, "EM"), (3, "S1"), (4, "S2")):
            if parts[0][i] is None:
                assert getattr(whole, k) is None
                continue
            want = sum(p[i] for p in parts)
            assert np.all(np.abs(getattr(whole, k) - want) <= 1e-10 * np.maximum(1.0, np.abs(want))), (cc["name"], k, rec)
        res, _ = tr.evaluate(gr.model_of(cc), cc["trials"], recursive=rec)
        assert abs(whole.ll - float(res.ll)) <= tr.REL_LL * abs(whole.ll)
    # one EM step from the case's parameters: the M-step's closed form on the per-trial sums, exposure ΣT_r
    whole = nhp.expected_statistics(proc, trials, recursive=False)
    fit = gr.process_of(nhp, c)
    nhp.em_(fit, trials, max_steps=1, guess=proc.params(), recursive=False)
    assert np.abs(fit.baseline.λ - np.clip(whole.bg / o[-1], 1e-6, 10.0)).max() <= 1e-11
    cnt = nhp.node_counts(nd, N)
    assert np.abs(fit.weights.W - np.clip(whole.EM / cnt[:, None], 1e-6, 10.0)).max() <= 1e-11
    # map_parents / cascades: no cascade spans a seam, and each trial alone gives the same parents
    par, pno, prob = nhp.map_parents(proc, trials)
    trial = tr.trial_of(f, M)
    assert np.all((par == 0) | (par > f[trial]))
    for r, trl in enumerate(trials):
        if len(trl[0]):
            p1, n1, q1 = nhp.map_parents(proc, trl)
            assert np.array_equal(par[f[r]:f[r + 1]], np.where(p1 > 0, p1 + f[r], 0)) and np.array_equal(prob[f[r]:f[r + 1]], q1)
    cas = nhp.cascades(proc, trials, parents="map")
    assert np.array_equal(trial[cas.root - 1], trial)                   # every event's root lies in its own trial
    # one device mle_ run: its objective is the per-trial sum at the solution
    fit = gr.process_of(nhp, c)
    out = nhp.mle_(fit, trials, optimizer="device", guess=proc.params(), recursive=False, max_steps=3)
    cf = dict(c, lam0=fit.baseline.λ.copy(), theta=fit.impulses.θ.copy(), W=fit.weights.W.copy())
    want = float(tr.evaluate(gr.model_of(cf), trials)[0].ll)
    print(f"mle_ device: {out.steps} steps, objective {out.maximum!r}, per-trial sum {want!r}")
    assert abs(out.maximum - want) <= 1e-9 * abs(want)
    host = gr.process_of(nhp, c)
    out_h = nhp.mle_(host, trials, guess=proc.params(), recursive=False, max_steps=3)
    ch = dict(c, lam0=host.baseline.λ.copy(), theta=host.impulses.θ.copy(), W=host.weights.W.copy())
    assert abs(out_h.maximum - float(tr.evaluate(gr.model_of(ch), trials)[0].ll)) <= 1e-9 * abs(want)


def test_a_short_chain_runs_on_trials(nhp, route):
    route({})
    c = tr.case("dense-net")
    proc = gr.process_of(nhp, c)
    res = nhp.mcmc_(proc, c["trials"], nsteps=5, seed=1, keep_samples=False, moments=True, diagnostics=True)
    assert res.steps == 5 and np.all(np.isfinite(proc.params()))
    N = c["N"]
    for network in (nhp.DenseNetworkModel(N), nhp.StochasticBlockNetworkModel(N, 2, z=np.arange(N) % 2),
                    nhp.LatentDistanceNetworkModel(N, 2, z=0.1 * np.random.default_rng(2).standard_normal((N, 2)), σ=2.0, σb=2.0)):
        proc = gr.process_of(nhp, c)
        proc.network = network
        res = nhp.mcmc_(proc, c["trials"], nsteps=3, seed=1, keep_samples=False, moments=True)
        assert res.steps == 3 and np.all(np.isfinite(res.mean)), type(network).__name__
    std = gr.process_of(nhp, tr.case("dense"))
    res = nhp.mcmc_(std, tr.case("dense")["trials"], nsteps=3, seed=1, device_draws=False)
    assert res.steps == 3 and np.all(np.isfinite(std.params()))


# -------------------------------------------------------------------------------------------------------------- compensator
def hold_compensator(label, nhp, c, trials, want=None):
    m = gr.model_of(c)
    want = want or tr.compensator(m, trials)
    proc = gr.process_of(nhp, c)
    got = nhp.compensator(proc, trials)
    worst = {}
    for k in ("at_events", "residuals", "total"):
        ratio, bad, err, B = ce.check(getattr(got, k), getattr(want, k))
        worst[k] = ratio
        assert len(bad) == 0, f"{label} {k}: {len(bad)} outside the bound\n" + ce.explain(getattr(got, k), getattr(want, k), bad, err, B)
    print(f"{label}: error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return got, want


@pytest.mark.parametrize("name", tr.COMP_SMALL)
def test_compensator_small_cases(nhp, route, name):
    """Trials shorter than one chunk (the no-prefix path: the allowance is 0 there), a node absent from a trial, empty trials."""
    route({})
    c = tr.case(name)
    got, want = hold_compensator(name, nhp, c, c["trials"])
    t, nd, f, o = tr.stack(c["trials"])
    for r, (e, n, T) in enumerate(c["trials"]):
        if len(e) == 0:                                                  # an empty trial adds λ0·T_r to total and nothing else
            rest = c["trials"][:r] + c["trials"][r + 1:]
            other = nhp.compensator(gr.process_of(nhp, c), rest).total
            assert np.abs(got.total - other - c["lam0"] * T).max() <= 4 * 2.0 ** -53 * np.abs(got.total).max()
            break
    tst = nhp.time_rescaling_test(gr.process_of(nhp, c), c["trials"])
    assert 0.0 <= tst.statistic <= 1.0 and tst.counts.sum() == len(t)


@pytest.mark.parametrize("name", tr.COMP_EDGES)
def test_compensator_trial_starts_at_the_chunk_and_group_edges(nhp, route, name):
    route({})
    c = tr.case(name)
    t, nd, f, o = tr.stack(c["trials"])
    if name.startswith("chunk"):
        assert [int(v) % 128 for v in f[1:4]] == [127, 0, 1] and not (c["trials"][1][1] == 2).any()
    else:
        assert list(f) == [0, 4000, 8191, 8193, 8300]
    got, want = hold_compensator(name, nhp, c, c["trials"])
    used = f[tr.trial_of(f, len(t))] < want.ws // 128 * 128
    assert used.any() and (~used).any()                                 # both paths of k_comp_events


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_several_trials_and_acceptance_of_one_recording(nhp, route):
    from nhp_amd import _lib, continuous
    route({})
    c = tr.case("ties")
    trials, one = c["trials"], c["trials"][0]
    proc = gr.process_of(nhp, c)
    ctx = nhp.default_context()
    ds = dataset(nhp, c)
    model = proc.device_model(ctx)
    lib = _lib.lib()
    q, out = np.array([0.5]), np.empty(c["N"])
    # the library (a Julia host reaches these directly): NHP_ENOTIMPL and the reason
    assert lib.nhp_cont_intensity(ctx.h, ds.h, model.h, _lib.dptr(q), 1, _lib.dptr(out)) == _lib.ENOTIMPL
    assert b"intensity at query times: not available on a dataset of 3 trials" in lib.nhp_last_error(ctx.h)
    counts = np.empty((2, c["N"]), dtype=np.int64)
    carry, phase = np.empty(c["N"]), np.zeros(2)
    rc = lib.nhp_cont_forecast(ctx.h, ds.h, model.h, 1.0, 2, 0, 1000, 0, carry.ctypes.data, counts.ctypes.data, None, None, None, _lib.dptr(phase))
    assert rc == _lib.ENOTIMPL and b"forecast: not available on a dataset of 3 trials" in lib.nhp_last_error(ctx.h)
    gx = np.array([0.0, 12.0, 24.0])
    lg = nhp.ContinuousStandardHawkesProcess(nhp.LogGaussianCoxProcess(gx, [np.ones(3) for _ in range(c["N"])]), proc.impulses, proc.weights)
    ll = C.c_double()
    lls = np.empty(c["N"])                                               # lgcp_loglik writes one value per node
    rc = lib.nhp_cont_loglik(ctx.h, ds.h, lg.device_model(ctx).h, 0, C.byref(ll))
    assert rc == _lib.ENOTIMPL and b"LogGaussianCoxProcess baseline: not available on a dataset of 3 trials" in lib.nhp_last_error(ctx.h)
    lam = np.ones((c["N"], 3))
    rc = lib.nhp_cont_lgcp_loglik(ctx.h, ds.h, None, _lib.dptr(gx), 3, _lib.dptr(lam), _lib.dptr(lls))
    assert rc == _lib.ENOTIMPL and b"lgcp_loglik: not available on a dataset of 3 trials" in lib.nhp_last_error(ctx.h)
    # the package, before any device work
    with pytest.raises(NotImplementedError, match="intensity at query times is not available on several trials"):
        nhp.intensity(proc, trials, 0.5)
    with pytest.raises(NotImplementedError, match="forecast is not available on several trials"):
        nhp.forecast(proc, trials, 1.0, nsamples=2)
    with pytest.raises(NotImplementedError, match="LogGaussianCoxProcess baseline is not available on several trials"):
        nhp.loglikelihood(lg, trials, recursive=False)
    with pytest.raises(NotImplementedError, match="several trials are not sharded"):
        nhp.ShardedDataset(proc, trials)
    # one recording is accepted by all of them, as a triple and as a list of one trial
    for data in (one, [one]):
        assert nhp.intensity(proc, data, 0.5).shape == (c["N"],)
        assert nhp.forecast(proc, data, 1.0, nsamples=2).counts.shape == (2, c["N"])
        assert np.isfinite(nhp.loglikelihood(lg, data, recursive=False))
    plain = continuous.DeviceDataset(ctx, one, c["N"], c["dt_max"])
    pn = np.zeros(len(one[0]), dtype=np.int64)
    assert lib.nhp_cont_lgcp_loglik(ctx.h, plain.h, _lib.iptr(pn), _lib.dptr(gx), 3, _lib.dptr(lam), _lib.dptr(lls)) == _lib.OK
    assert np.all(np.isfinite(lls))
    assert nhp.ShardedDataset(proc, one, rank=0, world=1).local.ntrials == 1
