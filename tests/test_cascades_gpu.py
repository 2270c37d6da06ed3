"""map_parents / cascades on the GPU (nhp_cont_map_parents, nhp_cont_cascades: csrc/cont_cascades.hip) against the numpy
restatement (tests/cascades_ref.py).

The arg-max is compared EXACTLY: tests/test_cascades_host.py shows that no event of the generated cases has its two largest
weights within 1e-6 relative, every case here asserts the same at 1e-9, and the device weights carry a few ulp.  prob is
held to 1e-11, the bound tests/test_compensator_gpu.py uses for the same sums.  Forest outputs are integers and one
maximum of times: bit-equal."""
import ctypes as C

import numpy as np
import pytest

import cascades_ref as cf
import compensator_ref as cr

pytestmark = pytest.mark.gpu

TOL = 1e-11


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _map_check(nhp, proc, data, ref, what):
    par, pno, prob = nhp.map_parents(proc, data)
    M = len(ref.parents)
    assert par.shape == pno.shape == prob.shape == (M,) and par.dtype == pno.dtype == np.int64
    if M > 1:
        gap = float(ref.gap[1:].min())
        assert gap >= 1e-9, (what, gap)            # no event whose arg-max the rounding of a weight could move
    else:
        gap = 1.0
    np.testing.assert_array_equal(par, ref.parents, err_msg=what)
    np.testing.assert_array_equal(pno, ref.parentnodes, err_msg=what)
    if M == 0:
        return par, pno, prob
    e_prob = float(np.max(np.abs(prob - ref.prob)))
    lam = nhp.total_intensity(proc, data)
    e_w = float(np.max(np.abs(prob * lam - ref.wmax)[1:] / np.maximum(1.0, ref.wmax[1:]))) if M > 1 else 0.0
    print(f"{what}: M={M} baseline share {np.mean(ref.parents == 0):.2f} smallest gap {gap:.1e} "
          f"|prob - ref| {e_prob:.2e} |prob·λ - w_max| {e_w:.2e}")
    assert prob[0] == 1.0 and par[0] == 0 and pno[0] == 0
    assert e_prob <= TOL and e_w <= TOL
    return par, pno, prob


def _same_bits(a, b):
    for x, y in zip(a, b):
        x, y = _np(x), _np(y)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.parametrize("kind", cf.KINDS)
@pytest.mark.parametrize("N,T,dt_max", cf.SHAPES)
def test_map_parity_generated_cases(nhp, kind, N, T, dt_max):
    cs = cf.case(nhp, kind, N, T, dt_max)
    got = _map_check(nhp, cs["proc"], cs["data"], cs["ref"], f"{kind} N={N}")
    # the same bits from a second call, from the device-built dataset and as device tensors
    import torch
    ctx = nhp.default_context()
    _same_bits(got, nhp.map_parents(cs["proc"], cs["data"]))
    _same_bits(got, nhp.map_parents(cs["proc"], nhp.DeviceDataset(ctx, cs["data"], N, dt_max, build="device")))
    dev = torch.device("cuda", ctx.device)
    tens = (torch.as_tensor(cs["times"]).to(dev), torch.as_tensor(cs["nodes"]).to(dev), T)
    out = nhp.map_parents(cs["proc"], tens, device=True)
    assert all(o.is_cuda for o in out) and out[0].dtype == out[1].dtype == torch.int64 and out[2].dtype == torch.float64
    _same_bits(got, out)


def test_map_parity_without_the_pair_cache(nhp, monkeypatch):
    """Logit-normal impulses with the pair cache switched off (NHP_PLQ=0, read on every call): the whole pdf per pair, the
    kernel variant a dataset without pair offsets takes -- the same bits as through the cache."""
    N, T, dt = cf.SHAPES[1]
    cs = cf.case(nhp, "logitnormal", N, T, dt)
    cached = nhp.map_parents(cs["proc"], cs["data"])
    monkeypatch.setenv("NHP_PLQ", "0")
    _same_bits(cached, _map_check(nhp, cs["proc"], cs["data"], cs["ref"], "logitnormal N=7 no pair cache"))


def test_map_parity_unbounded_window(nhp):
    """Δtmax = ∞: every earlier event is a category (windows up to ~800 long: 100 chunks of 8 per child)."""
    cs = cf.case(nhp, "exponential", 3, 450.0, np.inf)
    assert 600 <= len(cs["times"]) <= 1000
    _map_check(nhp, cs["proc"], cs["data"], cs["ref"], "exponential N=3 dt_max=inf")


def test_map_parity_long_windows(nhp):
    """N = 2, Δtmax = ∞, M = 3000: windows far beyond anything a lane could keep."""
    proc = cf.make_process(nhp, "exponential", 2, np.inf)
    times, nodes, _ = nhp.rand(proc, 3000.0, seed=1)
    assert len(times) >= 3000
    times, nodes = times[:3000], nodes[:3000]
    ref = cf.map_parents_ref(cr.Model.of(proc), times, nodes)
    _map_check(nhp, proc, (times, nodes, float(times[-1])), ref, "exponential N=2 dt_max=inf M=3000")


@pytest.mark.parametrize("kind", cf.KINDS)
def test_map_parity_masked_column(nhp, kind):
    """A network mask whose column 2 is zero: the events of node 3 have no parent but the baseline."""
    N, T, dt = cf.SHAPES[0]
    A = (np.random.default_rng(8).uniform(size=(N, N)) < 0.6).astype(np.float64)
    A[:, 2] = 0.0
    A[0, 0] = A[1, 0] = 1.0
    cs = cf.case(nhp, kind, N, T, dt, A=A)
    par, _, prob = _map_check(nhp, cs["proc"], cs["data"], cs["ref"], f"{kind} masked")
    on3 = cs["nodes"] == 3
    assert on3.sum() > 100 and np.all(par[on3] == 0) and np.all(prob[on3] == 1.0)


@pytest.mark.parametrize("kind", cf.KINDS)
def test_map_parity_lgcp_baseline(nhp, kind):
    N, T, dt = cf.SHAPES[1]
    cs = cf.case(nhp, kind, N, T, dt, lgcp_T=T)
    _map_check(nhp, cs["proc"], cs["data"], cs["ref"], f"{kind} lgcp")


def test_map_parity_node_without_events(nhp):
    N, T, dt = cf.SHAPES[1]
    cs = cf.case(nhp, "logitnormal", N, T, dt)
    nodes = np.where(cs["nodes"] == 4, 5, cs["nodes"])
    ref = cf.map_parents_ref(cs["model"], cs["times"], nodes)
    _map_check(nhp, cs["proc"], (cs["times"], nodes, T), ref, "node without events")


@pytest.mark.parametrize("M", [0, 1])
def test_map_parents_empty_and_single(nhp, M):
    proc = cf.make_process(nhp, "exponential", 3, 1.0)
    times, nodes = np.array([0.7])[:M], np.array([2], np.int64)[:M]
    ref = cf.map_parents_ref(cr.Model.of(proc), times, nodes)
    par, pno, prob = _map_check(nhp, proc, (times, nodes, 1.0), ref, f"M={M}")
    assert len(par) == M and (M == 0 or (par[0], pno[0], prob[0]) == (0, 0, 1.0))


@pytest.mark.parametrize("kind", cf.KINDS)
def test_map_parity_many_items(nhp, kind):
    """N = 64, M = 20000: every node's children are cut into several items (workgroups)."""
    N, M = 64, 20000
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
    proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
    ds = nhp.device_dataset(proc, (times, nodes, T))
    assert ds.scalars()["n_items"] > N
    ref = cf.map_parents_ref(cr.Model.of(proc), times, nodes)
    _map_check(nhp, proc, (times, nodes, T), ref, f"{kind} N=64 M=20000")


def test_exact_ties(nhp):
    """W·θ = 0.5·2 = 1 = λ0[0]: at d = 0 (the dataset's window keeps a simultaneous earlier event) the parent's weight
    W·θ·e^{-θ·0} equals the baseline exactly, and the parent must win.  Events 1 and 2 (node 1, same time) give event 3 two
    bit-equal parent weights: the later index must win."""
    N = 2
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.array([1.0, 0.015625])),
                                               nhp.ExponentialImpulseResponse(np.full((N, N), 2.0), 1.0, 1.0, 4.0),
                                               nhp.DenseWeightModel(np.full((N, N), 0.5)))
    times, nodes = np.array([1.0, 1.0, 1.5]), np.array([1, 1, 2], np.int64)
    ref = cf.map_parents_ref(cr.Model.of(proc), times, nodes)
    assert ref.gap[1] == 0.0 and ref.gap[2] == 0.0                      # both are exact ties in the restatement too
    par, pno, prob = nhp.map_parents(proc, (times, nodes, 2.0))
    assert list(par) == [0, 1, 2] and list(pno) == [0, 1, 1]
    np.testing.assert_array_equal(par, ref.parents)
    assert prob[0] == 1.0 and prob[1] == 0.5
    w = np.exp(-1.0)                                                    # 0.5·2·e^{-2·0.5}
    assert abs(prob[2] - w / (2.0 * w + 0.015625)) <= TOL


# ---- forests ----------------------------------------------------------------------------------------------------------
def _forest_check(got, want, what):
    for name, field in (("root", "root"), ("generation", "generation"), ("descendants", "descendants"),
                        ("cascade_root", "cascade_root"), ("cascade_size", "cascade_size"), ("cascade_depth", "cascade_depth"),
                        ("cascade_end", "cascade_end"), ("immigrants", "immigrants"), ("offspring", "offspring"), ("reach", "reach")):
        g, w = _np(getattr(got, name)), getattr(want, field)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")
    assert int(_np(got.reach).sum()) == len(want.root)


def _forest_case(nhp, par, N, what, **kw):
    M = len(par)
    times, nodes = cf.forest_data(M, N)
    proc = cf.make_process(nhp, "exponential", N, 1.0)
    want = cf.forest_ref(_np(par), times, nodes, N)
    got = nhp.cascades(proc, (times, nodes, max(M, 1) * 0.5), parents=par, **kw)
    _forest_check(got, want, what)
    depth = int(want.generation.max()) if M else 0
    print(f"{what}: M={M} cascades {len(want.cascade_root)} depth {depth} rounds {got.rounds}")
    assert got.rounds <= int(np.ceil(np.log2(depth + 1))) + 1
    return got


@pytest.mark.parametrize("M", [0, 1, 777])
def test_forest_all_immigrants(nhp, M):
    got = _forest_case(nhp, np.zeros(M, np.int64), 3, "all immigrants")
    assert got.rounds == 0 and "Cascades(" in repr(got)


@pytest.mark.parametrize("M", [5000, 100000])
def test_forest_chain(nhp, M):
    got = _forest_case(nhp, np.arange(M, dtype=np.int64), 4, "chain")
    assert got.rounds <= int(np.ceil(np.log2(M))) + 1 and int(got.cascade_depth[0]) == M - 1


def test_forest_star(nhp):
    M = 100000
    _forest_case(nhp, np.r_[0, np.ones(M - 1, np.int64)], 4, "star")


@pytest.mark.parametrize("N", [5, 64])
def test_forest_random(nhp, N):
    _forest_case(nhp, cf.random_forest(20000, seed=N), N, f"random forest N={N}")


def test_forest_random_few_roots_device_route(nhp):
    """Deep trees (1 % immigrants) with the parents and the outputs on the device."""
    import torch
    par = cf.random_forest(20000, seed=2, p_immigrant=0.01)
    dev = torch.device("cuda", nhp.default_context().device)
    got = _forest_case(nhp, torch.as_tensor(par).to(dev), 5, "random forest, 1 % immigrants", device=True)
    assert all(getattr(got, f).is_cuda for f in nhp.Cascades.FIELDS)


# ---- routes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cf.KINDS)
def test_route_map_and_sample(nhp, kind):
    N, T, dt = cf.SHAPES[0]
    cs = cf.case(nhp, kind, N, T, dt)
    want = cf.forest_ref(cs["ref"].parents, cs["times"], cs["nodes"], N)
    got = nhp.cascades(cs["proc"], cs["data"])                           # parents="map"
    np.testing.assert_array_equal(got.parents, cs["ref"].parents)
    _forest_check(got, want, f"{kind} map")
    drawn = nhp.resample_parents(cs["proc"], cs["data"], seed=5)[0]
    got_s = nhp.cascades(cs["proc"], cs["data"], parents="sample", seed=5)
    np.testing.assert_array_equal(got_s.parents, drawn)
    _forest_check(got_s, cf.forest_ref(drawn, cs["times"], cs["nodes"], N), f"{kind} sample")
    assert not np.array_equal(drawn, cs["ref"].parents)
    # two calls, and the host-built against the device-built dataset: the same bits
    ctx = nhp.default_context()
    again = nhp.cascades(cs["proc"], cs["data"])
    built = nhp.cascades(cs["proc"], nhp.DeviceDataset(ctx, cs["data"], N, dt, build="device"))
    for other in (again, built):
        _same_bits([getattr(got, f) for f in nhp.Cascades.FIELDS], [getattr(other, f) for f in nhp.Cascades.FIELDS])


def test_route_simulated_on_the_device(nhp):
    """rand(device=True, return_parents=True) -> cascades(parents=tensor, device=True): the true cascades of simulated data,
    device tensors throughout, equal to the restatement on the downloaded arrays."""
    import torch
    N, T, dt = cf.SHAPES[0]
    proc = cf.make_process(nhp, "exponential", N, dt)
    t, n, _, par = nhp.rand(proc, T, seed=3, device=True, return_parents=True)
    assert par.is_cuda and 800 <= par.numel() <= 2500
    got = nhp.cascades(proc, (t, n, T), parents=par, device=True)
    assert all(getattr(got, f).is_cuda for f in nhp.Cascades.FIELDS) and got.cascade_end.dtype == torch.float64
    want = cf.forest_ref(par.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy(), N)
    _forest_check(got, want, "device-simulated")
    assert int(want.generation.max()) >= 3
    # the immigrants of a simulated path are its baseline events: about λ0·T per node
    assert abs(int(got.immigrants.sum()) - proc.baseline.λ.sum() * T) < 6.0 * np.sqrt(proc.baseline.λ.sum() * T)


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_bad_parent_vectors_are_refused_and_write_nothing(nhp):
    import torch
    from nhp_amd import _lib
    M, N = 3000, 4
    times, nodes = cf.forest_data(M, N)
    proc = cf.make_process(nhp, "exponential", N, 1.0)
    data = (times, nodes, M * 0.5)
    good = cf.random_forest(M, seed=4)
    ctx = nhp.default_context()
    ds = nhp.device_dataset(proc, data, ctx)
    dev = torch.device("cuda", ctx.device)
    SENT = -7
    for k, v in ((1500, 1501), (0, 1), (1499, -1), (2999, M + 1), (10, 12)):
        bad = good.copy()
        bad[k] = v
        with pytest.raises(ValueError, match="must be 0 or the index of an earlier event"):
            nhp.cascades(proc, data, parents=bad)
        with pytest.raises(nhp.DomainError):
            nhp.cascades(proc, data, parents=torch.as_tensor(bad).to(dev), device=True)
        # straight through the C entry point with sentinel-filled device outputs: refused, nothing written
        outs = [torch.full((n,), SENT, dtype=torch.float64 if j == 6 else torch.int64, device=dev)
                for j, n in enumerate((M, M, M, M, M, M, M, N, N, N * N))]
        par = torch.as_tensor(bad).to(dev)
        torch.cuda.synchronize()
        ncasc, rounds = C.c_int64(SENT), C.c_int32(SENT)
        ptrs = [o.data_ptr() for o in outs]
        rc = _lib.lib().nhp_cont_cascades(ctx.h, ds.h, par.data_ptr(), 1, 1, *ptrs[:7], C.byref(ncasc), *ptrs[7:], C.byref(rounds))
        assert rc == _lib.EDOMAIN
        assert all(bool((o == SENT).all()) for o in outs) and ncasc.value == SENT and rounds.value == SENT
        # the context stays usable
        _forest_check(nhp.cascades(proc, data, parents=good), cf.forest_ref(good, times, nodes, N), "after a refusal")


def test_cascade_arrays_come_together(nhp):
    from nhp_amd import _lib
    M, N = 100, 3
    times, nodes = cf.forest_data(M, N)
    proc = cf.make_process(nhp, "exponential", N, 1.0)
    ctx = nhp.default_context()
    ds = nhp.device_dataset(proc, (times, nodes, M * 0.5), ctx)
    par, root, croot = cf.random_forest(M, seed=1), np.empty(M, np.int64), np.empty(M, np.int64)
    ncasc = C.c_int64()
    fn = _lib.lib().nhp_cont_cascades
    assert fn(ctx.h, ds.h, par.ctypes.data, 0, 0, root.ctypes.data, None, None, croot.ctypes.data, None, None, None, C.byref(ncasc),
              None, None, None, None) == _lib.EINVAL
    # per-event outputs alone: no cascade array is needed
    assert fn(ctx.h, ds.h, par.ctypes.data, 0, 0, root.ctypes.data, None, None, None, None, None, None, C.byref(ncasc),
              None, None, None, None) == _lib.OK
    want = cf.forest_ref(par, times, nodes, N)
    np.testing.assert_array_equal(root, want.root)
    assert ncasc.value == len(want.cascade_root)
    assert _lib.lib().nhp_cont_map_parents(ctx.h, ds.h, proc.device_model(ctx).h, 0, None, None, None) == _lib.EINVAL
