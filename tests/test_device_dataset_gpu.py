"""The device-built continuous dataset (nhp_cont_dataset_create_device) against the host-built one.

The device route must make the SAME dataset: every exported array equal byte for byte, every scalar equal, the same
status and message for bad input, and so the same results, bit for bit, from every evaluation downstream.  Built from
host arrays (build="device") and from torch tensors on the context's device (always the device route).
"""
import time

import numpy as np
import pytest

from helpers import random_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(nhp):
    from nhp_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope="module")
def torch_dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def build(nhp, ctx, data, N, dt_max, how, columns=None, torch_dev=None):
    from nhp_amd.continuous import DeviceDataset
    if how == "tensor":
        import torch
        events, nodes, T = data
        data = (torch.from_numpy(np.ascontiguousarray(events, dtype=np.float64)).to(torch_dev),
                torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.int64)).to(torch_dev), T)
        return DeviceDataset(ctx, data, N, dt_max, columns=columns)
    return DeviceDataset(ctx, data, N, dt_max, columns=columns, build=how)


def assert_same_layout(a, b):
    la, lb = a.layout(), b.layout()
    assert la["scalars"] == lb["scalars"]
    for k, x in la["arrays"].items():
        y = lb["arrays"][k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def check_all_routes(nhp, ctx, torch_dev, data, N, dt_max, columns=None):
    host = build(nhp, ctx, data, N, dt_max, "host", columns)
    for how in ("device", "tensor"):
        assert_same_layout(host, build(nhp, ctx, data, N, dt_max, how, columns, torch_dev))
    return host


def metric(nhp, N, M, kbar, dt_max=1.0):
    return nhp.synthetic.s_metric_data(N, M, kbar=kbar, dt_max=dt_max)


def test_empty_and_single(nhp, ctx, torch_dev):
    check_all_routes(nhp, ctx, torch_dev, (np.zeros(0), np.zeros(0, dtype=np.int64), 1.0), 4, 1.0)
    check_all_routes(nhp, ctx, torch_dev, (np.array([0.5]), np.array([3]), 1.0), 4, 1.0)


def test_zero_times_ties_and_infinite_window(nhp, ctx, torch_dev):
    rng = np.random.default_rng(5)
    M, N = 3000, 6
    nodes = rng.integers(1, N + 1, M)
    check_all_routes(nhp, ctx, torch_dev, (np.zeros(M), nodes, 1.0), N, 1.0)                       # all at t = 0.0
    ties = np.floor(np.sort(rng.uniform(0.0, 100.0, M)) * 2.0) / 2.0                                # heavy ties on a 0.5 grid
    ties[:40] = 0.0
    ds = check_all_routes(nhp, ctx, torch_dev, (ties, nodes, 100.0), N, 1.0)
    assert ds.scalars()["n_zero_time"] >= 40
    check_all_routes(nhp, ctx, torch_dev, (ties, nodes, 100.0), N, 0.5)                             # window = the tie step
    ds = check_all_routes(nhp, ctx, torch_dev, (ties, nodes, 100.0), N, float("inf"))
    assert ds.scalars()["max_window"] == M - 1


@pytest.mark.parametrize("N", [1, 65534, 65535])
def test_node_count_boundaries(nhp, ctx, torch_dev, N):
    # N <= 65534: child slices; N <= 65535: 8-byte records
    times, nodes, T = metric(nhp, N, 40000, 8.0)
    check_all_routes(nhp, ctx, torch_dev, (times, nodes, T), N, 1.0)


@pytest.mark.parametrize("kbar", [8.0, 64.0, 512.0])
def test_mean_windows(nhp, ctx, torch_dev, kbar):
    times, nodes, T = metric(nhp, 64, 60000, kbar)
    check_all_routes(nhp, ctx, torch_dev, (times, nodes, T), 64, 1.0)


def test_time_parts_with_large_items(nhp, ctx, torch_dev):
    # mean window 256 >= 192: four time parts (TP = 4); 8 nodes, 2e5 events: items of ~6000 children (> 4096)
    times, nodes, T = metric(nhp, 8, 200_000, 256.0)
    ds = check_all_routes(nhp, ctx, torch_dev, (times, nodes, T), 8, 1.0)
    assert ds.scalars()["n_items"] == 32 and ds.scalars()["max_item"] > 4096


@pytest.mark.parametrize("columns,kbar", [((8, 40), 8.0), ((3, 11), 512.0), ((0, 1), 64.0)])
def test_column_shards(nhp, ctx, torch_dev, columns, kbar):
    N = 64 if kbar != 512.0 else 16
    times, nodes, T = metric(nhp, N, 50000, kbar)
    check_all_routes(nhp, ctx, torch_dev, (times, nodes, T), N, 1.0, columns=columns)


@pytest.mark.parametrize("env", [{"NHP_SORT": "0"}, {"NHP_SORT": "1"}, {"NHP_XCD": "2"}, {"NHP_CHUNK": "64"},
                                 {"NHP_SORT": "1", "NHP_XCD": "4"}])
def test_environment_switches(nhp, ctx, torch_dev, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    times, nodes, T = metric(nhp, 32, 60000, 64.0)
    check_all_routes(nhp, ctx, torch_dev, (times, nodes, T), 32, 1.0)


def test_metric_dataset(nhp, ctx, torch_dev):
    times, nodes, T = metric(nhp, 1024, 1_000_000, 8.0)
    ds = check_all_routes(nhp, ctx, torch_dev, (times, nodes, T), 1024, 1.0)
    s = ds.scalars()
    assert s["n_slices"] > 0 and len(ds.array("poff")) == 1_000_001 and len(ds.array("ev8")) == 1_000_000


def _error(fn):
    with pytest.raises(Exception) as e:
        fn()
    return type(e.value), str(e.value)


@pytest.mark.parametrize("case", ["unsorted", "negative", "nan", "node0", "nodeN1", "node0_first", "node_and_time"])
def test_error_parity(nhp, ctx, torch_dev, case):
    N = 5
    times = np.linspace(0.0, 10.0, 500)
    nodes = (np.arange(500) % N + 1).astype(np.int64)
    if case == "unsorted":
        times[300] = times[100]
    elif case == "negative":
        times[:3] = -1.0
    elif case == "nan":
        times[250] = np.nan
    elif case == "node0":
        nodes[77] = 0
    elif case == "nodeN1":
        nodes[400] = N + 1
    elif case == "node0_first":
        nodes[0] = 0
    elif case == "node_and_time":          # both fail at one index: the node check comes first
        nodes[120], times[120] = N + 1, np.nan
    data = (times, nodes, 10.0)
    want = _error(lambda: build(nhp, ctx, data, N, 1.0, "host"))
    assert want[1]
    for how in ("device", "tensor"):
        assert _error(lambda: build(nhp, ctx, data, N, 1.0, how, torch_dev=torch_dev)) == want


def _results(nhp, proc, data):
    ll = nhp.loglikelihood(proc, data, recursive=False)
    llg, g = nhp.loglikelihood_gradient(proc, data, recursive=False)
    lam = nhp.total_intensity(proc, data)
    par, pn = nhp.resample_parents(proc, data, seed=11, step=3)
    return (ll, llg, lam, par, pn), g


# The gradient kernels accumulate with float atomics, so a gradient (and the Gibbs statistics behind a chain) varies in
# its last bits from run to run on ONE dataset; those are held to 1e-12, everything else to the bit.
def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(a)))


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_end_to_end_bitwise(nhp, ctx, torch_dev, kind):
    import torch
    from nhp_amd.continuous import DeviceDataset
    cases = [random_case(12, 20000, 2000.0, kind, 1.0, network=True, seed=41, nhp=nhp) for _ in range(3)]
    events, nodes, T = cases[0]["data"]
    N = 12
    host = DeviceDataset(ctx, (events, nodes, T), N, 1.0)
    dev = DeviceDataset(ctx, (events, nodes, T), N, 1.0, build="device")
    tev = torch.from_numpy(np.asarray(events, dtype=np.float64)).to(torch_dev)
    tnd = torch.from_numpy(np.asarray(nodes, dtype=np.int64)).to(torch_dev)
    want, want_g = _results(nhp, cases[0]["proc"], host)
    for got, got_g in (_results(nhp, cases[0]["proc"], dev), _results(nhp, cases[0]["proc"], (tev, tnd, T))):
        for a, b in zip(want, got):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        assert _close(want_g, got_g)
    chains = []
    for c, data in zip(cases, (host, dev, (tev, tnd, T))):
        r = nhp.mcmc_(c["proc"], data, nsteps=3, seed=5)
        chains.append(r.samples)
    for s in chains[1:]:
        assert len(s) == 3 and all(_close(a, b) for a, b in zip(chains[0], s))


def test_tensor_refill_rebuilds(nhp, ctx, torch_dev):
    import torch
    c = random_case(6, 5000, 500.0, "exponential", 1.0, seed=43, nhp=nhp)
    events, nodes, T = c["data"]
    tev = torch.from_numpy(np.asarray(events, dtype=np.float64)).to(torch_dev)
    tnd = torch.from_numpy(np.asarray(nodes, dtype=np.int64)).to(torch_dev)
    a = nhp.loglikelihood(c["proc"], (tev, tnd, T), recursive=False)
    assert nhp.loglikelihood(c["proc"], (tev, tnd, T), recursive=False) == a
    tev.mul_(0.5)                                   # in place: still sorted, shorter gaps -> more pairs
    b = nhp.loglikelihood(c["proc"], (tev, tnd, T), recursive=False)
    want = nhp.loglikelihood(c["proc"], (np.asarray(events) * 0.5, nodes, T), recursive=False)
    assert b != a and b == want


def test_tensor_argument_errors(nhp, ctx, torch_dev):
    import torch
    from nhp_amd.continuous import DeviceDataset
    ev = torch.linspace(0.0, 1.0, 10, dtype=torch.float64, device=torch_dev)
    nd = torch.ones(10, dtype=torch.int64, device=torch_dev)
    with pytest.raises(TypeError):
        DeviceDataset(ctx, (ev.float(), nd, 1.0), 2, 1.0)
    with pytest.raises(TypeError):
        DeviceDataset(ctx, (ev, nd.int(), 1.0), 2, 1.0)
    with pytest.raises(ValueError):
        DeviceDataset(ctx, (ev, nd.cpu(), 1.0), 2, 1.0)
    with pytest.raises(ValueError):
        DeviceDataset(ctx, (ev[::2], nd[::2].contiguous(), 1.0), 2, 1.0)
    with pytest.raises(ValueError):
        DeviceDataset(ctx, (ev, nd, 1.0), 2, 1.0, build="gpu")
    ds = DeviceDataset(ctx, (ev, nd, 1.0), 2, 1.0)
    assert len(ds) == 10 and ds.events is None and ds.build == "device"


def test_device_build_is_faster_at_metric_size(nhp, ctx):
    from nhp_amd.continuous import DeviceDataset
    times, nodes, T = metric(nhp, 1024, 1_000_000, 8.0)
    DeviceDataset(ctx, (times, nodes, T), 1024, 1.0, build="device")        # warm-up (module load, first allocations)

    def med(how):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            ds = DeviceDataset(ctx, (times, nodes, T), 1024, 1.0, build=how)
            ts.append(time.perf_counter() - t0)
            del ds
        return float(np.median(ts))
    host, dev = med("host"), med("device")
    assert dev < 0.5 * host, (dev, host)
