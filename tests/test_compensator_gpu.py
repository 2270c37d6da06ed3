"""compensator(process, data) / time_rescaling_test on the GPU (nhp_cont_compensator, csrc/cont_compensator.hip).

Parity with the numpy restatement of the definition (tests/compensator_ref.py) at 1e-11 -- the tolerance the likelihood
kernels are held to against the oracle -- determinism, the definition checked end to end by quadrature of
the library's own intensity, time rescaling on host- and device-simulated data, and the metric size."""
import numpy as np
import pytest

import compensator_ref as cr
from helpers import random_case

pytestmark = pytest.mark.gpu

TOL = 1e-11


def _check(got, want, what=""):
    """|got - want| <= TOL·max(1, want) for at_events and total, TOL·max(1, at_events) for the residuals; returns the largest
    ratio of an error to its bound."""
    at, res, total = want
    worst = 0.0
    for name, g, w, scale in (("at_events", got.at_events, at, at), ("residuals", got.residuals, res, at), ("total", got.total, total, total)):
        g = np.asarray(g)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if len(w) == 0:
            continue
        ratio = float(np.max(np.abs(g - w) / (TOL * np.maximum(1.0, scale))))
        print(f"{what} {name}: largest error / bound = {ratio:.3e}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, name, ratio)
    return worst


def _same(a, b):
    for x, y in zip(a, b):
        x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        assert np.array_equal(x, y)


CASES = [("exponential", 0.5, False, False), ("exponential", 1.0, False, False), ("exponential", 2.0, False, False),
         ("logitnormal", 0.5, False, False), ("logitnormal", 1.0, False, False), ("logitnormal", 2.0, False, False),
         ("exponential", np.inf, False, False),
         ("exponential", 1.0, True, False), ("logitnormal", 1.0, True, False),
         ("exponential", 1.0, False, True), ("logitnormal", 1.0, False, True)]


@pytest.mark.parametrize("kind,dt_max,network,lgcp", CASES)
def test_parity_with_the_restatement(nhp, kind, dt_max, network, lgcp):
    case = random_case(6, 1500, 150.0, kind, dt_max, network=network, lgcp=lgcp, seed=11, nhp=nhp)
    want = cr.compensator(cr.Model.of(case["proc"]), case["times"], case["nodes"], case["T"])
    got = nhp.compensator(case["proc"], case["data"])
    _check(got, want, f"{kind} dt_max={dt_max} network={network} lgcp={lgcp}")
    # the same bits from a second call, from the device-built dataset and from device tensors
    import torch
    _same(got, nhp.compensator(case["proc"], case["data"]))
    ctx = nhp.default_context()
    _same(got, nhp.compensator(case["proc"], nhp.DeviceDataset(ctx, case["data"], 6, dt_max, build="device")))
    dev = torch.device("cuda", ctx.device)
    tens = (torch.as_tensor(case["times"]).to(dev), torch.as_tensor(case["nodes"]).to(dev), case["T"])
    out = nhp.compensator(case["proc"], tens, device=True)
    assert all(o.is_cuda and o.dtype == torch.float64 for o in out)
    _same(got, out)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_parity_across_chunks_and_groups(nhp, kind):
    """20000 events: 157 chunks of 128 events in 3 groups of 64 chunks, so every level of the prefix is in use (the
    restatement in its O(window + N) form, which tests/test_compensator_host.py ties to the O(M²) one)."""
    case = random_case(5, 20000, 2500.0, kind, 1.0, seed=12, nhp=nhp)
    model = cr.Model.of(case["proc"])
    at = cr.at_events_slice(model, case["times"], case["nodes"], 0, 20000)
    want = (at, cr._residuals(at, case["nodes"] - 1, 5), cr.total_closed_form(model, case["times"], case["nodes"], case["T"]))
    _check(nhp.compensator(case["proc"], case["data"]), want, f"{kind} M=20000")


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_ties_and_a_node_without_events(nhp, kind):
    case = random_case(7, 1500, 150.0, kind, 1.0, seed=13, nhp=nhp)
    times = np.round(case["times"])                         # about ten events on each distinct time, t = 0 and t = T among them
    nodes = np.where(case["nodes"] == 4, 5, case["nodes"])  # node 4 has no events
    assert len(np.unique(times)) < len(times) / 3 and not np.any(nodes == 4)
    want = cr.compensator(cr.Model.of(case["proc"]), times, nodes, case["T"])
    got = nhp.compensator(case["proc"], (times, nodes, case["T"]))
    _check(got, want, f"{kind} ties")
    test = nhp.time_rescaling_test(case["proc"], (times, nodes, case["T"]))
    assert np.isnan(test.node_statistic[3]) and np.isnan(test.node_pvalue[3]) and test.counts[3] == 0
    assert np.all(np.isfinite(np.delete(test.node_pvalue, 3)))


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("M", [0, 1])
def test_no_event_and_one_event(nhp, kind, M):
    case = random_case(4, 10, 20.0, kind, 1.0, seed=14, nhp=nhp)
    data = (case["times"][:M], case["nodes"][:M], case["T"])
    want = cr.compensator(cr.Model.of(case["proc"]), *data)
    got = nhp.compensator(case["proc"], data)
    _check(got, want, f"{kind} M={M}")
    assert len(got.at_events) == M and len(got.total) == 4


def test_column_shard_is_refused(nhp):
    case = random_case(4, 200, 50.0, "exponential", 1.0, seed=15, nhp=nhp)
    ctx = nhp.default_context()
    with pytest.raises(NotImplementedError, match="column shard"):
        nhp.compensator(case["proc"], nhp.DeviceDataset(ctx, case["data"], 4, 1.0, columns=(0, 2)))
    with pytest.raises(NotImplementedError, match="column shard"):
        nhp.compensator(case["proc"], nhp.ShardedDataset(case["proc"], case["data"], ctx=ctx, rank=0, world=2))


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_total_is_the_integral_of_the_library_intensity(nhp, kind):
    """Independent of the restatement: 40-point Gauss-Legendre panels (split at every t_i and t_i + Δtmax; 32 sub-panels for
    the logit-normal pdf, steep at both ends of its window) of the batched intensity(process, data, times)."""
    case = random_case(3, 90, 30.0, kind, 1.0, seed=5, nhp=nhp)
    t, T = case["times"], case["T"]
    b = np.concatenate([[0.0, T], t, t + 1.0])
    want = cr.gauss_legendre_total(lambda q: nhp.intensity(case["proc"], case["data"], q), b[b <= T], 3,
                                   sub=1 if kind == "exponential" else 32)
    got = nhp.compensator(case["proc"], case["data"]).total
    err = float(np.max(np.abs(got - want) / want))
    print(f"{kind}: total against the quadrature of intensity(): max rel err {err:.3e}")
    assert err <= 1e-11


def _rescaling_case(nhp, s, kind, zero_weights=False):
    N = 4
    r = np.random.default_rng(s)
    lam0 = r.uniform(.3, .8, N)
    W = r.uniform(0, .5, (N, N)) / 1.5
    if kind == "exponential":
        imp = nhp.ExponentialImpulseResponse(3 * r.uniform(1, 5, (N, N)) + 6, 1.0, 1.0, 1.0)
    else:
        mu = r.normal(0, 1, (N, N))
        imp = nhp.LogitNormalImpulseResponse(mu, r.uniform(.5, 2, (N, N)), 1.0)
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), imp, nhp.DenseWeightModel(W))
    data = nhp.rand(proc, 400.0, seed=s + 10)
    if zero_weights:
        proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), imp, nhp.DenseWeightModel(np.zeros((N, N))))
    return proc, data


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_time_rescaling_on_host_simulated_data(nhp, s, kind):
    """Under the generating model the residuals are Exp(1) (pooled KS p: 0.585 / 0.179 / 0.459 exponential, 0.716 / 0.791 /
    0.275 logit-normal with the restatement); with W = 0 they are not (p < 1e-190)."""
    proc, data = _rescaling_case(nhp, s, kind)
    assert 2028 <= len(data[0]) <= 2570
    comp = nhp.compensator(proc, data)
    test = nhp.time_rescaling_test(proc, data, residuals=comp.residuals)
    d, p = cr.ks_exp1(comp.residuals)
    print(f"s={s} {kind}: M={len(data[0])} pooled KS D={test.statistic:.5f} p={test.pvalue:.4f}; node p={np.round(test.node_pvalue, 3)}")
    assert test.statistic == pytest.approx(d, rel=1e-12) and test.pvalue == pytest.approx(p, rel=1e-9)
    assert test.pvalue > 0.05
    counts = np.bincount(data[1] - 1, minlength=4)
    z = (comp.total - counts) / np.sqrt(comp.total)          # N(T) - Λ(T) is a martingale with variance E Λ(T)
    print(f"   counts - total in sigmas: {np.round(z, 2)}")
    assert np.all(np.abs(z) <= 4.0)
    assert np.array_equal(test.counts, counts)
    flat, _ = _rescaling_case(nhp, s, kind, zero_weights=True)
    p0 = nhp.time_rescaling_test(flat, data).pvalue
    print(f"   W = 0: p={p0:.3e}")
    assert p0 < 1e-50


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_device_simulated_data_end_to_end(nhp, kind):
    """rand(device=True) -> compensator(device=True) -> time_rescaling_test with no host copy of the events.  N = 64, about
    1e5 events, seed 7.  Exponential delays are not cut at Δtmax by rand while the intensity cuts them, so θ·Δtmax >= 12 keeps
    the share e^{-θΔtmax} of children outside the window below what 1e5 residuals resolve; the logit-normal kind has no such tail.
    Observed on the MI355X (the first and only seed tried): exponential 100152 events, pooled D = 0.00301, p = 0.324;
    logit-normal 100094 events, D = 0.00186, p = 0.877."""
    import torch
    N, T = 64, 2000.0
    r = np.random.default_rng(21)
    lam0 = r.uniform(.3, .8, N)
    W = r.uniform(0, 1, (N, N)) * 0.6 / N
    if kind == "exponential":
        imp = nhp.ExponentialImpulseResponse(r.uniform(12, 20, (N, N)), 1.0, 1.0, 1.0)
    else:
        imp = nhp.LogitNormalImpulseResponse(r.normal(0, 1, (N, N)), r.uniform(.5, 2, (N, N)), 1.0)
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), imp, nhp.DenseWeightModel(W))
    data = nhp.rand(proc, T, seed=7, device=True)
    assert data[0].is_cuda and 80_000 <= len(data[0]) <= 125_000
    comp = nhp.compensator(proc, data, device=True)
    assert all(o.is_cuda and o.dtype == torch.float64 for o in comp)
    test = nhp.time_rescaling_test(proc, data, residuals=comp.residuals)
    counts = torch.bincount(data[1] - 1, minlength=N).cpu().numpy()
    z = (comp.total.cpu().numpy() - counts) / np.sqrt(comp.total.cpu().numpy())
    print(f"{kind}: M={len(data[0])} pooled KS D={test.statistic:.5f} p={test.pvalue:.4f}; smallest node p={np.nanmin(test.node_pvalue):.4f}; "
          f"largest |counts - total| in sigmas {np.max(np.abs(z)):.2f}")
    assert test.pvalue > 1e-3
    # the device route and the host route of the test agree
    host = nhp.time_rescaling_test(proc, (data[0].cpu().numpy(), data[1].cpu().numpy(), T), residuals=comp.residuals.cpu().numpy())
    assert host.statistic == pytest.approx(test.statistic, rel=1e-12)
    np.testing.assert_allclose(host.node_statistic, test.node_statistic, rtol=1e-12)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_metric_size(nhp, kind):
    N, M = 1024, 1_000_000
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
    proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
    got = nhp.compensator(proc, (times, nodes, T))
    model = cr.Model.of(proc)
    want = cr.total_closed_form(model, times, nodes, T)
    err = float(np.max(np.abs(got.total - want) / want))
    print(f"{kind}: total, max rel err {err:.3e}")
    assert err <= 1e-11
    worst = 0.0
    for k0 in (0, 499_500, 999_000):
        at = cr.at_events_slice(model, times, nodes, k0, k0 + 1000)
        ratio = float(np.max(np.abs(got.at_events[k0:k0 + 1000] - at) / (TOL * np.maximum(1.0, at))))
        worst = max(worst, ratio)
    print(f"{kind}: at_events on three slices, largest error / bound = {worst:.3e}")
    assert worst <= 1.0
    # residuals: differences of at_events inside a node, whatever the slice
    order = np.argsort(nodes, kind="stable")
    first = np.concatenate([[True], np.diff(nodes[order]) != 0])
    res = np.where(first, got.at_events[order], got.at_events[order] - np.roll(got.at_events[order], 1))
    assert np.array_equal(got.residuals[order], res)
