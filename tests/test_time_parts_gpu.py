"""The kernels that walk the item table -- k_windowed, k_windowed_batch, k_grad_windowed, k_comp_events, the sampler kernels,
the cascade walk, k_info_blocks, k_info_hvp -- held to their references on datasets laid out in XCD time parts
(csrc/cont_data.hip: nhp_cont_partition), the layout long windows get by default.  The route comes from the default rule: no
test sets NHP_XCD for the cases below (one leg with NHP_XCD=8 apart), every test clears the route switches first, and every
test asserts from the dataset's own scalars and exported items that it ran on the layout it names: the items equal
tests/slices_ref.time_parts entry for entry (tests/test_time_parts_host.py holds that restatement to the properties of a
partition), n_items and max_item match, all_sole = 0, sl_rows = 0, and in the small cases at least one padding item and one
empty `first` item are there.

Cases (tests/cont_grad_ref.time_part_case; times on the dyadic grid 2⁻¹⁰, 12 ties, pairs at Δ = Δtmax exactly, exact zeros in
W, θ·Δtmax from 0.5 to 40; nodes 1..N-3 carry the bulk, node N-2 one event, node N-1 40 events inside the last quarter of the
event indices -- its first item is empty and still owns the column's constants --, node N none: the node the padding names):
    P4-exp, P4-logit, P4-net   N=9  M=1000 T=4   Δtmax=1   mean window 219: TP = 4, 40 items of which 4 padding
    P2-exp, P2-logit           N=10 M=1000 T=5.2 Δtmax=1   mean window 174, between 160 (not sliced) and 192: TP = 2, 24 items (4)
    P2-inf                     N=10 M=300  T=30  Δtmax=∞   mean window 149.5: TP = 2, 24 items (4); no saturated part
    large                      N=8  M=140 000 T=680 Δtmax=1  2.9·10⁷ pairs, TP = 4, 32 items of about 4375 children: only this
                               layout makes items above 4096 children.  Against the oracle only.
    P4-exp, NHP_XCD=8          TP = 8, one node per run of 8 items, 72 items, no padding

Every check uses the reference and the tolerance its kernel has elsewhere in the suite: cont_grad_ref (ll 1e-11, every
gradient entry inside cr.check's bound, δ = 0: these datasets have neither slices nor a pair list), compensator_exact_ref
(event_intensity, at_events / residuals / total), em_ref and vb_ref (exact=True) through the checks of tests/test_em_gpu.py
and tests/test_cont_vb_gpu.py, information_ref through those of tests/test_information_gpu.py, cascades_ref, and the oracle
for the sampler (integers and bits) and the batch (1e-11).

Largest error/bound seen on an MI355X, per kernel (the float64 host evaluations of the same sums, tests/test_cont_grad_host.py,
test_information_host.py and test_compensator_edges_host.py, reach the same size):
    nhp_cont_loglik             ll relative 2.2e-16 (P4-exp; 1.8e-14 on the large case), λ 0.14 of check_intensity's bound (P4-exp)
    nhp_cont_loglik_batch       relative 8.9e-15 against the oracle (P2-inf); enqueue and fetch: the synchronous bits
    nhp_cont_loglik_grad        0.057 (P2-logit, every group width; P4-exp 0.017 at G = 1), shards 0.014, NHP_XCD=8 0.011;
                                large case 3.3e-14 of max(1, |g|) against the oracle
    nhp_cont_em_stats           6.8e-05 of the 1e-10 bound (S1 of P4-exp); nhp_cont_vb_step 1.8e-04 (a KL piece of P4-exp)
    nhp_cont_information        0.026 (P2-inf; tile_nodes=3 0.018), nhp_cont_hessian_vec 0.019 (P4-exp)
    nhp_cont_compensator        0.20 (residuals of P2-inf; float64 on the host 0.20)
    nhp_cont_resample_parents, nhp_cont_map_parents   integers and bits equal; prob within 2.3e-16
No kernel defect was found on this layout.

Mistakes planted in scratch builds of nhp_cont_partition (the `first` flag only, so no address changes; one build each, this
file run once per build on an MI355X):
    it.first = (s == 0)   padding items become first     33 of 35 red; green: the NHP_XCD=8 leg and the large case, whose
                                                         tables have no padding
    it.first = real       every part becomes first       35 of 35 red
Most of that red is the items comparison, which every test makes.  With that comparison blind to `first` (a scratch plugin
that compared node, kbeg, kend only) the kernels' own outputs showed the mistakes in 20 and 22 tests: every case of the
log-likelihood / batch, gradient, shard, EM / VB and information tests (and, for `real`, the NHP_XCD=8 leg and the large
case: ll off by 0.79 relative), each at its log-likelihood assertion -- ll off by 70 to 160 for the padding (the integral
terms of node N once more per padding item), by thousands for `real`.  The sampler, compensator and most-likely-parents
tests stayed green: those kernels do not read `first`.  With the log-likelihood assertions switched off as well, the gradient
entries, the EM statistics and the information blocks stayed green too (the gradient's constants come from k_grad_init, not
from the first item; the statistics and the blocks have none) and only the VB step's Σ log λ̃ went red: on this layout a wrong `first` is a
wrong log-likelihood and nothing else, in every kernel that returns one -- which is why each of them has its ll held here.
"""
import ctypes as C

import numpy as np
import pytest

import compensator_exact_ref as ce
import cont_grad_ref as cr
import information_ref as ir
import sampler_slices_cases as sampler_cases
import slices_ref as sr
from helpers import rel
from test_cascades_gpu import _map_check
from test_compensator_edges_gpu import hold as hold_compensator
from test_compensator_edges_gpu import run as run_compensator
from test_cont_grad_edges_gpu import REL_LL, ROUTE_ENV, hold, route, two_pass_preconditions  # noqa: F401  (route: a fixture)
from test_cont_vb_gpu import _one_step_against_the_restatement, _with_priors
from test_em_gpu import _check as check_statistics
from test_em_gpu import _want as want_statistics
from test_enqueue_pairs_gpu import batch_ll, device_model, enqueue, sync_ll
from test_information_gpu import call as information
from test_information_gpu import hold as hold_information
from test_information_gpu import test_hessian_vector_product as check_hessian_vector_product
from test_time_parts_host import MAP_CASES, map_reference

pytestmark = pytest.mark.gpu

TP_OF = {name: 4 if name.startswith("P4") else 2 for name in cr.TIME_PART_CASES}
GRAD_THREADS = {"P4-exp": 512, "P4-logit": 512, "P4-net": 512, "P2-exp": 512, "P2-logit": 512, "P2-inf": 256}
"""k_grad_windowed's TH: 512 from 4096 pairs per item on (5485 with 40 items, 7267 and 1869 with 24)."""
assert ROUTE_ENV.count("NHP_XCD") == 1


def same_bits(a, b):
    """Equal bit for bit, a NaN (a pair of nodes without a drawn parent) standing where the other has one."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    m = ~np.isnan(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[m].view(np.uint64), b[m].view(np.uint64))


def exported_items(ds):
    it = ds.array("items")
    return np.stack([it["node"], it["kbeg"], it["kend"], it["first"]], axis=1).astype(np.int64)


def on_time_parts(ds, times, nodes, N, dt_max, TP, columns=None, parts=None, small=True):
    """The dataset is laid out in the TP time parts the rule gives: items entry for entry, the scalars; returns the items."""
    want = sr.time_parts(times, nodes, N, dt_max, columns=columns, parts=parts)
    assert want is not None and want[0] == TP, (want and want[0], TP)
    items, sc = exported_items(ds), ds.scalars()
    assert np.array_equal(items, want[1]), (items.tolist(), want[1].tolist())
    assert sc["n_items"] == len(items) and sc["max_item"] == int((items[:, 2] - items[:, 1]).max())
    assert sc["all_sole"] == 0 and sc["sl_rows"] == 0
    if small and columns is None:
        first = (items[:, 3] & 1) == 1
        empty = items[:, 1] == items[:, 2]
        assert first.sum() == N and (first & empty & (items[:, 0] == N - 2)).sum() == 1     # the late node's empty first item
        assert (~first & empty & (items[:, 0] == N - 1)).sum() >= 1 + (TP - 1 if parts is None else 0)   # padding on the empty node
        assert len(items) > N * TP or parts is not None
    return items


def case_on_time_parts(nhp, case, proc, data=None, **kw):
    """The cached dataset an entry point of the package just used for (proc, data)."""
    data = (case["times"], case["nodes"], case["T"]) if data is None else data
    ds = nhp.device_dataset(proc, data)
    return on_time_parts(ds, data[0], data[1], case["N"], case["dt_max"], TP_OF[case["name"]], **kw)


def prepared(name):
    case, res = cr.prepared(name)
    return dict(case, name=name), res


def fresh_dataset(nhp, case, columns=None, parts=None):
    ctx = nhp.default_context()
    ds = nhp.continuous.DeviceDataset(ctx, (case["times"], case["nodes"], case["T"]), case["N"], case["dt_max"], columns=columns)
    on_time_parts(ds, case["times"], case["nodes"], case["N"], case["dt_max"], parts or TP_OF[case["name"]], columns=columns, parts=parts)
    return ctx, ds


def gradient(nhp, case, P, columns=None, parts=None):
    """tests/test_cont_grad_edges_gpu.gradient on a dataset whose layout has been checked first."""
    from nhp_amd import _lib
    ctx, ds = fresh_dataset(nhp, case, columns=columns, parts=parts)
    model = cr.process_of(nhp, case).device_model(ctx)
    g, ll = np.full(P, np.nan), C.c_double()
    _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, 0, C.byref(ll), _lib.dptr(g), P), ctx.h)
    return ll.value, g, ds.scalars()


# ------------------------------------------------------------------------------------- log-likelihood, λ, batch, enqueue
def variants(case, count=8, seed=71):
    """`count` models of the case's kinds on its data: every parameter moved by up to a tenth, exact zeros kept."""
    rng = np.random.default_rng(seed)
    N = case["N"]
    out = []
    for _ in range(count):
        v = dict(case, lam0=case["lam0"] * rng.uniform(0.9, 1.1, N), W=case["W"] * rng.uniform(0.9, 1.1, (N, N)),
                 theta=case["theta"] * rng.uniform(0.9, 1.1, (N, N)), mu=case["mu"] + rng.normal(0.0, 0.1, (N, N)),
                 tau=case["tau"] * rng.uniform(0.9, 1.1, (N, N)))
        out.append(v)
    return out


@pytest.mark.parametrize("name", cr.TIME_PART_CASES)
def test_loglikelihood_intensity_batch_and_enqueue(nhp, orc, route, name):
    route({})
    case, res = prepared(name)
    ctx, ds = fresh_dataset(nhp, case)
    proc = cr.process_of(nhp, case)
    want = float(res.ll)
    got = nhp.loglikelihood(proc, ds, recursive=False)
    print(f"{name}: ll relative error {abs(got - want) / abs(want):.3g}")
    assert abs(got - want) <= REL_LL * abs(want), (name, got, want)
    lam = ce.event_intensity(cr.model_of(case), case["times"], case["nodes"])
    ratio, bad = ce.check_intensity(nhp.total_intensity(proc, ds), lam)
    print(f"{name}: total_intensity error/bound {ratio:.3g}")
    assert len(bad) == 0, f"{name}: events {bad[:8].ravel().tolist()} outside the bound"
    # the device build makes the same table, padding included, and gives the same bits
    dev = nhp.continuous.DeviceDataset(ctx, (case["times"], case["nodes"], case["T"]), case["N"], case["dt_max"], build="device")
    on_time_parts(dev, case["times"], case["nodes"], case["N"], case["dt_max"], TP_OF[name])
    assert dev.scalars() == ds.scalars() and nhp.loglikelihood(proc, dev, recursive=False) == got
    # one enqueue and fetch of the same model: the synchronous value, bit for bit
    model = device_model(nhp, ctx, proc)
    sync = sync_ll(nhp, ctx, ds, model)
    assert sync == got
    enqueue(nhp, ctx, ds, model, 0)
    assert ctx.fetch(0, 1)[0] == sync
    # eight models in one batch call against the oracle
    vs = variants(case)
    models = [device_model(nhp, ctx, cr.process_of(nhp, v)) for v in vs]
    out = batch_ll(nhp, ctx, ds, models)
    wants = [orc.loglik(cr.oracle_model(orc, v), v["times"], v["nodes"], v["T"], recursive=False) for v in vs]
    worst = max(rel(g, w) for g, w in zip(out, wants))
    print(f"{name}: batch of 8, largest relative error {worst:.3g}")
    assert worst < 1e-11 and len(set(out.tolist())) == 8
    assert rel(orc.loglik(cr.oracle_model(orc, case), case["times"], case["nodes"], case["T"], recursive=False), want) < 1e-11


# ------------------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize("name", cr.TIME_PART_CASES)
def test_gradient_every_entry_in_its_bound(nhp, route, name):
    case, res = prepared(name)
    P = len(res.grad)
    for group in (None, 1, 64):
        route({} if group is None else {"NHP_GROUP": str(group)})
        ll, g, sc = gradient(nhp, case, P)
        two_pass_preconditions(case, sc, group, GRAD_THREADS[name])
        hold(f"{name} G={sc['group']}" + ("" if group else " (the dataset's own)"), ll, g, res, case["N"])
        N = case["N"]
        empty = N - 1                                                   # node N: -T, zeros, -cnt·mask and nothing else
        assert g[empty] == -case["T"] and np.all(g[N + N * empty:N + N * empty + N] == 0.0)


def test_gradient_of_column_shards(nhp, route):
    """P4-exp as [0,4) + [4,9) and the single column [8,9): the empty node, whose shard holds `first` and padding items only."""
    case, whole = prepared("P4-exp")
    N, P = case["N"], len(whole.grad)
    col = np.concatenate([np.arange(N), np.tile(np.repeat(np.arange(N), N), 2)])
    total = np.zeros(P)
    for cols in ((0, 4), (4, 9), (8, 9)):
        _, res = cr.prepared("P4-exp", cols)
        route({})
        ll, g, sc = gradient(nhp, case, P, columns=cols)
        assert sc["n_items"] == {(0, 4): 16, (4, 9): 24, (8, 9): 8}[cols]
        foreign = (col < cols[0]) | (col >= cols[1])
        assert np.all(g[foreign] == 0.0) and not np.any(np.signbit(g[foreign])), f"{cols}: foreign entries must be exactly 0.0"
        hold(f"P4-exp shard {cols}", ll, g, res, N)
        if cols == (8, 9):
            assert np.array_equal(g[~foreign], res.const[~foreign])      # nothing but the constants
        else:
            total += g
    ratio, bad, err, B = cr.check(total, whole)
    assert len(bad) == 0, cr.explain(total, whole, N, bad, err, B)


def test_eight_time_parts_when_asked_for(nhp, route):
    """NHP_XCD=8: one node per run of 8 items, no padding; the partition and the device build accept it."""
    case, res = prepared("P4-exp")
    route({"NHP_XCD": "8"})
    ll, g, sc = gradient(nhp, case, len(res.grad), parts=8)
    assert sc["n_items"] == 72
    hold("P4-exp NHP_XCD=8", ll, g, res, case["N"])
    ctx = nhp.default_context()
    data = (case["times"], case["nodes"], case["T"])
    host = nhp.continuous.DeviceDataset(ctx, data, case["N"], case["dt_max"])
    dev = nhp.continuous.DeviceDataset(ctx, data, case["N"], case["dt_max"], build="device")
    assert np.array_equal(exported_items(host), exported_items(dev)) and host.scalars() == dev.scalars()
    proc = cr.process_of(nhp, case)
    for ds in (host, dev):
        got = nhp.loglikelihood(proc, ds, recursive=False)
        assert abs(got - float(res.ll)) <= REL_LL * abs(float(res.ll))


# ------------------------------------------------------------------------------------------------------------ EM and VB
@pytest.mark.parametrize("name", ["P4-exp", "P4-logit", "P2-inf"])
def test_em_statistics_and_one_vb_step(nhp, route, name):
    route({})
    case, _ = prepared(name)
    proc = _with_priors(cr.process_of(nhp, case))
    data = (case["times"], case["nodes"], case["T"])
    want, pr, _ = want_statistics(proc, data, False)
    got = nhp.expected_statistics(proc, data, recursive=False)
    worst = check_statistics(got, want, f"{name} statistics")
    print(f"{name}: statistics, largest error / bound {worst:.3g}")
    total = got.EM.sum(axis=0) + got.bg
    live = pr.cnt > 0
    assert np.max(np.abs(total - pr.cnt)[live] / pr.cnt[live]) <= 1e-12 * 10
    assert got.bg[case["N"] - 1] == 0.0 and np.all(got.EM[:, case["N"] - 1] == 0.0)      # the empty node
    case_on_time_parts(nhp, case, proc, data)
    _one_step_against_the_restatement(nhp, proc, data, case["kind"], case["dt_max"], False, f"{name} one step")
    case_on_time_parts(nhp, case, proc, data)


# --------------------------------------------------------------------------------------------------------- information
@pytest.mark.parametrize("name", ["P4-exp", "P4-logit", "P4-net", "P2-inf"])
def test_information_blocks_and_hessian_vector_products(nhp, route, name):
    route({})
    case, res = ir.prepared(name)
    case = dict(case, name=name)
    blocks = hold_information(name, information(nhp, case), case, res)
    assert np.all(blocks[case["N"] - 1] == 0.0)                          # node N has no event
    proc = ir.process_of(nhp, case)
    data = (case["times"], case["nodes"], case["T"])
    if name == "P4-exp":
        hold_information(name + " tile_nodes=3", information(nhp, case, tile_nodes=3), case, res)
    check_hessian_vector_product(nhp, name)                              # a random v and one unit vector per parameter kind
    case_on_time_parts(nhp, case, proc, data)


# --------------------------------------------------------------------------------------------------------- compensator
@pytest.mark.parametrize("name", ce.TIME_PART_CASES)
def test_compensator_every_entry_in_its_bound(nhp, route, name):
    route({})
    case, res = ce.prepared(name)
    case = dict(case, name=name)
    proc, data, got = run_compensator(nhp, case)
    assert len(got.at_events) == len(got.residuals) == len(case["times"]) and len(got.total) == case["N"]
    hold_compensator(name, got, (res.at_events, res.residuals, res.total))
    if name == "P2-inf":
        assert np.all(res.ws == 0)                                       # nothing saturates: the D = nullptr path
    order = np.argsort(case["nodes"], kind="stable")
    first = np.concatenate([[True], np.diff(case["nodes"][order]) != 0])
    at = got.at_events[order]
    assert np.array_equal(got.residuals[order], np.where(first, at, at - np.roll(at, 1)))
    case_on_time_parts(nhp, case, proc, data)


# ------------------------------------------------------------------------------------------------------------- parents
@pytest.mark.parametrize("name", cr.TIME_PART_CASES)
def test_resampled_parents_equal_the_oracle(nhp, orc, route, monkeypatch, name):
    route({})
    case, _ = prepared(name)
    ctx, ds = fresh_dataset(nhp, case)
    proc, om = cr.process_of(nhp, case), cr.oracle_model(orc, case)
    t, nodes, N, M = case["times"], case["nodes"], case["N"], len(case["times"])
    assert ds.scalars()["max_window"] + 1 <= 1024                         # NHP_SAMPLER=8 is not sent back to the single-lane kernel
    u = sampler_cases.uniforms(M)
    assert (u == 0.0).sum() >= 1 and (u == np.nextafter(1.0, 0.0)).sum() >= 1
    want_u = orc.resample_parents(om, t, nodes, u, flags=orc.MATH_DET)
    want_s = orc.resample_parents(om, t, nodes, orc.uniform_stream(3, 9, M), flags=orc.MATH_DET)
    assert np.all(want_u[0][u == np.nextafter(1.0, 0.0)] == 0) and (want_u[0] > 0).sum() > M // 10
    for which in ("1", "8", None):
        if which is None:
            monkeypatch.delenv("NHP_SAMPLER", raising=False)
        else:
            monkeypatch.setenv("NHP_SAMPLER", which)
        p, pn, st = nhp.resample_parents(proc, ds, u=u, with_stats=True)
        assert np.array_equal(p, want_u[0]) and np.array_equal(pn, want_u[1]), (name, which, "u")
        assert np.array_equal(st["cnt0"], orc.baseline_node_counts(nodes, pn, N)), (name, which)
        assert np.array_equal(st["Mn"], orc.node_counts(nodes, N)), (name, which)
        assert np.array_equal(st["Mnm"], orc.parent_counts(nodes, pn, N)), (name, which)
        assert st["Mnm"].sum() + st["cnt0"].sum() == M
        if case["kind"] == "exponential":
            assert same_bits(st["Xnm"], orc.duration_mean(t, nodes, p, N)), (name, which)
        p, pn = nhp.resample_parents(proc, ds, seed=3, step=9)
        assert np.array_equal(p, want_s[0]) and np.array_equal(pn, want_s[1]), (name, which, "philox")
    monkeypatch.delenv("NHP_SAMPLER", raising=False)


@pytest.mark.parametrize("name", MAP_CASES)
def test_most_likely_parents(nhp, route, name):
    route({})
    case, ref = map_reference(name)
    case = dict(case, name=name)
    proc = cr.process_of(nhp, case)
    data = (case["times"], case["nodes"], case["T"])
    _map_check(nhp, proc, data, ref, name)
    case_on_time_parts(nhp, case, proc, data)


# ---------------------------------------------------------------------------------------------- items above 4096 children
@pytest.fixture(scope="module")
def large(nhp, orc):
    """The large-item data, a model as tests/test_shapes_gpu.py makes them, and the oracle's values, computed once."""
    t, nodes, T, N, dt_max = cr.large_item_data()
    rng = np.random.default_rng(N + len(t))
    lam0 = rng.uniform(0.5, 1.5, N)
    W = rng.uniform(0.0, 1.0, (N, N)) / N
    th = rng.uniform(1.0, 5.0, (N, N))
    om = orc.ContModel(lam0, W, theta=th, dt_max=dt_max)
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), nhp.ExponentialImpulseResponse(th, 1.0, 1.0, dt_max),
                                               nhp.DenseWeightModel(W))
    u = np.random.default_rng(1).uniform(size=len(t))
    return dict(t=t, nodes=nodes, T=T, N=N, dt_max=dt_max, proc=proc, u=u,
                ll=orc.loglik_windowed(om, t, nodes, T, flags=orc.FAST_INTEGRAL), lam=orc.total_intensity(om, t, nodes),
                grad=orc.loglik_grad(om, t, nodes, T, recursive=False)[1],
                parents=orc.resample_parents(om, t, nodes, u, flags=orc.MATH_DET))


def test_items_above_4096_children(nhp, route, large):
    route({})
    L = large
    ctx = nhp.default_context()
    ds = nhp.continuous.DeviceDataset(ctx, (L["t"], L["nodes"], L["T"]), L["N"], L["dt_max"])
    items = on_time_parts(ds, L["t"], L["nodes"], L["N"], L["dt_max"], 4, small=False)
    sc = ds.scalars()
    assert sc["max_item"] > 4096 and sc["n_items"] == 32 == len(items) and np.all(items[:, 2] - items[:, 1] > 4096)
    assert sc["pairs"] / sc["M"] >= 192
    got = nhp.loglikelihood(L["proc"], ds, recursive=False)
    print(f"large: ll relative error {rel(got, L['ll']):.3g}")
    assert rel(got, L["ll"]) < 1e-11
    lam = nhp.total_intensity(L["proc"], ds)
    e_lam = float(np.max(np.abs(lam - L["lam"]) / lam))
    ll, g = nhp.loglikelihood_gradient(L["proc"], ds, recursive=False)
    e_g = float(np.max(np.abs(g - L["grad"]) / np.maximum(1.0, np.abs(L["grad"]))))
    print(f"large: total_intensity {e_lam:.3g}, gradient {e_g:.3g}")
    assert e_lam < 1e-12 and e_g < 1e-9 and rel(ll, L["ll"]) < 1e-11
    p, pn = nhp.resample_parents(L["proc"], ds, u=L["u"])
    assert np.array_equal(p, L["parents"][0]) and np.array_equal(pn, L["parents"][1])
