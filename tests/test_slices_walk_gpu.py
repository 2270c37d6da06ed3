"""The child-slice kernels on datasets that ARE sliced, with items that end at every edge of the rounds in which their slices
are dealt to the waves of a workgroup (csrc/nhp_internal.h: nhp_slice_of, snake order; csrc/cont_slices.hip: k_windowed_slices
phase A, k_slices_batch, k_windowed_slices_ln).

Data: N = 3, Δtmax = 1, NHP_CHUNK = 4096 (one item per node), nodes assigned by hand: node 1 has 64·(k-1) + 5 children (k slices,
the last with 5 lanes), node 2 exactly 64·k (k full slices), node 3 none.  For a workgroup of NW = BLOCK/64 waves k runs over
{1, NW-1, NW, NW+1, 2·NW, 2·NW+1, 3·NW+1}: fewer slices than waves, a full round, one more, two rounds, one into the third (the
second forward round) and one into the fourth.  Uniform times at 8 events per Δtmax, a few ties, one burst.  The largest case
(NW = 16, k = 49) has 6213 events.  (The gradient cases: 3 events per Δtmax and a burst of 40 -- building the parent slices
sorts each parent node's pairs in one lane, quadratic in their number.)  Every test first asserts from the dataset's scalars and its exported slice table that the
dataset kept its slices, k per item: a dataset that fell back to the pair list fails there.

Bounds: the oracle at the suite's 1e-11; the NHP_SLICES=0 route (8-byte pair list) at 1e-12 as test_cont_loglik_gpu holds it;
the gradient inside tests/cont_grad_ref.py's per-entry bound with the records' delay step, as test_cont_grad_edges_gpu; the batch
against the single evaluations at 1e-11 relative, as test_enqueue_lanes_gpu; repeated and enqueued evaluations to the bit."""
import copy
import ctypes as C

import numpy as np
import pytest

import cont_grad_ref as cr
from helpers import random_case, rel

pytestmark = pytest.mark.gpu

TOL = 1e-11
ROUTE_ENV = ("NHP_CHUNK", "NHP_SLICES", "NHP_SLICES_CFG", "NHP_SLICES_LN", "NHP_SLICES_LN_CFG", "NHP_SETS_CFG", "NHP_BATCH_SLICES",
             "NHP_GRAD_SLICES", "NHP_PLIST", "NHP_EV8", "NHP_GROUP", "NHP_XCD", "NHP_SORT")
BLOCKS = (64, 128, 256, 512, 1024)                   # launch_slices builds every one of them with C = 2, 4, 8


def edges(nw):
    return sorted({k for k in (1, nw - 1, nw, nw + 1, 2 * nw, 2 * nw + 1, 3 * nw + 1) if k >= 1})


ALL_K = sorted({k for b in BLOCKS for k in edges(b // 64)})
assert ALL_K == [1, 2, 3, 4, 5, 7, 8, 9, 13, 15, 16, 17, 25, 32, 33, 49]


def walk_data(k, rate=8.0, burst=120):
    """(times, nodes, T): node 1 with 64(k-1)+5 events, node 2 with 64k, node 3 with none, shuffled in time; `rate` events per
    Δtmax and a burst of up to `burst` events inside 0.7·Δtmax."""
    n1, n2 = 64 * (k - 1) + 5, 64 * k
    M = n1 + n2
    rng = np.random.default_rng(1000 + k)
    T = M / rate
    t = np.sort(rng.uniform(0.0, T, M))
    nt = min(40, M // 4)
    a = M // 6
    t[a:a + nt:2] = t[a + 1:a + nt + 1:2]                              # ties: parents at Δt = 0
    nb = min(burst, M // 4)
    b = M // 2
    t[b:b + nb] = np.sort(rng.uniform(t[b], t[b] + 0.7, nb))           # a burst: windows of up to ~nb parents
    t = np.sort(t)
    nodes = np.r_[np.full(n1, 1), np.full(n2, 2)].astype(np.int64)
    rng.shuffle(nodes)
    return t, nodes, float(T)


@pytest.fixture
def route(monkeypatch, nhp):
    def use(env):
        for key in ROUTE_ENV:
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
    yield use
    for key in ROUTE_ENV:
        monkeypatch.delenv(key, raising=False)
    nhp.invalidate_device_datasets()


def sliced_dataset(nhp, route, data, k):
    """The dataset with one item per node; asserts the intended slicing."""
    route({"NHP_CHUNK": "4096"})
    ctx = nhp.default_context()
    ds = nhp.continuous.DeviceDataset(ctx, data, 3, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["n_slices"] == 2 * k and sc["all_sole"] == 1, sc
    assert sc["max_item"] == 64 * k and sc["sl_rows"] * 64 <= 2 * sc["pairs"] + 4096
    assert list(ds.array("sl_item0")) == [0, k, 2 * k, 2 * k]
    items = ds.array("items")
    assert list(items["node"]) == [0, 1, 2] and list(items["kend"] - items["kbeg"]) == [64 * (k - 1) + 5, 64 * k, 0]
    return ctx, ds


def unsliced_dataset(nhp, route, data):
    route({"NHP_CHUNK": "4096", "NHP_SLICES": "0"})
    ctx = nhp.default_context()
    ds = nhp.continuous.DeviceDataset(ctx, data, 3, 1.0)
    assert ds.scalars()["sl_rows"] == 0
    return ds


def sync_ll(ctx, ds, model):
    from nhp_amd import _lib
    ll = C.c_double()
    _lib.check(_lib.lib().nhp_cont_loglik(ctx.h, ds.h, model.h, 0, C.byref(ll)), ctx.h)
    return ll.value


def model_case(nhp, orc, kind, network, lgcp, data):
    c = random_case(3, 8, data[2], kind, 1.0, network=network, lgcp=lgcp, seed=21, nhp=nhp, orc=orc)
    want = orc.loglik(c["om"], data[0], data[1], data[2], recursive=False)
    return c["proc"], want


@pytest.mark.parametrize("k", ALL_K)
def test_every_round_edge(nhp, orc, route, monkeypatch, k):
    from nhp_amd import _lib
    data = walk_data(k)
    blocks = [b for b in BLOCKS if k in edges(b // 64)]
    assert blocks
    cases = [("standard", *model_case(nhp, orc, "exponential", False, False, data)),
             ("network", *model_case(nhp, orc, "exponential", True, False, data))]
    ln_proc, ln_want = model_case(nhp, orc, "logitnormal", False, False, data)
    # the routes without slices: the same model on a dataset built with NHP_SLICES=0
    ctx = nhp.default_context()
    plain = unsliced_dataset(nhp, route, data)
    pairs = {name: sync_ll(ctx, plain, proc.device_model(ctx)) for name, proc, _ in cases}
    ln_pairs = sync_ll(ctx, plain, ln_proc.device_model(ctx))
    ctx, ds = sliced_dataset(nhp, route, data, k)
    for name, proc, want in cases:
        assert rel(pairs[name], want) < TOL
        model = proc.device_model(ctx)
        for b in blocks:
            for c in (2, 4, 8):
                monkeypatch.setenv("NHP_SLICES_CFG", f"{b},{c}")
                got = sync_ll(ctx, ds, model)
                print(f"k={k} {name} {b},{c}: oracle {rel(got, want):.2e} pair list {rel(got, pairs[name]):.2e}")
                assert rel(got, want) < TOL, (name, b, c, got, want)
                assert rel(got, pairs[name]) < 1e-12, (name, b, c, got, pairs[name])
        monkeypatch.delenv("NHP_SLICES_CFG")
        # the same inputs, the same bits: twice synchronously, then enqueued on both lanes
        a, b2 = sync_ll(ctx, ds, model), sync_ll(ctx, ds, model)
        for slot in (0, 1):
            _lib.check(_lib.lib().nhp_cont_loglik_enqueue(ctx.h, ds.h, model.h, 0, slot), ctx.h)
        lanes = ctx.fetch(0, 2)
        assert a == b2 == lanes[0] == lanes[1], (name, a, b2, lanes)
    # the logit-normal twin
    assert rel(ln_pairs, ln_want) < TOL
    ln_model = ln_proc.device_model(ctx)
    for b in (64, 256, 512):
        if k not in edges(b // 64):
            continue
        for c in (2, 4):
            monkeypatch.setenv("NHP_SLICES_LN_CFG", f"{b},{c}")
            got = sync_ll(ctx, ds, ln_model)
            print(f"k={k} logit-normal {b},{c}: oracle {rel(got, ln_want):.2e} pair list {rel(got, ln_pairs):.2e}")
            assert rel(got, ln_want) < TOL and rel(got, ln_pairs) < 1e-12, (b, c, got, ln_want, ln_pairs)
            assert sync_ll(ctx, ds, ln_model) == got
    monkeypatch.delenv("NHP_SLICES_LN_CFG", raising=False)
    # four models in one pass (k_slices_batch) against their single evaluations
    base = random_case(3, 8, data[2], "exponential", 1.0, seed=21, nhp=nhp)["proc"]      # (copied before it owns a device model)
    x = base.params()
    procs = []
    for q in range(4):
        p = copy.deepcopy(base)
        p.params_(x * (1.0 + 0.03 * q))
        procs.append(p)
    models = [p.device_model(ctx) for p in procs]
    single = np.array([sync_ll(ctx, ds, m) for m in models])
    assert len(set(single)) == 4
    arr = (C.c_void_p * 4)(*[m.h for m in models])
    for b in (256, 512, 1024):
        if k not in edges(b // 64):
            continue
        for c in (2, 4):
            monkeypatch.setenv("NHP_SETS_CFG", f"{b},{c}")
            out = np.empty(4)
            _lib.check(_lib.lib().nhp_cont_loglik_batch(ctx.h, ds.h, arr, 4, 0, _lib.dptr(out)), ctx.h)
            print(f"k={k} batch {b},{c}: {np.max(np.abs(out - single) / np.abs(single)):.2e}")
            assert np.all(np.abs(out - single) <= 1e-11 * np.abs(single)), (b, c, out, single)
            again = np.empty(4)
            _lib.check(_lib.lib().nhp_cont_loglik_batch(ctx.h, ds.h, arr, 4, 0, _lib.dptr(again)), ctx.h)
            assert np.array_equal(out, again)
    monkeypatch.delenv("NHP_SETS_CFG", raising=False)


def test_grid_baseline(nhp, orc, route, monkeypatch):
    """FLAT = false: the child's own time is read at 64·j + lane, whatever order the slices come in."""
    k = 17                                                              # NW = 4: 4·NW+1, NW = 8: 2·NW+1, NW = 16: NW+1
    data = walk_data(k)
    ctx = nhp.default_context()
    plain = unsliced_dataset(nhp, route, data)
    for network in (False, True):
        proc, want = model_case(nhp, orc, "exponential", network, True, data)
        pairs = sync_ll(ctx, plain, proc.device_model(ctx))
        assert rel(pairs, want) < TOL
        ctx, ds = sliced_dataset(nhp, route, data, k)
        model = proc.device_model(ctx)
        for cfg in ("256,2", "512,2", "512,4", "1024,2", "1024,8"):
            monkeypatch.setenv("NHP_SLICES_CFG", cfg)
            got = sync_ll(ctx, ds, model)
            print(f"grid baseline, network={network} {cfg}: oracle {rel(got, want):.2e} pair list {rel(got, pairs):.2e}")
            assert rel(got, want) < TOL and rel(got, pairs) < 1e-12, (cfg, got, want, pairs)
            assert sync_ll(ctx, ds, model) == got
        monkeypatch.delenv("NHP_SLICES_CFG")


@pytest.mark.parametrize("block", BLOCKS)
def test_gradient_at_the_third_round(nhp, route, monkeypatch, block):
    """k_windowed_slices<.., GRAD>: phase A leaves 1/λ of child 64·j + lane in LDS for phase B, in the order phase A walks;
    k = 2·NW + 1 puts one slice into the third round."""
    from nhp_amd import _lib
    nw = block // 64
    k = 2 * nw + 1
    t, nodes, T = walk_data(k, rate=3.0, burst=40)        # (the parent slices sort every node's pairs in one lane: fewer pairs)
    rng = np.random.default_rng(77)
    W = rng.uniform(0.05, 1.0, (3, 3)) / 3 * 2.0
    W[0, 1] = 0.0
    case = dict(N=3, T=T, times=t, nodes=nodes, kind="exponential", dt_max=1.0, lam0=rng.uniform(0.5, 1.5, 3), W=W,
                theta=rng.uniform(0.5, 8.0, (3, 3)), mu=None, tau=None, A=None, grid_x=None, recursive=False)
    res = cr.evaluate(cr.model_of(case), t, nodes, T, recursive=False)
    P = len(res.grad)
    ctx, ds = sliced_dataset(nhp, route, (t, nodes, T), k)
    sc = ds.scalars()
    assert 320 + 16 * 4 + 512 + 8 * (sc["max_item"] + 1) <= 160 * 1024
    delta = 2.0 ** -(48 - max(sc["sl_nb"], int(sc["max_item"]).bit_length()))
    model = cr.process_of(nhp, case).device_model(ctx)
    first = None
    for c in (2, 4, 8):
        monkeypatch.setenv("NHP_SLICES_CFG", f"{block},{c}")
        g, ll = np.full(P, np.nan), C.c_double()
        _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, 0, C.byref(ll), _lib.dptr(g), P), ctx.h)
        assert abs(ll.value - float(res.ll)) <= TOL * abs(float(res.ll)), (block, c, ll.value, float(res.ll))
        ratio, bad, err, B = cr.check(g, res, delta)
        print(f"gradient {block},{c}: error/bound {ratio:.3g}")
        assert len(bad) == 0, f"{block},{c}: {len(bad)} entries outside the bound\n" + cr.explain(g, res, 3, bad, err, B)
        g2, ll2 = np.full(P, np.nan), C.c_double()
        _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, 0, C.byref(ll2), _lib.dptr(g2), P), ctx.h)
        assert ll2.value == ll.value and np.array_equal(g, g2)
