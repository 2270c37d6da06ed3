"""The exit the exponential child-slice kernels share (csrc/cont_slices.hip: sl_exit_park, sl_exit_sums): Σ log λ of
a workgroup as one logarithm per (model, wave) of the wave's mantissa product, the integral's sums parked by quads of lanes in
the head and added by the first wave at the exit.  k_windowed_slices (fused and deferred exit) and k_slices_batch (the pair, the
fused batch of 2 and 4) all call it, so: an evaluation alone, in a pair, in a NHP_PAIR_ENQUEUE=0 context and in a
NHP_DEFER_FINALIZE=0 context are equal to the bit; all are held to the oracle at the suite's 1e-11; the fused batch of two and of
three models (split into passes as nhp_cont_loglik_batch sees fit) to the single evaluations at 1e-11.

Data: the sliced one-item-per-node datasets of tests/test_enqueue_pairs_gpu.py (N = 3, NHP_CHUNK = 4096: node 1 with 64(k-1)+5
children, node 2 with 64k, node 3 with NONE) at k in {1, NW, NW+1, 2·NW+1}: waves without a slice, with exactly one, with two and a
part-filled last one; and tests/test_pair_head_gpu.py's 128 events per node at N = 1, 3 and 1025 (BLOCK 512: two trips of the
head).  Value edges of the formation: baselines from 1e-300 to 1e+300 across the nodes (and a model that is tiny everywhere:
Σ log λ of about -2e5, which a plain product of the rates could not carry), one child with λ = 0 or λ < 0 in one model of a pair
only, a masked model next to an unmasked one."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

from helpers import random_case, rel

pytestmark = pytest.mark.gpu

TOL = 1e-11
PER = 128
BUILD_ENV = ("NHP_CHUNK", "NHP_SLICES", "NHP_SLICES_CFG", "NHP_SLICES_LN", "NHP_SLICES_LN_CFG", "NHP_SETS_CFG", "NHP_BATCH_SLICES",
             "NHP_PLIST", "NHP_XCD", "NHP_SORT", "NHP_DEFER_FINALIZE", "NHP_PAIR_ENQUEUE")
SIDES = (("paired", {}), ("single", {"NHP_PAIR_ENQUEUE": "0"}), ("fused", {"NHP_DEFER_FINALIZE": "0"}))


@contextlib.contextmanager
def environment(**env):
    """The route switches cleared, `env` set, everything put back afterwards."""
    saved = {k: os.environ.pop(k, None) for k in BUILD_ENV}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in BUILD_ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def walk_data(k, rate=8.0, burst=120):
    """tests/test_slices_walk_gpu.py: node 1 with 64(k-1)+5 events, node 2 with 64k, node 3 with none, shuffled in time."""
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


def node_data(N):
    """tests/test_pair_head_gpu.py: 128 events on each of the nodes 2..N, none on node 1; N = 1: 128 events on the only node."""
    nodes = np.repeat(np.arange(2, N + 1, dtype=np.int64), PER) if N > 1 else np.ones(PER, dtype=np.int64)
    M = len(nodes)
    rng = np.random.default_rng(5200 + N)
    T = M / 8.0
    t = np.sort(rng.uniform(0.0, T, M))
    rng.shuffle(nodes)
    return t, nodes, float(T)


def lib_of(nhp):
    from nhp_amd import _lib
    return _lib


def pair_launches(nhp, ctx):
    fn = lib_of(nhp).lib().nhp_debug_pair_launches
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
    return int(fn(ctx.h))


def enqueue(nhp, ctx, ds, model, slot):
    L = lib_of(nhp)
    L.check(L.lib().nhp_cont_loglik_enqueue(ctx.h, ds.h, model.h, 0, slot), ctx.h)


def sync_ll(nhp, ctx, ds, model):
    L = lib_of(nhp)
    ll = C.c_double()
    L.check(L.lib().nhp_cont_loglik(ctx.h, ds.h, model.h, 0, C.byref(ll)), ctx.h)
    return ll.value


def batch_ll(nhp, ctx, ds, models):
    L = lib_of(nhp)
    arr = (C.c_void_p * len(models))(*[m.h for m in models])
    out = np.empty(len(models))
    L.check(L.lib().nhp_cont_loglik_batch(ctx.h, ds.h, arr, len(models), 0, L.dptr(out)), ctx.h)
    return out


def device_model(nhp, ctx, proc):
    d, keep = proc.lower()
    m = nhp.continuous.DeviceModel(ctx, d)
    del keep
    return m


def walk_dataset(nhp, ctx, data, k):
    """One item per node; asserts the intended slicing (as tests/test_enqueue_pairs_gpu.py)."""
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, 3, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["n_slices"] == 2 * k and sc["all_sole"] == 1, sc
    assert sc["max_item"] == 64 * k and list(ds.array("sl_item0")) == [0, k, 2 * k, 2 * k]
    items = ds.array("items")
    assert list(items["node"]) == [0, 1, 2] and list(items["kend"] - items["kbeg"]) == [64 * (k - 1) + 5, 64 * k, 0]
    return ds


def node_dataset(nhp, ctx, data, N):
    """One item per node, two slices on every node with events (as tests/test_pair_head_gpu.py)."""
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, N, 1.0)
    sc = ds.scalars()
    busy = max(N - 1, 1)
    assert sc["sl_rows"] > 0 and sc["n_items"] == N and sc["n_slices"] == 2 * busy and sc["all_sole"] == 1, sc
    assert sc["max_item"] == PER
    return ds


def exponential(nhp, orc, lam0, W, theta, A=None):
    """(process, oracle model) of the given parameters, Δtmax = 1."""
    N = len(lam0)
    base, imp, wm = nhp.HomogeneousProcess(lam0), nhp.ExponentialImpulseResponse(theta, 1.0, 1.0, 1.0), nhp.DenseWeightModel(W)
    if A is None:
        proc = nhp.ContinuousStandardHawkesProcess(base, imp, wm)
    else:
        proc = nhp.ContinuousNetworkHawkesProcess(base, imp, wm, A, nhp.BernoulliNetworkModel(0.5, N))
    return proc, orc.ContModel(lam0, W, theta=theta, dt_max=1.0, A=A)


class World:
    """Three contexts; data, processes and oracle values made once per dataset and left unchanged."""

    def __init__(self, nhp, orc):
        self.nhp, self.orc = nhp, orc
        self.ctx = {}
        for name, env in SIDES:
            with environment(**env):
                self.ctx[name] = nhp.Context()

    @functools.lru_cache(maxsize=None)
    def walk_case(self, k):
        """Three standard models and a masked one on walk_data(k), with their oracle values."""
        data = walk_data(k)
        cases = [random_case(3, 8, data[2], "exponential", 1.0, network=(q == 3), seed=8100 + q, nhp=self.nhp, orc=self.orc) for q in range(4)]
        want = [self.orc.loglik(c["om"], *data, recursive=False) for c in cases]
        assert len(set(want)) == 4
        return data, [c["proc"] for c in cases], want

    @functools.lru_cache(maxsize=None)
    def node_case(self, N):
        data = node_data(N)
        cases = [random_case(N, 8, data[2], "exponential", 1.0, network=(q == 3), seed=8200 + 7 * N + q, nhp=self.nhp, orc=self.orc)
                 for q in range(4)]
        want = [self.orc.loglik(c["om"], *data, recursive=False) for c in cases]
        assert len(set(want)) == 4
        return data, [c["proc"] for c in cases], want

    def close(self):
        self.ctx = None


@pytest.fixture(scope="module")
def world(nhp, orc):
    w = World(nhp, orc)
    yield w
    w.close()


def every_route(nhp, world, make_dataset, procs, want, cfg, label):
    """Three standard models and a masked one: alone (nhp_cont_loglik), enqueued in each of the three contexts -- five standard
    evaluations and two of the masked model, which pair where the context pairs -- and the fused batch of 2 and of 3."""
    got = {}
    for name, _ in SIDES:
        ctx = world.ctx[name]
        ds = make_dataset(ctx)
        models = [device_model(nhp, ctx, p) for p in procs]
        with environment(**({"NHP_SLICES_CFG": cfg} if cfg else {})):
            refs = [sync_ll(nhp, ctx, ds, m) for m in models]
            for s in range(7):                                          # (a slot's buffer grows at its first use: a joining call)
                enqueue(nhp, ctx, ds, models[0], s)
            ctx.synchronize()
            p0 = pair_launches(nhp, ctx)
            for s in range(5):
                enqueue(nhp, ctx, ds, models[s % 3], s)
            enqueue(nhp, ctx, ds, models[3], 5)
            enqueue(nhp, ctx, ds, models[3], 6)
            out = list(ctx.fetch(0, 7))
            assert pair_launches(nhp, ctx) - p0 == (3 if name == "paired" else 0), (label, name)
        expect = [refs[s % 3] for s in range(5)] + [refs[3], refs[3]]
        worst = max(rel(refs[q], want[q]) for q in range(4))
        print(f"{label} {name}: slots that differ from the synchronous value {sum(g != r for g, r in zip(out, expect))}, oracle {worst:.2e}")
        assert out == expect, (label, name, out, expect)
        assert worst < TOL, (label, name, refs, want)
        got[name] = refs
        if name == "paired":                                            # the fused batch: its own BLOCK and C, the same exit
            for n in (2, 3):
                b = batch_ll(nhp, ctx, ds, models[:n])
                assert np.all(np.abs(b - np.array(refs[:n])) <= TOL * np.abs(refs[:n])), (label, n, b, refs[:n])
        models = None
        ds._fin()
    assert got["paired"] == got["single"] == got["fused"], (label, got)


CONFIGS = [(64, 2), (128, 2), (256, 2), (512, 2), (256, 4), (128, 8)]


@pytest.mark.parametrize("block,c", CONFIGS)
def test_every_block_at_the_round_edges(nhp, world, block, c):
    nw = block // 64
    for k in sorted({1, nw, nw + 1, 2 * nw + 1}):
        data, procs, want = world.walk_case(k)
        every_route(nhp, world, lambda ctx: walk_dataset(nhp, ctx, data, k), procs, want, f"{block},{c}", f"BLOCK {block} C {c} k {k}")


@pytest.mark.parametrize("N", [1, 3, 1025])
def test_node_counts_at_block_512(nhp, world, N):
    """N = 1 and 3: most threads of the head have no entry and park 0; N = 1025: two trips, the second with one node."""
    data, procs, want = world.node_case(N)
    every_route(nhp, world, lambda ctx: node_dataset(nhp, ctx, data, N), procs, want, "512,2", f"N {N}")


def value_world(world):
    """walk_data(3) and the parameters the value edges start from."""
    data = walk_data(3)
    rng = np.random.default_rng(8300)
    W = rng.uniform(0.05, 1.0, (3, 3))
    theta = rng.uniform(1.0, 5.0, (3, 3))
    return data, W, theta


def pair_of(nhp, world, data, proc_a, proc_b, cfg):
    """proc_a and proc_b in ONE pass (slots 1 and 2 behind a first evaluation that starts at once), per context; -> {side: (alone
    a, alone b)} after asserting that every enqueued value is the synchronous one's bits (NaN: both NaN)."""
    out = {}
    for name, _ in SIDES:
        ctx = world.ctx[name]
        ds = walk_dataset(nhp, ctx, data, 3)
        ma, mb = device_model(nhp, ctx, proc_a), device_model(nhp, ctx, proc_b)
        with environment(**({"NHP_SLICES_CFG": cfg} if cfg else {})):
            ra, rb = sync_ll(nhp, ctx, ds, ma), sync_ll(nhp, ctx, ds, mb)
            for s in range(3):
                enqueue(nhp, ctx, ds, mb, s)
            ctx.synchronize()
            p0 = pair_launches(nhp, ctx)
            enqueue(nhp, ctx, ds, mb, 0)
            enqueue(nhp, ctx, ds, ma, 1)
            enqueue(nhp, ctx, ds, mb, 2)
            got = ctx.fetch(0, 3)
            pairs = pair_launches(nhp, ctx) - p0
        same = lambda x, y: (np.isnan(x) and np.isnan(y)) or x == y
        assert same(got[0], rb) and same(got[1], ra) and same(got[2], rb), (name, cfg, got, ra, rb)
        out[name] = (ra, rb, pairs)
        ma = mb = None
        ds._fin()
    return out


@pytest.mark.parametrize("cfg", [None, "512,2"])
def test_baselines_over_600_orders_of_magnitude(nhp, orc, world, cfg):
    """λ0 = {1e-300, 1e+300, 1}: 192 children at 1e+300 (exponents of +997 each) next to children at their parents' terms; and a model
    whose rates are all about 1e-290: Σ log λ ≈ -2e5, exponent sums of about -3e5 per workgroup."""
    data, W, theta = value_world(world)
    wide, om_wide = exponential(nhp, orc, np.array([1e-300, 1e300, 1.0]), W, theta)
    tiny, om_tiny = exponential(nhp, orc, np.array([1e-300, 1e-280, 1e-300]), W * 1e-290, theta)
    want = [orc.loglik(om, *data, recursive=False) for om in (om_wide, om_tiny)]
    assert np.isfinite(want).all() and want[1] < -1e5
    res = pair_of(nhp, world, data, wide, tiny, cfg)
    for name, (ra, rb, pairs) in res.items():
        print(f"{cfg} {name}: wide {rel(ra, want[0]):.2e}, tiny {rel(rb, want[1]):.2e}")
        assert rel(ra, want[0]) < TOL and rel(rb, want[1]) < TOL, (name, ra, rb, want)
        assert pairs == (1 if name == "paired" else 0)
    assert res["paired"][:2] == res["single"][:2] == res["fused"][:2]
    ctx = world.ctx["paired"]
    ds = walk_dataset(nhp, ctx, data, 3)
    b = batch_ll(nhp, ctx, ds, [device_model(nhp, ctx, wide), device_model(nhp, ctx, tiny)])
    assert rel(b[0], want[0]) < TOL and rel(b[1], want[1]) < TOL
    ds._fin()


def test_zero_and_negative_intensity_in_one_slot_only(nhp, orc, world):
    """The first event has no parent: λ = λ0 of its node, exactly 0 in the model whose baseline is 0 there -> -inf in that slot.
    A weight of -50 from node 1 to itself makes λ negative at the node's children with a recent parent -> NaN in that slot.  The
    other model of the pass is untouched."""
    data, W, theta = value_world(world)
    first = int(data[1][0]) - 1
    lam0 = np.array([0.7, 1.3, 0.9])
    good, om_good = exponential(nhp, orc, lam0, W, theta)
    want = orc.loglik(om_good, *data, recursive=False)
    zero0 = lam0.copy()
    zero0[first] = 0.0
    zero, _ = exponential(nhp, orc, zero0, W, theta)
    Wn = W.copy()
    Wn[0, 0] = -50.0
    neg, _ = exponential(nhp, orc, lam0, Wn, theta)
    for bad, check in ((zero, lambda v: v == -np.inf), (neg, np.isnan)):
        res = pair_of(nhp, world, data, bad, good, None)
        for name, (ra, rb, pairs) in res.items():
            assert check(ra), (name, ra)
            assert rel(rb, want) < TOL, (name, rb, want)
            assert pairs == (1 if name == "paired" else 0)
        assert res["paired"][1] == res["single"][1] == res["fused"][1]
        ctx = world.ctx["paired"]
        ds = walk_dataset(nhp, ctx, data, 3)
        b = batch_ll(nhp, ctx, ds, [device_model(nhp, ctx, bad), device_model(nhp, ctx, good)])
        assert check(b[0]) and rel(b[1], want) < TOL, b
        ds._fin()


def test_masked_next_to_unmasked(nhp, orc, world):
    """A model with an adjacency mask enqueued next to one without: each value is its own synchronous one, whichever way the
    context launches them, and the fused batch takes the two in one pass."""
    data, W, theta = value_world(world)
    lam0 = np.array([0.7, 1.3, 0.9])
    A = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])
    masked, om_m = exponential(nhp, orc, lam0, W, theta, A=A)
    plain, om_p = exponential(nhp, orc, lam0, W, theta)
    want = [orc.loglik(om, *data, recursive=False) for om in (om_m, om_p)]
    assert want[0] != want[1]
    res = pair_of(nhp, world, data, masked, plain, None)
    for name, (ra, rb, _) in res.items():
        assert rel(ra, want[0]) < TOL and rel(rb, want[1]) < TOL, (name, ra, rb, want)
    assert res["paired"][:2] == res["single"][:2] == res["fused"][:2]
    ctx = world.ctx["paired"]
    ds = walk_dataset(nhp, ctx, data, 3)
    b = batch_ll(nhp, ctx, ds, [device_model(nhp, ctx, masked), device_model(nhp, ctx, plain)])
    assert rel(b[0], want[0]) < TOL and rel(b[1], want[1]) < TOL, (b, want)
    ds._fin()
