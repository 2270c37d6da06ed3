"""The head of k_slices_batch<BLOCK, C, S, DEFER> (csrc/cont_slices.hip, DESIGN 3.1d "The pair kernel's head"): the parent nodes
are walked in trips, every load of a trip -- cnt once per node, both models' W, θ and A -- is requested before any is used, and
λ0[m][c] is read once with the item header.  What must not move: every enqueued value is nhp_cont_loglik's of its model to the
bit, equals a NHP_PAIR_ENQUEUE=0 context to the bit, and stays inside the suite's 1e-11 against the oracle.

Node counts sit at the edges of the trips.  A trip is 2·BLOCK nodes in every build of this kernel (128 at BLOCK 64, 1024 at
BLOCK 512); the single kernel's trip at BLOCK 64 is 4·64 = 256, and those edges are kept as well: N in {127, 128, 129, 255, 256,
257, 513} at BLOCK 64, {1023, 1024, 1025} at BLOCK 512, and N = 1, 3 at BLOCK 512, where most threads have no entry at all.

Data, in the manner of tests/test_enqueue_pairs_gpu.py's big_data(): one item per node (NHP_CHUNK = 4096), 128 events on every
node but the first, which has none (N = 1: the 128 events are the only node's), mean window 8; slicing asserted from the
scalars.  Models, oracle values and data are made once per N and left unchanged."""
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


def node_data(N):
    """128 events on each of the nodes 2..N (1-based), none on node 1, shuffled in time; N = 1: 128 events on the only node."""
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


def enqueue(nhp, ctx, ds, model, slot, flags=0):
    L = lib_of(nhp)
    L.check(L.lib().nhp_cont_loglik_enqueue(ctx.h, ds.h, model.h, flags, slot), ctx.h)


def sync_ll(nhp, ctx, ds, model, flags=0):
    L = lib_of(nhp)
    ll = C.c_double()
    L.check(L.lib().nhp_cont_loglik(ctx.h, ds.h, model.h, flags, C.byref(ll)), ctx.h)
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


def sliced_dataset(nhp, ctx, data, N):
    """One item per node, two slices on every node with events; asserts the intended slicing."""
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, N, 1.0)
    sc = ds.scalars()
    busy = max(N - 1, 1)
    assert sc["sl_rows"] > 0 and sc["n_items"] == N and sc["n_slices"] == 2 * busy and sc["all_sole"] == 1, sc
    assert sc["max_item"] == PER
    items = ds.array("items")
    assert list(items["node"]) == list(range(N))
    assert list(items["kend"] - items["kbeg"]) == ([0] if N > 1 else []) + [PER] * busy
    return ds


class World:
    """The two contexts, and per N: data, three standard processes, one masked one, their oracle values."""

    def __init__(self, nhp, orc):
        self.nhp, self.orc = nhp, orc
        with environment():
            self.paired = nhp.Context()
        with environment(NHP_PAIR_ENQUEUE="0"):
            self.single = nhp.Context()

    @functools.lru_cache(maxsize=None)
    def case(self, N):
        data = node_data(N)
        cases = [random_case(N, 8, data[2], "exponential", 1.0, network=(q == 3), seed=5300 + 7 * N + q, nhp=self.nhp, orc=self.orc)
                 for q in range(4)]
        want = [self.orc.loglik(c["om"], *data, recursive=False) for c in cases]
        assert len(set(want)) == 4
        return data, [c["proc"] for c in cases], want

    def close(self):
        self.paired = self.single = None


@pytest.fixture(scope="module")
def world(nhp, orc):
    w = World(nhp, orc)
    yield w
    w.close()


def streak(nhp, ctx, ds, ms, net, cfg, pairs):
    """Five evaluations of three standard models and a pair of the masked one; the synchronous values of the same context."""
    with environment(NHP_SLICES_CFG=cfg):
        refs = [sync_ll(nhp, ctx, ds, m) for m in ms] + [sync_ll(nhp, ctx, ds, net)]
        for s in range(7):                                              # (a slot's buffer grows at its first use: a joining call)
            enqueue(nhp, ctx, ds, ms[0], s)
        ctx.synchronize()
        p0 = pair_launches(nhp, ctx)
        for s in range(5):
            enqueue(nhp, ctx, ds, ms[s % 3], s)
        enqueue(nhp, ctx, ds, net, 5)                                   # masked models: a pair of their own
        enqueue(nhp, ctx, ds, net, 6)
        got = ctx.fetch(0, 7)
        assert pair_launches(nhp, ctx) - p0 == pairs, (cfg, pair_launches(nhp, ctx) - p0)
    return list(got), [refs[s % 3] for s in range(5)] + [refs[3], refs[3]]


CASES = [(64, 2, n) for n in (127, 128, 129, 255, 256, 257, 513)] + [(64, 4, 257), (64, 8, 257)] + \
        [(512, 2, n) for n in (1, 3, 1023, 1024, 1025)] + [(512, 4, 1025), (512, 8, 1025)]


@pytest.mark.parametrize("block,c,N", CASES)
def test_streak_at_the_trip_edges(nhp, world, block, c, N):
    data, procs, want = world.case(N)
    got = {}
    for name, pairs in (("paired", 3), ("single", 0)):
        ctx = getattr(world, name)
        ds = sliced_dataset(nhp, ctx, data, N)
        models = [device_model(nhp, ctx, p) for p in procs]
        got[name], refs = streak(nhp, ctx, ds, models[:3], models[3], f"{block},{c}", pairs)
        worst = max(rel(got[name][s], want[s % 3] if s < 5 else want[3]) for s in range(7))
        print(f"BLOCK {block} C {c} N {N} {name}: slots that differ from the synchronous value "
              f"{sum(g != r for g, r in zip(got[name], refs))}, oracle {worst:.2e}")
        assert got[name] == refs, (block, c, N, name, got[name], refs)
        assert worst < TOL
        models = None
        ds._fin()
    assert got["paired"] == got["single"]


@pytest.mark.parametrize("N", [257, 1025])
@pytest.mark.parametrize("n_models", [2, 3])
def test_fused_route(nhp, world, N, n_models):
    """nhp_cont_loglik_batch goes through the same head with its own (fused) exit; that route promises the oracle's 1e-11, not bits."""
    data, procs, want = world.case(N)
    ctx = world.paired
    ds = sliced_dataset(nhp, ctx, data, N)
    models = [device_model(nhp, ctx, p) for p in procs[:n_models]]
    out = batch_ll(nhp, ctx, ds, models)
    worst = max(rel(out[q], want[q]) for q in range(n_models))
    print(f"N {N}, {n_models} models: oracle {worst:.2e}")
    assert worst < TOL, (out, want[:n_models])
    models = None
    ds._fin()


@pytest.mark.parametrize("N", [129, 1025])
def test_masked_integral_all_first(nhp, world, N):
    """Every item is its node's first (all_sole), so every workgroup adds its column of the integral; with an adjacency mask the
    integral is Σ cnt[p]·a·w.  A pair of the masked model against nhp_cont_loglik, to the bit, and the oracle (which masks too)."""
    data, procs, want = world.case(N)
    ctx = world.paired
    ds = sliced_dataset(nhp, ctx, data, N)
    assert ds.scalars()["all_sole"] == 1
    net = device_model(nhp, ctx, procs[3])
    other = device_model(nhp, ctx, procs[3])                            # the same parameters, a model of its own
    ref = sync_ll(nhp, ctx, ds, net)
    for s in range(3):
        enqueue(nhp, ctx, ds, net, s)
    ctx.synchronize()
    p0 = pair_launches(nhp, ctx)
    enqueue(nhp, ctx, ds, net, 0)
    enqueue(nhp, ctx, ds, net, 1)
    enqueue(nhp, ctx, ds, other, 2)
    got = list(ctx.fetch(0, 3))
    assert pair_launches(nhp, ctx) - p0 == 1
    assert got == [ref, ref, ref], (got, ref)
    assert rel(ref, want[3]) < TOL
    net = other = None
    ds._fin()
