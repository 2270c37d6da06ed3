"""Inside a streak nhp_cont_loglik_enqueue holds one eligible evaluation back and launches it with the next one: two models
in one pass over the dataset's child slices (csrc/cont_slices.hip: k_slices_batch<BLOCK, C, 2, DEFER>; csrc/cont_loglik.hip:
nhp_cont_loglik_enqueue, nhp_ctx::flush_held; include/nhp.h: the enqueue contract).

What is held to what: every enqueued value to the synchronous nhp_cont_loglik of its model with `==` -- the pass of two
repeats the single kernel's arithmetic and order -- and the streak to the oracle at the suite's 1e-11.  How many launches carried
two evaluations is read from nhp_debug_pair_launches, how many joins summed from nhp_debug_finalize_launches.

Data: the small sliced datasets of tests/test_slices_walk_gpu.py (N = 3, NHP_CHUNK = 4096, node 1 with 64(k-1)+5 children, node 2
with 64k, node 3 none, ties and a burst; slicing asserted from the scalars) and the N = 1024 dataset of
tests/test_deferred_finalize_gpu.py (128 children on nodes 1..1023: two columns of 1025 entries in LDS).  Two contexts: `paired`
(the default) and `single`, created under NHP_PAIR_ENQUEUE=0."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import random_case, rel

pytestmark = pytest.mark.gpu

TOL = 1e-11
K = 3                                                    # slices per item of the streak's dataset
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


def big_data():
    N, per = 1024, 128
    M = (N - 1) * per
    rng = np.random.default_rng(4101)
    T = M / 8.0
    t = np.sort(rng.uniform(0.0, T, M))
    nodes = np.repeat(np.arange(1, N, dtype=np.int64), per)
    rng.shuffle(nodes)
    return t, nodes, float(T)


def lib_of(nhp):
    from nhp_amd import _lib
    return _lib


def counter(nhp, ctx, name):
    fn = getattr(lib_of(nhp).lib(), name)
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
    return int(fn(ctx.h))


def pair_launches(nhp, ctx):
    return counter(nhp, ctx, "nhp_debug_pair_launches")


def finalize_launches(nhp, ctx):
    return counter(nhp, ctx, "nhp_debug_finalize_launches")


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


def sliced_dataset(nhp, ctx, data, k):
    """One item per node; asserts the intended slicing (as tests/test_slices_walk_gpu.py)."""
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, 3, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["n_slices"] == 2 * k and sc["all_sole"] == 1, sc
    assert sc["max_item"] == 64 * k and list(ds.array("sl_item0")) == [0, k, 2 * k, 2 * k]
    items = ds.array("items")
    assert list(items["node"]) == [0, 1, 2] and list(items["kend"] - items["kbeg"]) == [64 * (k - 1) + 5, 64 * k, 0]
    return ds


class Side:
    """One context with its own datasets and models."""

    def __init__(self, nhp, env, world):
        with environment(**env):
            self.ctx = nhp.Context()
        self.small = sliced_dataset(nhp, self.ctx, world.small, K)
        self.other = sliced_dataset(nhp, self.ctx, world.small, K)       # the same events, another dataset
        with environment(NHP_CHUNK="4096", NHP_SLICES="0"):
            self.plain = nhp.continuous.DeviceDataset(self.ctx, world.small, 3, 1.0)
        assert self.plain.scalars()["sl_rows"] == 0
        self.models = {name: [device_model(nhp, self.ctx, p) for p in procs] for name, procs in world.procs.items()}
        # one evaluation on either lane: a lane's first launch makes room for its partial sums, which is a joining call
        for slot in (0, 1):
            enqueue(nhp, self.ctx, self.small, self.models["standard"][0], slot)
        self.ctx.fetch(0, 2)

    def close(self):
        # every handle keeps its context alive and destroys itself through it: the context goes with the last of them, also
        # when the traceback of a failed test still holds some
        self.models = self.small = self.other = self.plain = self.ctx = None


class World:
    pass


@pytest.fixture(scope="module")
def world(nhp, orc):
    """Data, processes and oracle values (computed once, left unchanged); the two contexts."""
    w = World()
    w.small = walk_data(K)
    shapes = {"standard": ("exponential", False, False), "network": ("exponential", True, False),
              "lgcp": ("exponential", False, True), "logitnormal": ("logitnormal", False, False)}
    w.procs, w.want = {}, {}
    for name, (kind, network, lgcp) in shapes.items():
        n = 4 if name == "standard" else 1
        cases = [random_case(3, 8, w.small[2], kind, 1.0, network=network, lgcp=lgcp, seed=700 + q, nhp=nhp, orc=orc) for q in range(n)]
        w.procs[name] = [c["proc"] for c in cases]
        w.want[name] = [orc.loglik(c["om"], *w.small, recursive=False) for c in cases]
    assert len(set(w.want["standard"])) == 4
    w.paired = Side(nhp, {}, w)
    w.single = Side(nhp, {"NHP_PAIR_ENQUEUE": "0"}, w)
    yield w
    w.paired.close()
    w.single.close()


def test_streak_to_the_bit(nhp, world):
    """Seven enqueues of four models into seven slots: the first starts at once, the other six go two by two."""
    got = {}
    for name in ("paired", "single"):
        side = getattr(world, name)
        ms = side.models["standard"]
        refs = [sync_ll(nhp, side.ctx, side.small, m) for m in ms]
        side.ctx.synchronize()
        p0, f0 = pair_launches(nhp, side.ctx), finalize_launches(nhp, side.ctx)
        for k in range(7):
            enqueue(nhp, side.ctx, side.small, ms[k % 4], k)
        assert finalize_launches(nhp, side.ctx) == f0                  # an enqueue joins nothing
        got[name] = side.ctx.fetch(0, 7)
        assert pair_launches(nhp, side.ctx) - p0 == (3 if name == "paired" else 0)
        assert finalize_launches(nhp, side.ctx) - f0 == 1
        worst = max(rel(got[name][k], world.want["standard"][k % 4]) for k in range(7))
        print(f"{name}: slots that differ from the synchronous value {sum(got[name][k] != refs[k % 4] for k in range(7))}, oracle {worst:.2e}")
        assert list(got[name]) == [refs[k % 4] for k in range(7)]
        assert worst < TOL
    assert np.array_equal(got["paired"], got["single"])


def test_streak_ends_with_one_held(nhp, world):
    """Six enqueues: the sixth has no partner and is launched by the fetch."""
    side = world.paired
    ms = side.models["standard"]
    refs = [sync_ll(nhp, side.ctx, side.small, m) for m in ms]
    side.ctx.synchronize()
    p0, f0 = pair_launches(nhp, side.ctx), finalize_launches(nhp, side.ctx)
    for k in range(6):
        enqueue(nhp, side.ctx, side.small, ms[k % 4], k)
    got = side.ctx.fetch(0, 6)
    assert pair_launches(nhp, side.ctx) - p0 == 2 and finalize_launches(nhp, side.ctx) - f0 == 1
    assert list(got) == [refs[k % 4] for k in range(6)]


@pytest.mark.parametrize("block", [64, 128, 256, 512])
def test_every_block_and_rows(nhp, world, block):
    """k_slices_batch<BLOCK, C, 2, DEFER> for every C, items that end at the edges of the rounds in which the slices are dealt: an
    item with fewer slices than waves (k = 1), a full round, one more, one into the third round; the childless column."""
    nw = block // 64
    ctx = world.paired.ctx
    ms = world.paired.models["standard"]
    net = world.paired.models["network"][0]
    for k in sorted({1, nw, nw + 1, 2 * nw + 1}):
        ds = sliced_dataset(nhp, ctx, walk_data(k), k)
        for c in (2, 4, 8):
            with environment(NHP_SLICES_CFG=f"{block},{c}"):
                refs = [sync_ll(nhp, ctx, ds, m) for m in ms]
                ref_net = sync_ll(nhp, ctx, ds, net)
                assert len(set(refs)) == 4
                ctx.synchronize()
                p0 = pair_launches(nhp, ctx)
                for s in range(5):
                    enqueue(nhp, ctx, ds, ms[s % 4], s)
                enqueue(nhp, ctx, ds, net, 5)                           # masked models: a pair of their own
                enqueue(nhp, ctx, ds, net, 6)
                got = ctx.fetch(0, 7)
                assert pair_launches(nhp, ctx) - p0 == 3, (block, c, k)
                want = [refs[s % 4] for s in range(5)] + [ref_net, ref_net]
                assert list(got) == want, (block, c, k, got, want)
        ds._fin()


def test_1024_nodes(nhp, world):
    """Two columns of 1025 entries in LDS, 1024 workgroups of 128 threads' worth of children each."""
    ctx = world.paired.ctx
    data = big_data()
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, 1024, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 1024 and sc["n_slices"] == 2 * 1023 and sc["all_sole"] == 1, sc
    procs = [random_case(1024, 8, data[2], "exponential", 1.0, network=True, seed=400 + q, nhp=nhp)["proc"] for q in range(3)]
    ms = [device_model(nhp, ctx, p) for p in procs]
    refs = [sync_ll(nhp, ctx, ds, m) for m in ms]
    assert len(set(refs)) == 3
    for s in range(5):                                                  # (the slots' buffers grow to 1024 partial pairs: joining calls)
        enqueue(nhp, ctx, ds, ms[0], s)
    ctx.synchronize()
    p0, f0 = pair_launches(nhp, ctx), finalize_launches(nhp, ctx)
    for s in range(5):
        enqueue(nhp, ctx, ds, ms[s % 3], s)
    got = ctx.fetch(0, 5)
    assert pair_launches(nhp, ctx) - p0 == 2 and finalize_launches(nhp, ctx) - f0 == 1
    assert list(got) == [refs[s % 3] for s in range(5)]
    ms = None
    ds._fin()


@pytest.mark.parametrize("partner", ["other_dataset", "logitnormal", "network", "lgcp", "recursive", "same_slot", "pair_list"])
def test_partners_that_do_not_pair(nhp, world, partner):
    """One evaluation held, then one that cannot share its pass: both are launched alone, each value is its own."""
    side, L = world.paired, lib_of(nhp)
    ctx, ms = side.ctx, side.models["standard"]
    ds2, m2, flags2, slot2 = side.small, ms[2], 0, 2
    if partner == "other_dataset":
        ds2 = side.other
    elif partner == "pair_list":
        ds2 = side.plain
    elif partner in ("logitnormal", "network", "lgcp"):
        m2 = side.models[partner][0]
    elif partner == "recursive":
        flags2 = L.LL_RECURSIVE
    else:
        slot2 = 1
    ref0, ref1 = sync_ll(nhp, ctx, side.small, ms[0]), sync_ll(nhp, ctx, side.small, ms[1])
    ref2 = sync_ll(nhp, ctx, ds2, m2, flags2)
    spread = abs(ref2 - sync_ll(nhp, ctx, ds2, m2, flags2))            # (0.0 where the route repeats its bits)
    assert partner == "recursive" or spread == 0.0
    if partner in ("logitnormal", "network", "lgcp"):
        assert rel(ref2, world.want[partner][0]) < TOL
    ctx.synchronize()
    p0 = pair_launches(nhp, ctx)
    enqueue(nhp, ctx, side.small, ms[0], 0)
    enqueue(nhp, ctx, side.small, ms[1], 1)                             # held
    enqueue(nhp, ctx, ds2, m2, slot2, flags2)
    got = ctx.fetch(0, 3)
    assert pair_launches(nhp, ctx) == p0
    assert got[0] == ref0
    assert abs(got[slot2] - ref2) <= spread, (partner, got, ref2)
    if slot2 != 1:
        assert got[1] == ref1


@pytest.mark.parametrize("point", ["set_params", "dataset_destroy", "model_destroy", "synchronize", "timer", "batch"])
def test_flush_points(nhp, world, point):
    """One evaluation held before each kind of joining call: that call launches it first, with the parameters, the dataset
    and the model it was enqueued with."""
    side = world.paired
    ctx, ms, procs = side.ctx, side.models["standard"], world.procs["standard"]
    refs = [sync_ll(nhp, ctx, side.small, m) for m in ms]
    m = device_model(nhp, ctx, procs[0])                                # made before the streak: making them is a joining call
    ds = sliced_dataset(nhp, ctx, world.small, K)
    assert sync_ll(nhp, ctx, ds, ms[0]) == refs[0]                      # (its slice planes are built by its first evaluation)
    ctx.synchronize()
    p0, f0 = pair_launches(nhp, ctx), finalize_launches(nhp, ctx)
    if point == "timer":
        ctx.timer_start()
    enqueue(nhp, ctx, side.small, ms[3], 4)
    if point == "set_params":
        enqueue(nhp, ctx, side.small, m, 5)
        m.set_params(procs[1].params())
        assert finalize_launches(nhp, ctx) == f0 + 1
        assert ctx.fetch(5, 1)[0] == refs[0]
        after = sync_ll(nhp, ctx, side.small, m)                        # ... and the next evaluation sees the new parameters
        assert after != refs[0] and rel(after, world.want["standard"][1]) < TOL
    elif point == "dataset_destroy":
        enqueue(nhp, ctx, ds, ms[0], 5)
        ds._fin()
        assert finalize_launches(nhp, ctx) == f0 + 1
        assert ctx.fetch(5, 1)[0] == refs[0]
    elif point == "model_destroy":
        enqueue(nhp, ctx, side.small, m, 5)
        m._fin()
        assert finalize_launches(nhp, ctx) == f0 + 1
        assert ctx.fetch(5, 1)[0] == refs[0]
    elif point == "synchronize":
        enqueue(nhp, ctx, side.small, ms[0], 5)
        assert finalize_launches(nhp, ctx) == f0
        ctx.synchronize()
        assert finalize_launches(nhp, ctx) == f0 + 1
        assert ctx.fetch(5, 1)[0] == refs[0]
    elif point == "timer":
        enqueue(nhp, ctx, side.small, ms[0], 5)
        assert ctx.timer_stop() > 0.0
        assert finalize_launches(nhp, ctx) == f0 + 1
        assert ctx.fetch(5, 1)[0] == refs[0]
    else:
        enqueue(nhp, ctx, side.small, ms[0], 7)                         # (the batch writes slots 0..3)
        out = batch_ll(nhp, ctx, side.small, ms)
        assert np.all(np.abs(out - np.array(refs)) <= 1e-11 * np.abs(refs)), (out, refs)
        assert ctx.fetch(7, 1)[0] == refs[0]
    assert pair_launches(nhp, ctx) == p0
    if point != "batch":                                                # (nhp_cont_loglik and the batch write the first slots)
        assert ctx.fetch(4, 1)[0] == refs[3]


def test_context_close_with_one_held(nhp, world):
    """nhp_ctx_destroy launches what is held while its dataset and model are alive, and waits for it."""
    with environment():
        ctx = nhp.Context()
    ds = sliced_dataset(nhp, ctx, world.small, K)
    m = device_model(nhp, ctx, world.procs["standard"][0])
    ref = sync_ll(nhp, ctx, ds, m)
    assert rel(ref, world.want["standard"][0]) < TOL
    enqueue(nhp, ctx, ds, m, 0)
    enqueue(nhp, ctx, ds, m, 1)                                         # held
    # the handles' own destroy functions would go through the context: they are not called once it is gone (two small
    # allocations stay with the process)
    ds._fin.detach()
    m._fin.detach()
    ctx.close()
    side = world.paired
    assert sync_ll(nhp, side.ctx, side.small, side.models["standard"][0]) == ref     # the device is as it was


@pytest.mark.parametrize("again", [1, 2])
def test_a_slot_changes_its_lane(nhp, world, again):
    """Single into slot 0, slots 1 and 2 in one pass -- both on ONE lane, so one of them not on the lane its own parity names --
    then that slot once more, alone, with another model: the lanes are joined in between and the last value stands."""
    side = world.paired
    ctx, ms = side.ctx, side.models["standard"]
    refs = [sync_ll(nhp, ctx, side.small, m) for m in ms]
    ctx.synchronize()
    p0 = pair_launches(nhp, ctx)
    enqueue(nhp, ctx, side.small, ms[0], 0)
    enqueue(nhp, ctx, side.small, ms[1], 1)
    enqueue(nhp, ctx, side.small, ms[2], 2)
    enqueue(nhp, ctx, side.small, ms[3], again)
    got = ctx.fetch(0, 3)
    assert pair_launches(nhp, ctx) - p0 == 1
    want = [refs[0], refs[1], refs[2]]
    want[again] = refs[3]
    assert list(got) == want
