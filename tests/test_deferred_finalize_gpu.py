"""Enqueued log-likelihoods over the child slices leave their last sum to the next join (csrc/context.hip: k_finalize_slots;
csrc/cont_slices.hip: the `defer` exit of k_windowed_slices and k_windowed_slices_ln; include/nhp.h: the enqueue contract).

Two contexts made for this module: `deferred` (the default) and `fused`, created under NHP_DEFER_FINALIZE=0, where every
evaluation keeps the fused last-workgroup sum.  The deferred sum repeats the fused one's order, so the two are held to bit
equality; both are held to the oracle at the suite's 1e-11.

Data: N = 3, Δtmax = 1, NHP_CHUNK = 4096 (one item per node): node 1 with 64·2 + 5 children, node 2 with 64·3, node 3 none --
three slices per item, asserted from the dataset's scalars as tests/test_slices_walk_gpu.py does.  One N = 1024 dataset with 128
children on each of the nodes 1..1023 and none on node 1024 (the padding records' node takes 11 bits; 1024 partial pairs per
slot against 3).  Models: exponential and logit-normal impulses, standard and network, five parameter sets each (three at
N = 1024), told apart by their values."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import random_case, rel

pytestmark = pytest.mark.gpu

TOL = 1e-11
K = 3                                                    # slices per item of the small dataset
KINDS = [("exponential", False), ("exponential", True), ("logitnormal", False), ("logitnormal", True)]
BUILD_ENV = ("NHP_CHUNK", "NHP_SLICES", "NHP_SLICES_CFG", "NHP_SLICES_LN", "NHP_SLICES_LN_CFG", "NHP_PLIST", "NHP_XCD", "NHP_SORT",
             "NHP_DEFER_FINALIZE")


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


def small_data():
    n1, n2 = 64 * (K - 1) + 5, 64 * K
    M = n1 + n2
    rng = np.random.default_rng(4100)
    T = M / 8.0
    t = np.sort(rng.uniform(0.0, T, M))
    t[50:70:2] = t[51:71:2]                              # ties: parents at Δt = 0
    t[160:200] = np.sort(rng.uniform(t[160], t[160] + 0.7, 40))      # a burst: windows of up to 40 parents
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


def launches(nhp, ctx):
    fn = lib_of(nhp).lib().nhp_debug_finalize_launches
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


class Side:
    """One context with its own datasets and models."""

    def __init__(self, nhp, env, world):
        with environment(**env):
            self.ctx = nhp.Context()
        with environment(NHP_CHUNK="4096"):
            self.small = nhp.continuous.DeviceDataset(self.ctx, world.small, 3, 1.0)
            self.big = nhp.continuous.DeviceDataset(self.ctx, world.big, 1024, 1.0)
        with environment(NHP_CHUNK="4096", NHP_SLICES="0"):
            self.plain = nhp.continuous.DeviceDataset(self.ctx, world.small, 3, 1.0)
        sc = self.small.scalars()
        assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["n_slices"] == 2 * K and sc["max_item"] == 64 * K, sc
        assert list(self.small.array("sl_item0")) == [0, K, 2 * K, 2 * K]
        sc = self.big.scalars()
        assert sc["sl_rows"] > 0 and sc["n_items"] == 1024 and sc["n_slices"] == 2 * 1023 and sc["sl_nb"] == 11, sc
        item0 = self.big.array("sl_item0")
        assert item0[1023] == item0[1024] == 2 * 1023                    # the last column has no children
        assert self.plain.scalars()["sl_rows"] == 0
        self.models = {kind: [device_model(nhp, self.ctx, p) for p in world.procs[kind]] for kind in KINDS}
        self.big_models = [device_model(nhp, self.ctx, p) for p in world.big_procs]

    def close(self):
        self.models = self.big_models = self.small = self.big = self.plain = None
        self.ctx.close()


class World:
    pass


@pytest.fixture(scope="module")
def world(nhp, orc):
    """Data, processes and oracle values (computed once, left unchanged); the two contexts."""
    w = World()
    w.small, w.big = small_data(), big_data()
    w.procs, w.want = {}, {}
    for kind in KINDS:
        cases = [random_case(3, 8, w.small[2], kind[0], 1.0, network=kind[1], seed=300 + q, nhp=nhp, orc=orc) for q in range(5)]
        w.procs[kind] = [c["proc"] for c in cases]
        w.want[kind] = [orc.loglik(c["om"], *w.small, recursive=False) for c in cases]
        assert len(set(w.want[kind])) == 5
    cases = [random_case(1024, 8, w.big[2], "exponential", 1.0, network=True, seed=400 + q, nhp=nhp, orc=orc) for q in range(3)]
    w.big_procs = [c["proc"] for c in cases]
    w.big_want = [orc.loglik(c["om"], *w.big, recursive=False) for c in cases]
    assert len(set(w.big_want)) == 3
    w.deferred = Side(nhp, {}, w)
    w.fused = Side(nhp, {"NHP_DEFER_FINALIZE": "0"}, w)
    yield w
    w.deferred.close()
    w.fused.close()


def streak(nhp, side, ds, models):
    """2·MAX_SLOTS + 1 enqueues over the rotating models, no join in between; every slot fetched.  Returns the values and,
    per slot, the index of the model whose evaluation came last."""
    S = lib_of(nhp).MAX_SLOTS
    n, R = 2 * S + 1, len(models)
    for k in range(n):
        enqueue(nhp, side.ctx, ds, models[k % R], k % S)
    last = np.array([(2 * S if s == 0 else S + s) % R for s in range(S)])
    return side.ctx.fetch(0, S), last


def check_streak(nhp, w, pick, want):
    before = launches(nhp, w.deferred.ctx)
    got_d, last = streak(nhp, w.deferred, *pick(w.deferred))
    assert launches(nhp, w.deferred.ctx) > before
    got_f, _ = streak(nhp, w.fused, *pick(w.fused))
    assert launches(nhp, w.fused.ctx) == 0
    expect = np.array(want)[last]
    worst = np.max(np.abs(got_d - expect) / np.abs(expect))
    print(f"deferred against the oracle: {worst:.2e}; slots that differ from the fused sum: {int(np.sum(got_d != got_f))}")
    assert np.array_equal(got_d, got_f)
    assert worst < TOL


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"{k[0]}-{'network' if k[1] else 'standard'}")
def test_deferred_against_fused(nhp, world, kind):
    check_streak(nhp, world, lambda side: (side.small, side.models[kind]), world.want[kind])


def test_deferred_against_fused_1024_nodes(nhp, world):
    check_streak(nhp, world, lambda side: (side.big, side.big_models), world.big_want)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"{k[0]}-{'network' if k[1] else 'standard'}")
def test_single_calls_and_batch(nhp, world, kind):
    """nhp_cont_loglik and nhp_cont_loglik_batch keep the fused sum: the same bits from both contexts, with slots pending in
    the deferred one when they are called."""
    d, f = world.deferred, world.fused
    for s in (0, 1, 2):
        enqueue(nhp, d.ctx, d.small, d.models[kind][4], s)
    single_d = [sync_ll(nhp, d.ctx, d.small, m) for m in d.models[kind]]
    single_f = [sync_ll(nhp, f.ctx, f.small, m) for m in f.models[kind]]
    assert single_d == single_f
    assert all(rel(g, v) < TOL for g, v in zip(single_d, world.want[kind]))
    enqueue(nhp, d.ctx, d.small, d.models[kind][4], 1)
    enqueue(nhp, d.ctx, d.small, d.models[kind][3], 7)
    out_d, out_f = batch_ll(nhp, d.ctx, d.small, d.models[kind]), batch_ll(nhp, f.ctx, f.small, f.models[kind])
    assert np.array_equal(out_d, out_f)
    assert all(rel(g, v) < TOL for g, v in zip(out_d, world.want[kind]))
    assert d.ctx.fetch(7, 1)[0] == single_d[3]            # the batch wrote slots 0..4; the pending slot behind them stands


def test_slot_reuse(nhp, world):
    d = world.deferred
    for kind in KINDS:
        ms = d.models[kind]
        ref = sync_ll(nhp, d.ctx, d.small, ms[1])
        for slot in (5, 6):
            enqueue(nhp, d.ctx, d.small, ms[0], slot)
            enqueue(nhp, d.ctx, d.small, ms[1], slot)
        got = d.ctx.fetch(5, 2)
        assert got[0] == got[1] == ref, (kind, got, ref)


def test_two_grid_sizes_in_one_launch(nhp, world):
    d = world.deferred
    kind = KINDS[0]
    refs = [sync_ll(nhp, d.ctx, d.small, d.models[kind][2]), sync_ll(nhp, d.ctx, d.big, d.big_models[1])]
    assert rel(refs[0], world.want[kind][2]) < TOL and rel(refs[1], world.big_want[1]) < TOL
    before = launches(nhp, d.ctx)
    enqueue(nhp, d.ctx, d.small, d.models[kind][2], 0)      # 3 partial pairs
    enqueue(nhp, d.ctx, d.big, d.big_models[1], 1)          # 1024
    enqueue(nhp, d.ctx, d.big, d.big_models[1], 2)
    enqueue(nhp, d.ctx, d.small, d.models[kind][2], 3)
    got = d.ctx.fetch(0, 4)
    assert launches(nhp, d.ctx) == before + 1
    assert list(got) == [refs[0], refs[1], refs[1], refs[0]]


@pytest.mark.parametrize("join", ["fetch", "synchronize", "timer", "set_params", "dataset_destroy"])
@pytest.mark.parametrize("slot", [2, 3])
def test_joins(nhp, world, join, slot):
    """A pending slot before each kind of joining call: the sum is made by that call (one launch) and holds the value of
    the parameters and the dataset the evaluation was enqueued with."""
    d = world.deferred
    kind = KINDS[0]
    procs = world.procs[kind]
    ref = sync_ll(nhp, d.ctx, d.small, d.models[kind][0])
    d.ctx.synchronize()
    before = launches(nhp, d.ctx)
    if join == "set_params":
        m = device_model(nhp, d.ctx, procs[0])
        enqueue(nhp, d.ctx, d.small, m, slot)
        m.set_params(procs[1].params())
        assert launches(nhp, d.ctx) == before + 1
        assert d.ctx.fetch(slot, 1)[0] == ref
        after = sync_ll(nhp, d.ctx, d.small, m)             # ... and the next evaluation sees the new parameters
        assert after != ref and rel(after, world.want[kind][1]) < TOL
    elif join == "dataset_destroy":
        with environment(NHP_CHUNK="4096"):
            ds = nhp.continuous.DeviceDataset(d.ctx, world.small, 3, 1.0)
        assert ds.scalars()["n_slices"] == 2 * K
        enqueue(nhp, d.ctx, ds, d.models[kind][0], slot)
        ds._fin()                                           # nhp_cont_dataset_destroy: the partial sums are the context's
        assert launches(nhp, d.ctx) == before + 1
        assert d.ctx.fetch(slot, 1)[0] == ref
    elif join == "timer":
        enqueue(nhp, d.ctx, d.small, d.models[kind][0], slot)
        d.ctx.timer_start()
        assert launches(nhp, d.ctx) == before + 1
        enqueue(nhp, d.ctx, d.small, d.models[kind][0], slot + 2)
        assert d.ctx.timer_stop() > 0.0
        assert launches(nhp, d.ctx) == before + 2
        got = d.ctx.fetch(slot, 3)
        assert got[0] == got[2] == ref
    else:
        enqueue(nhp, d.ctx, d.small, d.models[kind][0], slot)
        assert launches(nhp, d.ctx) == before             # an enqueue joins nothing
        if join == "synchronize":
            d.ctx.synchronize()
            assert launches(nhp, d.ctx) == before + 1
        assert d.ctx.fetch(slot, 1)[0] == ref
    assert launches(nhp, d.ctx) == before + (2 if join == "timer" else 1)


@pytest.mark.parametrize("slot", [3, 4])
def test_overwrites(nhp, world, slot):
    """A pending slot, then an evaluation that writes the slot's value itself: the later one wins."""
    d, L = world.deferred, lib_of(nhp)
    kind = KINDS[0]
    ms = d.models[kind]
    rec = sync_ll(nhp, d.ctx, d.small, ms[1], L.LL_RECURSIVE)
    spread = abs(rec - sync_ll(nhp, d.ctx, d.small, ms[1], L.LL_RECURSIVE))     # (0.0 where the route repeats its bits)
    windowed = sync_ll(nhp, d.ctx, d.small, ms[0])
    assert abs(windowed - rec) > 1e-6 * abs(rec)
    enqueue(nhp, d.ctx, d.small, ms[0], slot)
    enqueue(nhp, d.ctx, d.small, ms[1], slot, L.LL_RECURSIVE)
    assert abs(d.ctx.fetch(slot, 1)[0] - rec) <= spread
    # ... and the pair-list kernel of a dataset without slices, which stays on the slot's lane and joins nothing
    plain = sync_ll(nhp, d.ctx, d.plain, ms[2])
    before = launches(nhp, d.ctx)
    enqueue(nhp, d.ctx, d.small, ms[0], slot)
    enqueue(nhp, d.ctx, d.plain, ms[2], slot)
    enqueue(nhp, d.ctx, d.small, ms[3], slot + 2)
    got = d.ctx.fetch(slot, 3)
    assert launches(nhp, d.ctx) == before + 1
    assert got[0] == plain and got[2] == sync_ll(nhp, d.ctx, d.small, ms[3])


def test_empty_joins_launch_nothing(nhp, world):
    d, f = world.deferred, world.fused
    kind = KINDS[2]
    d.ctx.synchronize()
    before = launches(nhp, d.ctx)
    d.ctx.synchronize()
    d.ctx.fetch(0, 8)
    d.ctx.timer_start()
    d.ctx.timer_stop()
    sync_ll(nhp, d.ctx, d.small, d.models[kind][0])
    batch_ll(nhp, d.ctx, d.small, d.models[kind])
    enqueue(nhp, d.ctx, d.plain, d.models[kind][0], 1)      # the pair-list route defers nothing
    d.ctx.fetch(1, 1)
    assert launches(nhp, d.ctx) == before
    enqueue(nhp, f.ctx, f.small, f.models[kind][0], 1)      # NHP_DEFER_FINALIZE=0: nor does the slices route
    assert f.ctx.fetch(1, 1)[0] == sync_ll(nhp, f.ctx, f.small, f.models[kind][0])
    assert launches(nhp, f.ctx) == 0
