"""nhp_cont_loglik_enqueue over the context's two lanes: odd slots run on the second internal stream, even ones on the
main stream, and every other call on the context is ordered against both (include/nhp.h: the ordering contract).

Reference values are the synchronous nhp_cont_loglik of the same device model on the same device dataset.  The fused
reduction of the windowed kernels has a fixed order, so two synchronous calls are expected to agree to the bit and the
enqueued path is then held to bit equality; `reference` measures this per model and route instead of assuming it -- a
route whose two synchronous calls differ is held to the spread of those two calls (and to nothing wider).
"""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N0, M0, KBAR = 64, 20_000, 8.0


def _lib(nhp):
    from nhp_amd import _lib as L
    return L


def sync_ll(nhp, ctx, ds, model, flags=0):
    L = _lib(nhp)
    ll = C.c_double()
    L.check(L.lib().nhp_cont_loglik(ctx.h, ds.h, model.h, flags, C.byref(ll)), ctx.h)
    return ll.value


def reference(nhp, ctx, ds, model, flags=0):
    """(value, spread) of two synchronous calls; spread == 0.0 where the route is bit-reproducible."""
    a, b = sync_ll(nhp, ctx, ds, model, flags), sync_ll(nhp, ctx, ds, model, flags)
    assert np.isfinite(a) and np.isfinite(b)
    return a, abs(a - b)


def enqueue(nhp, ctx, ds, model, slot, flags=0):
    L = _lib(nhp)
    L.check(L.lib().nhp_cont_loglik_enqueue(ctx.h, ds.h, model.h, flags, slot), ctx.h)


def same(got, ref):
    value, spread = ref
    return abs(got - value) <= spread          # spread == 0.0: the same bits


def processes(nhp, N, M, T, kind, n):
    """n distinct parameter sets of one shape: the synthetic process with every parameter scaled by 1 + 0.03 k."""
    base = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
    x = base.params()
    out = []
    for k in range(n):
        p = copy.deepcopy(base)
        p.params_(x * (1.0 + 0.03 * k))
        out.append(p)
    return out


def dataset(nhp, ctx, N, M):
    data = nhp.synthetic.s_metric_data(N, M, kbar=KBAR)
    return nhp.continuous.DeviceDataset(ctx, data, N, 1.0), data


def fresh_models(nhp, ctx, procs):
    out = []
    for p in procs:
        d, keep = p.lower()
        out.append(nhp.continuous.DeviceModel(ctx, d))
        del keep
    return out


class Setup:
    def __init__(self, nhp, N, M, kind="exponential", n=4):
        self.ctx = nhp.default_context()
        self.ds, self.data = dataset(nhp, self.ctx, N, M)
        self.procs = processes(nhp, N, M, self.data[2], kind, n)
        self.models = fresh_models(nhp, self.ctx, self.procs)


@pytest.fixture(scope="module")
def small(nhp):
    """N = 64, M = 20 000, four exponential models and their synchronous values (computed once, left unchanged)."""
    s = Setup(nhp, N0, M0)
    s.refs = [reference(nhp, s.ctx, s.ds, m) for m in s.models]
    assert len({r[0] for r in s.refs}) == 4         # the four models are told apart by their values
    return s


@pytest.fixture(scope="module")
def big(nhp):
    """N = 256, M = 200 000: an evaluation that outlasts a host call."""
    return Setup(nhp, 256, 200_000)


def streak(nhp, s, refs, flags_of=lambda k: 0):
    """64 enqueues into slots 0..63 with model k % 4, no synchronisation in between, one fetch."""
    for k in range(64):
        enqueue(nhp, s.ctx, s.ds, s.models[k % 4], k, flags_of(k))
    got = s.ctx.fetch(0, 64)
    bad = [(k, got[k], refs(k)) for k in range(64) if not same(got[k], refs(k))]
    assert not bad, bad[:4]


def test_streak(nhp, small):
    streak(nhp, small, lambda k: small.refs[k % 4])


def test_streak_larger_dataset(nhp, big):
    assert big.ds.scalars()["sl_rows"] > 0          # the child-slices route of the benchmark's headline
    refs = [reference(nhp, big.ctx, big.ds, m) for m in big.models]
    streak(nhp, big, lambda k: refs[k % 4])


def test_streak_logit_normal(nhp):
    s = Setup(nhp, N0, M0, kind="logitnormal")
    refs = [reference(nhp, s.ctx, s.ds, m) for m in s.models]
    streak(nhp, s, lambda k: refs[k % 4])


def test_streak_without_pair_lists(nhp, small, monkeypatch):
    monkeypatch.setenv("NHP_PLIST", "0")            # k_windowed (read on every call)
    refs = [reference(nhp, small.ctx, small.ds, m) for m in small.models]
    streak(nhp, small, lambda k: refs[k % 4])


def test_streak_pair_list(nhp):
    s = Setup(nhp, 256, 2_000)
    assert s.ds.scalars()["sl_rows"] == 0           # the slices rule rejects this dataset: the pair list
    refs = [reference(nhp, s.ctx, s.ds, m) for m in s.models]
    streak(nhp, s, lambda k: refs[k % 4])


def test_streak_one_node(nhp):
    s = Setup(nhp, 1, M0)
    refs = [reference(nhp, s.ctx, s.ds, m) for m in s.models]
    streak(nhp, s, lambda k: refs[k % 4])


def test_streak_with_recursive_evaluations(nhp, small):
    # the recursive formulation on every other odd slot (it stays on the main stream), windowed evaluations on the even
    # and the remaining odd slots
    REC = _lib(nhp).LL_RECURSIVE
    rec = [reference(nhp, small.ctx, small.ds, m, REC) for m in small.models]
    flags_of = lambda k: REC if k % 4 == 1 else 0
    streak(nhp, small, lambda k: rec[k % 4] if k % 4 == 1 else small.refs[k % 4], flags_of)


def test_same_slot_keeps_its_order(nhp, small):
    s = small
    for slot in (3, 4):
        enqueue(nhp, s.ctx, s.ds, s.models[0], slot)
        enqueue(nhp, s.ctx, s.ds, s.models[1], slot)
        assert same(s.ctx.fetch(slot, 1)[0], s.refs[1])


def test_parameter_uploads_between_enqueues(nhp, big):
    # write after enqueue, read after write: the upload waits for the evaluation that still reads the old parameters
    # and the next evaluation sees the new ones, on either lane
    s = big
    xs = [p.params() for p in s.procs]
    m = fresh_models(nhp, s.ctx, [s.procs[0]])[0]
    refs = []
    for x in xs:
        m.set_params(x)
        refs.append(reference(nhp, s.ctx, s.ds, m))
    assert len({r[0] for r in refs}) == 4
    for odd in (1, 0):
        for k in range(200):
            m.set_params(xs[k % 4])
            enqueue(nhp, s.ctx, s.ds, m, (2 * k + odd) % 64)
            if k % 32 == 31 or k == 199:
                got = s.ctx.fetch(0, 64)                # the 32 slots of this lane (8 after the last iteration)
                for j in range(k - k % 32, k + 1):
                    slot = (2 * j + odd) % 64
                    assert same(got[slot], refs[j % 4]), (odd, j, slot, got[slot], refs[j % 4])


def test_timer_spans_both_lanes(nhp, small):
    s = small
    s.ctx.synchronize()
    s.ctx.timer_start()
    for k in range(8):
        enqueue(nhp, s.ctx, s.ds, s.models[k % 4], k)
    assert s.ctx.timer_stop() > 0.0
    got = s.ctx.fetch(0, 8)
    assert all(same(got[k], s.refs[k % 4]) for k in range(8)), got


def test_first_use_on_the_second_lane(nhp, small):
    # a fresh dataset: its layout is built on the main stream by the very evaluation that runs on the second lane
    s = small
    ds = nhp.continuous.DeviceDataset(s.ctx, s.data, N0, 1.0)
    enqueue(nhp, s.ctx, ds, s.models[2], 1)
    assert same(s.ctx.fetch(1, 1)[0], s.refs[2])


def test_destroy_right_after_enqueue(nhp, small):
    s = small
    ds = nhp.continuous.DeviceDataset(s.ctx, s.data, N0, 1.0)
    model = fresh_models(nhp, s.ctx, [s.procs[3]])[0]
    ref = reference(nhp, s.ctx, ds, model)
    assert ref[0] == s.refs[3][0]
    enqueue(nhp, s.ctx, ds, model, 1)
    model._fin()                                    # nhp_cont_model_destroy
    ds._fin()                                       # nhp_cont_dataset_destroy
    assert same(s.ctx.fetch(1, 1)[0], ref)


def test_batch_after_a_streak(nhp, small):
    s, L = small, _lib(nhp)
    order = [0, 1, 2, 3, 3, 2, 1, 0]
    arr = (C.c_void_p * 8)(*[s.models[j].h for j in order])

    def batch():
        out = np.empty(8)
        L.check(L.lib().nhp_cont_loglik_batch(s.ctx.h, s.ds.h, arr, 8, 0, L.dptr(out)), s.ctx.h)
        return out

    # the same call with nothing in flight before it, twice: the batch's own values and their repeatability (the lane
    # sequence and the order of every sum are fixed, so the spread is expected to be 0.0: the same bits)
    s.ctx.synchronize()
    alone = batch()
    s.ctx.synchronize()
    spread = np.abs(batch() - alone)
    for k in range(8):
        enqueue(nhp, s.ctx, s.ds, s.models[k % 4], 2 * k + 1)
    out = batch()
    assert np.all(np.abs(out - alone) <= spread), (out, alone, spread)
    # against the synchronous values: the batch takes compatible models several at a time through its own kernels, whose
    # sums run in another order than the single-model kernel's, so the bits differ (2.1e-10 .. 2.5e-10 absolute at
    # |ll| = 6.3e4, 4e-15 relative).  Bound: ~1.8e5 terms (M events + 8 M pairs) summed in fp64 in two orders differ by
    # at most n * 2^-53 = 2e-11 relative to the sum of magnitudes; the suite holds the batch to 1e-11
    # (test_cont_loglik_gpu.py).
    for j, got in zip(order, out):
        assert abs(got - s.refs[j][0]) <= 1e-11 * abs(s.refs[j][0]), (j, got, s.refs[j])
    got = s.ctx.fetch(0, 16)                        # the batch wrote slots 0..7; the streak's slots 9..15 stand
    assert all(same(got[2 * k + 1], s.refs[k % 4]) for k in range(4, 8)), got
