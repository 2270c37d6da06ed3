"""The slice walk after its row diet (csrc/cont_slices.hip: sl_request, k_slices_batch, k_windowed_slices; DESIGN 3.1d, "The row
diet"): record requests from a scalar base with the rows as immediates, the hi plane without a mask, the slice table through
the scalar cache.  Integer, address and scheduling work only, so every value must keep the bits the tree before it gave.
The models' columns keep their layout in LDS, S planes of N + 1 entries (interleaving them was measured and not taken), so the
column-length cases below hold the unchanged layout under the new requests: they are not a test of a new layout.

What is held to what
  * every enqueued value -- paired context and NHP_PAIR_ENQUEUE=0 context -- to the synchronous nhp_cont_loglik of its model
    with `==`, the pair launches counted as tests/test_enqueue_pairs_gpu.py counts them;
  * every value to the oracle within 1e-11·max(1, |want|), the bound of the existing slice tests;
  * every value to the bits the parent commit's library gave for the same dataset, model and configuration
    (tests/golden/slice_walk_parent_bits.json: this project's own outputs, as float.hex strings; the sampler's draws as integers).

Data (all sliced, one item per node under NHP_CHUNK = 4096, Δtmax = 1; slicing asserted from the scalars and the slice table)
  * rows: N = 3, node 2 owns 64 clusters of 18 events and one of 5, each cluster inside 0.9·Δtmax and 3·Δtmax from the next, so the
    i-th event of a cluster has exactly i parents.  Sorted by window its 1157 children make 19 slices of K = 17, 16, ..., 5, 4, 4,
    3, 2, 1, 0 rows (the last with 5 lanes, the four before it with windows of two lengths): K = 0, 1 and 2C-1, 2C, 2C+1 for C = 2,
    4, 8.  Node 1 has 5 isolated events (one slice of no rows), node 3 none (no slice on any wave).
  * walk(N, active, k): the events of tests/test_slices_walk_gpu.py on the nodes `active` of N -- the first with 64(k-1)+5
    children (k slices, the last with 5 lanes), the second with 64k, a third with 37.  k over {1, NW, NW+1, 2·NW+1} of the
    configuration's NW = BLOCK/64: fewer slices than waves (waves without a slice), a full round, a last slice alone on its wave
    in the second round, one into the third.  N = 1, 3, 257, 1025 with children on the first, a middle and the LAST node: the
    second model's plane at (N+1)·16 bytes, the zero entry at index N, a second head trip at BLOCK = 512 (N = 1025 > 2·512).

The logit-normal, sampler and gradient cases run kernels whose text this change leaves as it was (the gradient build all but:
its slice-table index is clamped); they are here because the issue lists them, and they pin those routes' bits for a later change.
The -DNHP_BATCH_SETS=4 build is not run here: the suite runs the default build."""
import json
import os

import numpy as np
import pytest

import cont_grad_ref as cr
from helpers import random_case
from test_enqueue_pairs_gpu import batch_ll, device_model, enqueue, environment, pair_launches, sync_ll

pytestmark = pytest.mark.gpu

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slice_walk_parent_bits.json")
with open(GOLDEN_PATH) as _f:
    GOLDEN = json.load(_f)

CFGS = ((64, 2), (512, 2), (512, 4), (256, 8))
DT_MAX = 1.0


def within(got, want):
    return abs(got - want) <= 1e-11 * max(1.0, abs(want))


def parent_bits(key, value):
    """`value` (a float, or a list of floats or integers) is what the parent commit's library gave under `key`."""
    got = value.hex() if isinstance(value, float) else [v.hex() if isinstance(v, float) else int(v) for v in value]
    assert key in GOLDEN, key
    assert GOLDEN[key] == got, (key, GOLDEN[key], got)


# ---- data -------------------------------------------------------------------------------------------------------------------
def rows_data():
    rng = np.random.default_rng(1901)
    t, nodes = [], []
    for q, size in enumerate([18] * 64 + [5]):
        start = 3.0 * q
        t += list(start + np.sort(rng.uniform(0.0, 0.9, size)))
        nodes += [2] * size
        if q < 5:
            t.append(start + 1.95)
            nodes.append(1)
    t, nodes = np.array(t), np.array(nodes, dtype=np.int64)
    order = np.argsort(t, kind="stable")
    t, nodes = t[order], nodes[order]
    assert np.all(np.diff(t) > 0.0)
    return t, nodes, float(3.0 * 65)


ROWS_K = list(range(17, 3, -1)) + [4, 3, 2, 1, 0]                # node 2's slices; before them node 1's single slice of no rows


def walk_data(N, active, k, rate=8.0, burst=60, seed=0):
    counts = [64 * (k - 1) + 5, 64 * k, 37][:len(active)]
    M = sum(counts)
    rng = np.random.default_rng(1900 + 31 * k + N + seed)
    T = M / rate
    t = np.sort(rng.uniform(0.0, T, M))
    nt = min(40, M // 4)
    a = M // 6
    t[a:a + nt:2] = t[a + 1:a + nt + 1:2]                              # ties: parents at Δt = 0
    nb = min(burst, M // 4)
    b = M // 2
    t[b:b + nb] = np.sort(rng.uniform(t[b], t[b] + 0.7, nb))           # a burst
    t = np.sort(t)
    nodes = np.concatenate([np.full(c, n) for c, n in zip(counts, active)]).astype(np.int64)
    rng.shuffle(nodes)
    return t, nodes, float(T)


def active_of(N):
    return {1: (1,), 3: (1, 2)}.get(N, (1, N // 2 + 1, N))


def sliced(nhp, ctx, data, N, want_slices):
    """The dataset, one item per node; `want_slices`: slices per item, node by node."""
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, N, DT_MAX)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == N and sc["all_sole"] == 1 and sc["n_slices"] == sum(want_slices), sc
    assert list(np.diff(ds.array("sl_item0"))) == list(want_slices)
    return ds


def slices_of(N, active, k):
    per = dict(zip(active, [k, k, 1]))
    return [per.get(n, 0) for n in range(1, N + 1)]


# ---- the two contexts ---------------------------------------------------------------------------------------------------------
class World:
    pass


@pytest.fixture(scope="module")
def world(nhp):
    w = World()
    w.ctx = {}
    for side, env in (("paired", {}), ("single", {"NHP_PAIR_ENQUEUE": "0"})):
        with environment(**env):
            w.ctx[side] = nhp.Context()
    yield w
    w.ctx = None


def models_for(nhp, orc, N, data, seed):
    """Two standard models and a masked one, with the oracle's values (computed once per dataset)."""
    out = []
    for name, network, s in (("std0", False, seed), ("std1", False, seed + 1), ("mask", True, seed + 2)):
        c = random_case(N, 8, data[2], "exponential", DT_MAX, network=network, seed=s, nhp=nhp, orc=orc)
        out.append((name, c["proc"], orc.loglik(c["om"], *data, recursive=False)))
    return out


def every_route(nhp, world, tag, data, N, want_slices, made, cfgs):
    """Synchronous, paired and unpaired enqueues of `made` on the dataset under every configuration of `cfgs`."""
    sides = {}
    for side, ctx in world.ctx.items():
        ds = sliced(nhp, ctx, data, N, want_slices)
        ms = [device_model(nhp, ctx, p) for _, p, _ in made]
        for slot in range(7):                                               # (the slots' buffers: their first use is a joining call)
            enqueue(nhp, ctx, ds, ms[0], slot)
        ctx.fetch(0, 7)
        sides[side] = (ctx, ds, ms)
    for block, c in cfgs:
        with environment(NHP_SLICES_CFG=f"{block},{c}"):
            got = {}
            for side, (ctx, ds, ms) in sides.items():
                refs = [sync_ll(nhp, ctx, ds, m) for m in ms]
                ctx.synchronize()
                p0 = pair_launches(nhp, ctx)
                for slot, q in enumerate((0, 1, 0, 1, 0)):                  # one alone, then two standard pairs
                    enqueue(nhp, ctx, ds, ms[q], slot)
                enqueue(nhp, ctx, ds, ms[2], 5)                             # masked models: a pair of their own
                enqueue(nhp, ctx, ds, ms[2], 6)
                out = list(ctx.fetch(0, 7))
                assert pair_launches(nhp, ctx) - p0 == (3 if side == "paired" else 0), (tag, block, c, side)
                assert out == [refs[q] for q in (0, 1, 0, 1, 0, 2, 2)], (tag, block, c, side, out, refs)
                # a standard model held, then a masked one: they do not share a pass, each value is its own
                ctx.synchronize()
                p0 = pair_launches(nhp, ctx)
                enqueue(nhp, ctx, ds, ms[0], 0)
                enqueue(nhp, ctx, ds, ms[1], 1)
                enqueue(nhp, ctx, ds, ms[2], 2)
                out = list(ctx.fetch(0, 3))
                assert pair_launches(nhp, ctx) == p0, (tag, block, c, side)
                assert out == refs, (tag, block, c, side, out, refs)
                got[side] = refs
            assert got["paired"] == got["single"], (tag, block, c, got)
            for (name, _, want), v in zip(made, got["paired"]):
                print(f"{tag} {block},{c} {name}: {v!r} oracle {want!r} |diff| {abs(v - want):.2e}")
                assert within(v, want), (tag, block, c, name, v, want)
                parent_bits(f"{tag}/{block},{c}/{name}", v)
    return sides


def release(sides):
    for side in list(sides):
        sides[side] = None


# ---- rows per slice -----------------------------------------------------------------------------------------------------------
def test_every_row_count(nhp, orc, world):
    """K = 0, 1, 2C-1, 2C, 2C+1 under every configuration; a slice of no rows as an item's only slice; an item of no slices."""
    data = rows_data()
    made = models_for(nhp, orc, 3, data, 1910)
    sides = every_route(nhp, world, "rows", data, 3, [1, 19, 0], made, CFGS)
    ds = sides["paired"][1]
    assert list(np.diff(ds.array("sl_row"))[:20]) == [0] + ROWS_K
    items = ds.array("items")
    assert list(items["kend"] - items["kbeg"]) == [5, 18 * 64 + 5, 0]
    for _, c in CFGS:
        assert {0, 1, 2 * c - 1, 2 * c, 2 * c + 1} <= set(ROWS_K)
    release(sides)


# ---- slices per item ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,c", CFGS)
def test_every_round_edge(nhp, orc, world, block, c):
    nw = block // 64
    for k in sorted({1, nw, nw + 1, 2 * nw + 1}):
        data = walk_data(3, (1, 2), k)
        made = models_for(nhp, orc, 3, data, 1920 + k)
        release(every_route(nhp, world, f"walk3-k{k}", data, 3, slices_of(3, (1, 2), k), made, [(block, c)]))


# ---- column lengths: the second plane's distance, the zero entry, the head's second trip ----------------------------------------
@pytest.mark.parametrize("N", [1, 3, 257, 1025])
def test_every_column_length(nhp, orc, world, N):
    active, k = active_of(N), 2
    data = walk_data(N, active, k, burst=60 if N <= 3 else 30)             # (five slices on many nodes: a shorter burst keeps them)
    made = models_for(nhp, orc, N, data, 1940 + N)
    sides = every_route(nhp, world, f"cols{N}", data, N, slices_of(N, active, k), made, CFGS)
    if N > 3:
        assert set(np.unique(data[1])) == {1, N // 2 + 1, N}               # parents on the first, a middle and the last node
    release(sides)


# ---- nhp_cont_loglik_batch: two and three models in one call --------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 1025])
def test_fused_batch(nhp, orc, world, N):
    ctx = world.ctx["paired"]
    active, k = active_of(N), 2
    data = rows_data() if N == 3 else walk_data(N, active, k, burst=30)
    ds = sliced(nhp, ctx, data, N, [1, 19, 0] if N == 3 else slices_of(N, active, k))
    made = models_for(nhp, orc, N, data, 1960 + N)
    ms = [device_model(nhp, ctx, p) for _, p, _ in made]
    for cfg in (None, "256,2", "512,4", "1024,2"):
        with environment(**({} if cfg is None else {"NHP_SETS_CFG": cfg})):
            for take in ((0, 1), (2, 2), (0, 1, 0)):                       # two standard, two masked, three
                out = batch_ll(nhp, ctx, ds, [ms[q] for q in take])
                for r, q in enumerate(take):
                    print(f"batch N={N} {cfg} {take} [{r}]: {out[r]!r} oracle {made[q][2]!r}")
                    assert within(float(out[r]), made[q][2]), (N, cfg, take, r, out[r], made[q][2])
                parent_bits(f"batch{N}/{cfg}/{''.join(map(str, take))}", [float(v) for v in out])


# ---- the slow walk ------------------------------------------------------------------------------------------------------------
def test_slow_walk(nhp, orc, world):
    """θ·Δtmax = 800 > 704: nhp_exp_term_slow, row by row, with the same decode; beside a model inside the limit the pass takes
    the slow walk for both."""
    data = rows_data()
    rng = np.random.default_rng(1970)
    made = []
    for name, scale in (("slow", 800.0), ("fast", 3.0)):
        lam0, W = rng.uniform(0.5, 1.5, 3), rng.uniform(0.1, 1.0, (3, 3)) * (2.0 / 3.0)
        theta = scale * rng.uniform(0.5, 1.0, (3, 3)) / DT_MAX
        theta[1, 1] = scale / DT_MAX                                       # (node 2's own column: the one with the rows)
        om = orc.ContModel(lam0, W, theta=theta, dt_max=DT_MAX, A=None, grid_x=None)
        proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), nhp.ExponentialImpulseResponse(theta, 1.0, 1.0, DT_MAX),
                                                   nhp.DenseWeightModel(W))
        made.append((name, proc, orc.loglik(om, *data, recursive=False)))
    for side, ctx in world.ctx.items():
        ds = sliced(nhp, ctx, data, 3, [1, 19, 0])
        ms = [device_model(nhp, ctx, p) for _, p, _ in made]
        for block, c in CFGS:
            with environment(NHP_SLICES_CFG=f"{block},{c}"):
                refs = [sync_ll(nhp, ctx, ds, m) for m in ms]
                ctx.synchronize()
                p0 = pair_launches(nhp, ctx)
                for slot, q in enumerate((0, 0, 0, 1, 0)):                  # alone, slow with slow, fast with slow
                    enqueue(nhp, ctx, ds, ms[q], slot)
                out = list(ctx.fetch(0, 5))
                assert pair_launches(nhp, ctx) - p0 == (2 if side == "paired" else 0)
                assert out == [refs[q] for q in (0, 0, 0, 1, 0)], (side, block, c, out, refs)
                for (name, _, want), v in zip(made, refs):
                    print(f"slow walk {side} {block},{c} {name}: {v!r} oracle {want!r}")
                    assert within(v, want), (side, block, c, name, v, want)
                    parent_bits(f"slow/{block},{c}/{name}", v)


# ---- the routes that share the request path ---------------------------------------------------------------------------------------
def test_logit_normal(nhp, orc, world):
    ctx = world.ctx["paired"]
    data = walk_data(3, (1, 2), 5)
    ds = sliced(nhp, ctx, data, 3, slices_of(3, (1, 2), 5))
    c = random_case(3, 8, data[2], "logitnormal", DT_MAX, seed=1980, nhp=nhp, orc=orc)
    want = orc.loglik(c["om"], *data, recursive=False)
    m = device_model(nhp, ctx, c["proc"])
    for cfg in (None, "64,2", "512,4"):
        with environment(**({} if cfg is None else {"NHP_SLICES_LN_CFG": cfg})):
            got = sync_ll(nhp, ctx, ds, m)
            print(f"logit-normal {cfg}: {got!r} oracle {want!r}")
            assert within(got, want), (cfg, got, want)
            parent_bits(f"ln/{cfg}", got)


@pytest.mark.parametrize("kind", ["exponential", "logitnormal"])
def test_parent_sampler_sweep(nhp, orc, world, monkeypatch, kind):
    ctx = world.ctx["paired"]
    data = walk_data(3, (1, 2), 5)
    ds = sliced(nhp, ctx, data, 3, slices_of(3, (1, 2), 5))
    c = random_case(3, 8, data[2], kind, DT_MAX, network=True, seed=1985, nhp=nhp, orc=orc)
    want = orc.resample_parents(c["om"], data[0], data[1], orc.uniform_stream(3, 9, len(data[0])), flags=orc.MATH_DET)
    for cfg in (None, "512,8"):                                            # (the draws do not depend on the configuration: one list)
        monkeypatch.delenv("NHP_SAMPLER_CFG", raising=False)
        if cfg is not None:
            monkeypatch.setenv("NHP_SAMPLER_CFG", cfg)
        p, pn = nhp.resample_parents(c["proc"], ds, seed=3, step=9, ctx=ctx)
        assert np.array_equal(p, want[0]) and np.array_equal(pn, want[1]), cfg
        parent_bits(f"sampler/{kind}", list(p) + list(pn))


def test_gradient(nhp, world):
    """k_windowed_slices<., ., ., GRAD>: phase A shares the walk, phase B the requests (on the parent slices)."""
    from nhp_amd import _lib
    import ctypes as C
    ctx = world.ctx["paired"]
    k = 3
    t, nodes, T = walk_data(3, (1, 2), k, rate=3.0, burst=40)
    rng = np.random.default_rng(1990)
    W = rng.uniform(0.05, 1.0, (3, 3)) / 3 * 2.0
    case = dict(N=3, T=T, times=t, nodes=nodes, kind="exponential", dt_max=DT_MAX, lam0=rng.uniform(0.5, 1.5, 3), W=W,
                theta=rng.uniform(0.5, 8.0, (3, 3)), mu=None, tau=None, A=None, grid_x=None, recursive=False)
    res = cr.evaluate(cr.model_of(case), t, nodes, T, recursive=False)
    P = len(res.grad)
    ds = sliced(nhp, ctx, (t, nodes, T), 3, slices_of(3, (1, 2), k))
    sc = ds.scalars()
    delta = 2.0 ** -(48 - max(sc["sl_nb"], int(sc["max_item"]).bit_length()))
    model = cr.process_of(nhp, case).device_model(ctx)
    for block, c in CFGS:
        with environment(NHP_SLICES_CFG=f"{block},{c}"):
            g, ll = np.full(P, np.nan), C.c_double()
            _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, 0, C.byref(ll), _lib.dptr(g), P), ctx.h)
        assert within(ll.value, float(res.ll)), (block, c, ll.value, float(res.ll))
        ratio, bad, err, B = cr.check(g, res, delta)
        print(f"gradient {block},{c}: error/bound {ratio:.3g}")
        assert len(bad) == 0, f"{block},{c}: {len(bad)} entries outside the bound\n" + cr.explain(g, res, 3, bad, err, B)
        parent_bits(f"grad/{block},{c}", [ll.value] + [float(v) for v in g])
