"""The child-slice kernels' shared exit by quads and the batch kernel's head without its selects (csrc/cont_slices.hip: sl_exit_sums,
the head of k_slices_batch; DESIGN 3.1d, "The exit by quads").  A wave parks 16 quad products and 16 quad exponent sums per model; one
lane of the first wave finishes them.  The head always multiplies by the mask entry (1.0 without a mask) and knows at compile time,
in the paired build, that every item is its node's first.

Data and helpers are those of tests/test_slices_epilogue_gpu.py (imported, not edited): the N = 3 walk datasets with
NHP_CHUNK = 4096 -- node 1 with 64(k-1)+5 children, node 2 with 64k, node 3 with none -- at k in {1, NW, NW+1, 2·NW+1}: waves with no
slice, one slice, two slices and a part-filled last one whose 5 children leave one quad full, one with a single lane and fourteen
of {1.0, 0}; here also last slices of exactly 4 children and of exactly 1.  Every route -- an evaluation alone, in a pair, in a
NHP_PAIR_ENQUEUE=0 and in a NHP_DEFER_FINALIZE=0 context -- equal to the bit and within 1e-11 of the oracle.  Value edges: baselines
from 1e-300 to 1e+300, a model tiny everywhere, and λ = 0 / λ < 0 at children whose lanes all have (lane & 3) != 0, so that they
reach the result through the quad step only.  The head: 128 events per node at N = 1, 3, 1025 (BLOCK 512) and N = 130 (BLOCK 64), a
masked model beside an unmasked one in both orders, and a dataset whose nodes are cut into several items (not all `first`)."""
import numpy as np
import pytest

import test_slices_epilogue_gpu as ep
from helpers import random_case, rel

pytestmark = pytest.mark.gpu

TOL = ep.TOL
world = ep.world                                                        # (the module-scoped fixture: three contexts)


def rem_data(k, rem):
    """ep.walk_data with 64(k-1)+rem events on node 1."""
    n1, n2 = 64 * (k - 1) + rem, 64 * k
    M = n1 + n2
    rng = np.random.default_rng(2000 + 10 * k + rem)
    T = M / 8.0
    t = np.sort(rng.uniform(0.0, T, M))
    nb = M // 4
    b = M // 2
    t[b:b + nb] = np.sort(rng.uniform(t[b], t[b] + 0.7, nb))            # a burst: long windows
    t = np.sort(t)
    nodes = np.r_[np.full(n1, 1), np.full(n2, 2)].astype(np.int64)
    rng.shuffle(nodes)
    return t, nodes, float(T)


def rem_dataset(nhp, ctx, data, k, rem):
    with ep.environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, 3, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["n_slices"] == 2 * k and sc["all_sole"] == 1, sc
    items = ds.array("items")
    assert list(items["kend"] - items["kbeg"]) == [64 * (k - 1) + rem, 64 * k, 0]
    return ds


def cases_on(world, N, data, seed):
    """Three standard models and a masked one with their oracle values."""
    cases = [random_case(N, 8, data[2], "exponential", 1.0, network=(q == 3), seed=seed + q, nhp=world.nhp, orc=world.orc) for q in range(4)]
    want = [world.orc.loglik(c["om"], *data, recursive=False) for c in cases]
    assert len(set(want)) == 4
    return [c["proc"] for c in cases], want


@pytest.mark.parametrize("block", [64, 128, 256, 512])
def test_exit_edges_at_every_block(nhp, world, block):
    nw = block // 64
    for k in sorted({1, nw, nw + 1, 2 * nw + 1}):
        data, procs, want = world.walk_case(k)
        ep.every_route(nhp, world, lambda ctx: ep.walk_dataset(nhp, ctx, data, k), procs, want, f"{block},2", f"BLOCK {block} k {k}")


@pytest.mark.parametrize("rem", [4, 1])
def test_last_slice_of_one_quad_and_of_one_lane(nhp, world, rem):
    """A last slice with exactly 4 children (one full quad, fifteen of {1.0, 0} or {0.5, 1}) and exactly 1 (one lane of one quad);
    k = 1: that slice is the item's only one; k = 2 at 64 threads: the wave's second; k = 9 at 512: the first wave's second."""
    for block, k in ((64, 1), (64, 2), (512, 9)):
        data = rem_data(k, rem)
        procs, want = cases_on(world, 3, data, 8400 + 10 * k + rem)
        ep.every_route(nhp, world, lambda ctx: rem_dataset(nhp, ctx, data, k, rem), procs, want, f"{block},2", f"rem {rem} BLOCK {block} k {k}")


def pair_of(nhp, world, make_dataset, proc_a, proc_b, cfg):
    """ep.pair_of on any dataset: proc_a and proc_b in ONE pass (slots 1 and 2 behind a first evaluation that starts at once), per
    context -> {side: (alone a, alone b, pair launches)}, every enqueued value being the synchronous one's bits (NaN: both NaN)."""
    out = {}
    for name, _ in ep.SIDES:
        ctx = world.ctx[name]
        ds = make_dataset(ctx)
        ma, mb = ep.device_model(nhp, ctx, proc_a), ep.device_model(nhp, ctx, proc_b)
        with ep.environment(**({"NHP_SLICES_CFG": cfg} if cfg else {})):
            ra, rb = ep.sync_ll(nhp, ctx, ds, ma), ep.sync_ll(nhp, ctx, ds, mb)
            for s in range(3):
                ep.enqueue(nhp, ctx, ds, mb, s)
            ctx.synchronize()
            p0 = ep.pair_launches(nhp, ctx)
            ep.enqueue(nhp, ctx, ds, mb, 0)
            ep.enqueue(nhp, ctx, ds, ma, 1)
            ep.enqueue(nhp, ctx, ds, mb, 2)
            got = ctx.fetch(0, 3)
            pairs = ep.pair_launches(nhp, ctx) - p0
        same = lambda x, y: (np.isnan(x) and np.isnan(y)) or x == y
        assert same(got[0], rb) and same(got[1], ra) and same(got[2], rb), (name, cfg, got, ra, rb)
        out[name] = (ra, rb, pairs)
        ma = mb = None
        ds._fin()
    return out


@pytest.mark.parametrize("cfg", ["64,2", "256,2"])
def test_baselines_over_600_orders_of_magnitude(nhp, orc, world, cfg):
    """ep's value edges at workgroups of one and of four waves (ep runs the dataset's own and 512): λ0 = {1e-300, 1e+300, 1} and a
    model whose rates are all about 1e-290, Σ log λ ≈ -2e5: quad exponent sums of ±4000, sixteen of them per (model, wave)."""
    data, W, theta = ep.value_world(world)
    wide, om_wide = ep.exponential(nhp, orc, np.array([1e-300, 1e300, 1.0]), W, theta)
    tiny, om_tiny = ep.exponential(nhp, orc, np.array([1e-300, 1e-280, 1e-300]), W * 1e-290, theta)
    want = [orc.loglik(om, *data, recursive=False) for om in (om_wide, om_tiny)]
    assert np.isfinite(want).all() and want[1] < -1e5
    res = pair_of(nhp, world, lambda ctx: ep.walk_dataset(nhp, ctx, data, 3), wide, tiny, cfg)
    for name, (ra, rb, pairs) in res.items():
        print(f"{cfg} {name}: wide {rel(ra, want[0]):.2e}, tiny {rel(rb, want[1]):.2e}")
        assert rel(ra, want[0]) < TOL and rel(rb, want[1]) < TOL, (name, ra, rb, want)
        assert pairs == (1 if name == "paired" else 0)
    assert res["paired"][:2] == res["single"][:2] == res["fused"][:2]


G = 253


def planted_data():
    """ep.walk_data(3) with two gaps of 2·Δtmax: event G, moved to node 3, has no parent and is the only parent of event G+1 on
    node 2; event G+2 on node 2 has none.  Node 2 keeps 192 children, node 3 gets one."""
    t, nodes, T = ep.walk_data(3)
    t, nodes = t.copy(), nodes.copy()
    nodes[G], nodes[G + 1], nodes[G + 2] = 3, 2, 2
    t[G:] += 2.0
    t[G + 2:] += 2.0
    return t, nodes, float(T + 4.0)


def planted_dataset(nhp, ctx, data):
    """-> (dataset, lanes of node 2's children without a parent, lane of event G+1), the lanes read from the dataset itself."""
    with ep.environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, data, 3, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["all_sole"] == 1, sc
    items, ch = ds.array("items"), ds.array("child_w")
    assert list(items["node"]) == [0, 1, 2] and list(items["kend"] - items["kbeg"])[1:] == [192, 1]
    mine = ch[items["kbeg"][1]:items["kend"][1]]                        # node 2's children in lane order
    length = mine["idx"] - mine["first"]
    empty = [int(p) % 64 for p in np.flatnonzero(length == 0)]
    one = [int(p) % 64 for p in np.flatnonzero(mine["idx"] == G + 1)]
    assert len(one) == 1 and length[mine["idx"] == G + 1][0] == 1
    return ds, empty, one[0]


def test_zero_and_negative_intensity_behind_the_quad_step(nhp, orc, world):
    """λ0 = 0 on node 2 in one model: its children without a parent have λ = 0 exactly -> -inf in that slot.  W[3 -> 2] = -50 in one
    model: event G+1, whose only parent is the one event of node 3, has λ < 0 -> NaN in that slot.  All of these children sit in lanes
    with (lane & 3) != 0 (asserted from the dataset): their mantissas reach the parked product through the DPP steps only.  The other
    model of the pass is untouched."""
    data = planted_data()
    _, W, theta = ep.value_world(world)
    lam0 = np.array([0.7, 1.3, 0.9])
    good, om_good = ep.exponential(nhp, orc, lam0, W, theta)
    want = orc.loglik(om_good, *data, recursive=False)
    zero0 = lam0.copy()
    zero0[1] = 0.0
    zero, _ = ep.exponential(nhp, orc, zero0, W, theta)
    Wn = W.copy()
    Wn[2, 1] = -50.0
    neg, om_neg = ep.exponential(nhp, orc, lam0, Wn, theta)
    lanes = {}

    def make(ctx):
        ds, empty, one = planted_dataset(nhp, ctx, data)
        lanes["empty"], lanes["one"] = empty, one
        return ds

    for bad, check, which in ((zero, lambda v: v == -np.inf, "empty"), (neg, np.isnan, "one")):
        for order in (0, 1):                                            # the bad model first or second in the pass
            a, b = (bad, good) if order == 0 else (good, bad)
            res = pair_of(nhp, world, make, a, b, None)
            hit = lanes[which] if which == "empty" else [lanes[which]]
            print(f"{which}: lanes {hit}")
            assert len(hit) >= 1 and all(l & 3 for l in hit), hit
            for name, (ra, rb, pairs) in res.items():
                rbad, rgood = (ra, rb) if order == 0 else (rb, ra)
                assert check(rbad), (name, order, rbad)
                assert rel(rgood, want) < TOL, (name, order, rgood, want)
                assert pairs == (1 if name == "paired" else 0)
            assert res["paired"][1 - order] == res["single"][1 - order] == res["fused"][1 - order]


@pytest.mark.parametrize("N,cfg", [(1, "512,2"), (3, "512,2"), (1025, "512,2"), (130, "64,2")])
def test_head_trips(nhp, world, N, cfg):
    """N = 1 and 3: most threads of the head have no entry; N = 1025 at 512 threads and N = 130 at 64: a second trip of the batch
    kernel's head (2·BLOCK nodes a trip) with one and two nodes in it."""
    data, procs, want = world.node_case(N)
    ep.every_route(nhp, world, lambda ctx: ep.node_dataset(nhp, ctx, data, N), procs, want, cfg, f"N {N} {cfg}")


@pytest.mark.parametrize("N,cfg", [(1025, "512,2"), (130, "64,2")])
def test_masked_beside_unmasked_in_both_orders(nhp, world, N, cfg):
    """A model that multiplies by its mask enqueued beside one that multiplies by 1.0, in both orders and with later trips of the
    head: each value is its own synchronous one, whichever way the context launches them (the pairing rule keeps a masked and an
    unmasked model in passes of their own; ep.every_route pairs the masked model with itself, in test_head_trips here)."""
    data, procs, want = world.node_case(N)
    for a, b in ((3, 0), (0, 3)):
        res = pair_of(nhp, world, lambda ctx: ep.node_dataset(nhp, ctx, data, N), procs[a], procs[b], cfg)
        for name, (ra, rb, pairs) in res.items():
            assert rel(ra, want[a]) < TOL and rel(rb, want[b]) < TOL, (name, ra, rb, want[a], want[b])
        assert res["paired"][:2] == res["single"][:2] == res["fused"][:2]


def test_items_that_are_not_first(nhp, world):
    """NHP_CHUNK = 48 cuts the 128 children of a node into three items, of which one is `first` and carries the node's integral: no
    pairs (the paired build takes every item for first and is refused such a dataset), the single kernel and the fused batch --
    given the single kernel's workgroup -- take the wave-uniform branch.  Oracle at 1e-11, the routes to the bit."""
    N = 3
    data, procs, want = world.node_case(N)
    got = {}
    for name, _ in ep.SIDES:
        ctx = world.ctx[name]
        with ep.environment(NHP_CHUNK="48"):
            ds = nhp.continuous.DeviceDataset(ctx, data, N, 1.0)
        sc = ds.scalars()
        items = ds.array("items")
        assert sc["sl_rows"] > 0 and sc["all_sole"] == 0 and sc["n_items"] > N and 0 < np.count_nonzero(items["first"]) < len(items), sc
        models = [ep.device_model(nhp, ctx, p) for p in procs]
        with ep.environment(NHP_SLICES_CFG="256,2", NHP_SETS_CFG="256,2"):
            refs = [ep.sync_ll(nhp, ctx, ds, m) for m in models]
            for s in range(4):
                ep.enqueue(nhp, ctx, ds, models[0], s)
            ctx.synchronize()
            p0 = ep.pair_launches(nhp, ctx)
            for s in range(4):
                ep.enqueue(nhp, ctx, ds, models[s], s)
            out = list(ctx.fetch(0, 4))
            assert ep.pair_launches(nhp, ctx) == p0
            assert out == refs, (name, out, refs)
            batch = [ep.batch_ll(nhp, ctx, ds, models[:n]) for n in (2, 3, 4)]
        worst = max(rel(refs[q], want[q]) for q in range(4))
        print(f"{name}: oracle {worst:.2e}, batch of 4 {[rel(b, r) for b, r in zip(batch[2], refs)]}")
        assert worst < TOL, (name, refs, want)
        for b in batch:
            assert list(b) == refs[:len(b)], (name, list(b), refs)
        got[name] = (refs, [list(b) for b in batch])
        models = None
        ds._fin()
    assert got["paired"] == got["single"] == got["fused"], got


def test_a_streak_at_1024_nodes_still_pairs(nhp, world):
    """The pairing rule takes the workgroup's LDS from the launchers' one formula: at N = 1024 two columns and the exit's area of a
    512-thread workgroup must still fit four times per CU, or a streak would quietly fall back to single launches."""
    N = 1024
    rng = np.random.default_rng(8500)
    M = 15 * 64 * 4                                                     # a few nodes with 13+ slices: the 512-thread workgroup
    nodes = rng.integers(1, 5, M).astype(np.int64)
    T = M / 64.0
    t = np.sort(rng.uniform(0.0, T, M))
    case = random_case(N, 8, T, "exponential", 1.0, network=False, seed=8501, nhp=nhp, orc=world.orc)
    want = world.orc.loglik(case["om"], t, nodes, T, recursive=False)
    ctx = world.ctx["paired"]
    with ep.environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, (t, nodes, T), N, 1.0)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["all_sole"] == 1 and sc["max_item"] >= 12 * 64, sc
    model = ep.device_model(nhp, ctx, case["proc"])
    with ep.environment():
        ref = ep.sync_ll(nhp, ctx, ds, model)
        for s in range(7):
            ep.enqueue(nhp, ctx, ds, model, s)
        ctx.synchronize()
        p0 = ep.pair_launches(nhp, ctx)
        for s in range(7):
            ep.enqueue(nhp, ctx, ds, model, s)
        out = list(ctx.fetch(0, 7))
        assert ep.pair_launches(nhp, ctx) - p0 == 3
    assert out == [ref] * 7 and rel(ref, want) < TOL, (out, ref, want)
    ds._fin()
