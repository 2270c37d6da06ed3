"""The slice kernels' pair term on the GPU (csrc/nhp_math.h: nhp_exp_term_fast / nhp_exp_term_slow; csrc/cont_slices.hip:
k_slices_batch, k_windowed_slices<., ., ., GRAD = false>): rates from far inside the fast path's limit
(θ·Δtmax = 1015.625·ln 2 = 703.98) to far outside it.

Data: N = 3, one item per node under NHP_CHUNK = 4096 -- node 1 with 69 children (two slices, the second of 5), node 2 with 64,
node 3 with none -- no ties, windows of unequal length inside a slice (padding rows), and eight planted pairs whose delay is
Δtmax·(1 - 2^-30): the top of the records' delay range, where the scaled argument is largest.  Slicing is asserted from the scalars.

For every θ·Δtmax in CASES and every (BLOCK, C) the kernels are built with: the synchronous call, the paired enqueue, the
NHP_PAIR_ENQUEUE=0 enqueue -- equal to the bit -- and nhp_cont_loglik_batch over eight models (groups of four) against the oracle
at the suite's 1e-11.  A model inside the limit paired with one outside it gets the bits it gets alone, in either order."""
import numpy as np
import pytest

from helpers import rel
from test_enqueue_pairs_gpu import batch_ll, device_model, enqueue, environment, pair_launches, sync_ll

pytestmark = pytest.mark.gpu

TOL = 1e-11
LIMIT = 1015.625 * np.log(2.0)                                # θ·Δtmax at the limit: 65000 / (64 / ln 2)
CASES = [1e-6, 1.0, 700.0, LIMIT * (1 - 1e-9), LIMIT * (1 + 1e-9), 800.0, 1e7, 1e8]      # (1e8: the scaled argument passes 2^31)
NAMES = ["1e-6", "1", "700", "just inside", "just outside", "800", "1e7", "1e8"]
DT_MAX = 1.0


def data():
    rng = np.random.default_rng(1801)
    n1, n2, planted = 69, 64, 8
    M = n1 + n2
    T = M / 8.0
    t = np.sort(rng.uniform(1.5, T, M - planted))
    assert np.all(np.diff(t) > 0.0)
    late = t[rng.choice(np.arange(20, M - planted), planted, replace=False)]
    t = np.sort(np.r_[t, late - DT_MAX * (1.0 - 2.0 ** -30)])
    assert np.all(np.diff(t) > 1e-9)
    nodes = np.r_[np.full(n1, 1), np.full(n2, 2)].astype(np.int64)
    rng.shuffle(nodes)
    return t, nodes, float(T)


def processes(nhp, orc, scale, seed):
    """θ[p, c]·Δtmax in [scale/2, scale], the largest entry exactly `scale`."""
    rng = np.random.default_rng(seed)
    lam0 = rng.uniform(0.5, 1.5, 3)
    W = rng.uniform(0.1, 1.0, (3, 3)) * (2.0 / 3.0)
    theta = scale * rng.uniform(0.5, 1.0, (3, 3)) / DT_MAX
    theta[rng.integers(0, 3), rng.integers(0, 2)] = scale / DT_MAX         # (a column that has children)
    om = orc.ContModel(lam0, W, theta=theta, dt_max=DT_MAX, A=None, grid_x=None)
    proc = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(lam0), nhp.ExponentialImpulseResponse(theta, 1.0, 1.0, DT_MAX),
                                               nhp.DenseWeightModel(W))
    return proc, om


def dataset(nhp, ctx, d):
    with environment(NHP_CHUNK="4096"):
        ds = nhp.continuous.DeviceDataset(ctx, d, 3, DT_MAX)
    sc = ds.scalars()
    assert sc["sl_rows"] > 0 and sc["n_items"] == 3 and sc["n_slices"] == 3 and sc["all_sole"] == 1 and sc["max_item"] == 69, sc
    return ds


class World:
    pass


@pytest.fixture(scope="module")
def world(nhp, orc):
    w = World()
    w.data = data()
    made = [processes(nhp, orc, s, 1810 + q) for q, s in enumerate(CASES)]
    w.want = [orc.loglik(om, *w.data, recursive=False) for _, om in made]   # computed once, left unchanged
    assert np.all(np.isfinite(w.want)) and len(set(w.want)) == len(CASES)
    w.ctx, w.ds, w.models = {}, {}, {}
    for side, env in (("paired", {}), ("single", {"NHP_PAIR_ENQUEUE": "0"})):
        with environment(**env):
            w.ctx[side] = nhp.Context()
        w.ds[side] = dataset(nhp, w.ctx[side], w.data)
        w.models[side] = [device_model(nhp, w.ctx[side], p) for p, _ in made]
        for slot in (0, 1):                                                # (a lane's first launch makes room: a joining call)
            enqueue(nhp, w.ctx[side], w.ds[side], w.models[side][1], slot)
        w.ctx[side].fetch(0, 2)
    # the top of the delay range is in the windows (eight pairs at (1 - 2^-30)·Δtmax), and the slices hold padding records
    t = w.data[0]
    gaps = t[:, None] - t[None, :]
    assert np.sum((gaps >= DT_MAX * (1.0 - 2.0 ** -29)) & (gaps < DT_MAX)) >= 8
    sc = w.ds["paired"].scalars()
    assert 64 * sc["sl_rows"] > sc["pairs"] > 0, sc
    yield w
    w.models = w.ds = w.ctx = None


@pytest.mark.parametrize("block", [64, 128, 256, 512])
def test_every_rate_on_every_route(nhp, world, block):
    worst = 0.0
    for c in (2, 4, 8):
        with environment(NHP_SLICES_CFG=f"{block},{c}"):
            for q, name in enumerate(NAMES):
                got = {}
                for side in ("paired", "single"):
                    ctx, ds, m = world.ctx[side], world.ds[side], world.models[side][q]
                    ref = sync_ll(nhp, ctx, ds, m)
                    ctx.synchronize()
                    p0 = pair_launches(nhp, ctx)
                    for slot in range(3):                                  # one alone, two in one pass (or three alone)
                        enqueue(nhp, ctx, ds, m, slot)
                    out = ctx.fetch(0, 3)
                    assert pair_launches(nhp, ctx) - p0 == (1 if side == "paired" else 0)
                    got[side] = [ref] + list(out)
                e = rel(got["paired"][0], world.want[q])
                worst = max(worst, e)
                print(f"block {block} C {c} θ·Δtmax {name}: {got['paired'][0]!r} oracle {world.want[q]!r} rel {e:.2e}")
                assert len(set(got["paired"] + got["single"])) == 1, (block, c, name, got)
                assert e < TOL, (block, c, name, e)
    print(f"block {block}: worst against the oracle {worst:.2e}")


@pytest.mark.parametrize("cfg", [None, "256,2", "512,4", "1024,2"])
def test_batch_of_eight(nhp, world, cfg):
    """Groups of four: every case once as the first of eight, the other rates beside it (inside and outside the limit mixed)."""
    ctx, ds, ms = world.ctx["paired"], world.ds["paired"], world.models["paired"]
    env = {} if cfg is None else {"NHP_SETS_CFG": cfg}
    with environment(**env):
        for q, name in enumerate(NAMES):
            order = [(q + r) % len(CASES) for r in range(8)]
            out = batch_ll(nhp, ctx, ds, [ms[i] for i in order])
            errs = [rel(out[r], world.want[i]) for r, i in enumerate(order)]
            print(f"batch {cfg} from θ·Δtmax {name}: worst {max(errs):.2e}")
            assert max(errs) < TOL, (cfg, name, errs)


@pytest.mark.parametrize("block,c", [(64, 2), (128, 4), (256, 8), (512, 2)])
def test_a_model_outside_the_limit_beside_one_inside(nhp, world, block, c):
    """The pass takes the slow path for both; each model's value is the one it has alone (there: the fast path for the one
    inside), to the bit."""
    ctx, ds, ms = world.ctx["paired"], world.ds["paired"], world.models["paired"]
    with environment(NHP_SLICES_CFG=f"{block},{c}"):
        for inside, outside in ((1, 5), (2, 4), (3, 6), (0, 7)):
            alone = {i: sync_ll(nhp, ctx, ds, ms[i]) for i in (inside, outside)}
            for first, second in ((inside, outside), (outside, inside)):
                ctx.synchronize()
                p0 = pair_launches(nhp, ctx)
                enqueue(nhp, ctx, ds, ms[inside], 0)                       # alone: the streak's first
                enqueue(nhp, ctx, ds, ms[first], 1)
                enqueue(nhp, ctx, ds, ms[second], 2)
                out = ctx.fetch(0, 3)
                assert pair_launches(nhp, ctx) - p0 == 1
                assert list(out) == [alone[inside], alone[first], alone[second]], (block, c, NAMES[inside], NAMES[outside], out, alone)
            assert rel(alone[inside], world.want[inside]) < TOL and rel(alone[outside], world.want[outside]) < TOL

