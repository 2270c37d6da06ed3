"""k_sampler_slices (csrc/cont_slices.hip), the parent sampler of a sliced dataset, against the oracle's sequential draw on
datasets that KEEP their slices.  Every dataset is built explicitly with its item size (NHP_CHUNK), and every test first holds
the dataset's scalars to the layout rule restated in numpy (tests/slices_ref.py): a dataset that fell back to the pair list
fails there, before a single index is compared.  tests/test_sampler_slices_host.py shows on the CPU that each input holds what
its case is named for (tests/sampler_slices_cases.py lists them).

Everything compared is integers or bits: np.array_equal is the bound.

Per input, for both impulse kinds, a standard model and a network model with an LGCP baseline, and every (workgroup, cache)
shape: parents and parent nodes equal the oracle's (flags = MATH_DET) for explicit uniforms -- with 0 and the largest double
below 1 planted -- and for the Philox stream; the lane-per-child kernel (NHP_SAMPLER_SLICES=0 with NHP_SAMPLER_EXPO_SLICES=0)
and the single-lane kernel (NHP_SAMPLER=1) give the same arrays on the same dataset.

Which kernel ran cannot be seen from outside.  The tests pin the conditions nhp_launch_sampler_slices decides on: sl_rows > 0,
an exponential or logit-normal model, sl_max_rows + 1 <= 1024.  For the bursts of case D that is sl_max_rows = 1022 and 1023
(the slice kernel, up to 1024 weights summed in sequence) and 1024 (back to the single-lane kernel and its pairwise sum).

Uniforms drawn at random almost never fall within an ulp of a threshold, so they do not see a sum or a share whose last bit is
wrong.  Each case therefore also runs two uniform vectors that sit ON the oracle's thresholds (cases.threshold_uniforms: cp_k
of a random parent k of every child, found by bisecting the oracle itself, and the double below it).

What these found in the kernel as it was: k_sampler_slices took the exponential rate as θ where the reference, the oracle and
the other two sampler kernels take inv(scale) = 1/(1/θ).  The two differ in the last bit for about one θ in six, the weights
with them, and on the threshold uniforms the indices: 27 of the 80 tests here were red (every exponential case of A, B, E,
F-9 and F-9-short, one of F-1-short; C, D, F-1 and the logit-normal kind green), all 80 green with random uniforms alone.
Fixed in the kernel.

Planted mistakes (scratch builds of the fixed k_sampler_slices, one mistake each, arithmetic only; this file run once per
build, 80 tests):
  1. the baseline added first instead of last in the sum: 67 red -- all 64 index cases (A, B, C, E, F; both kinds, both
     models) and the bursts D-1023, D-1024 (both kinds); D-1025 green, as it must be: it runs the single-lane kernel.
  2. colw[p] without the mask A: 20 red -- every logit-normal network case (14 index cases: F-1 and F-1-short have a 1 x 1 mask
     of 1), and the statistics, column-shard and device-build tests of the logit-normal kind; the exponential kind reads its
     a·w from the other column and stays green, the standard models have no mask.
  3. wk_at(kk2) / s replaced by a multiplication with 1.0 / s: 67 red, the same 67 as for 1.
Before the threshold uniforms were added, 1 and 3 were green everywhere (80 passed each): with random and planted uniforms
alone the file could not go red for a last-bit mistake.  The statistics, shard, device-build and error-flag tests draw from the
Philox stream or random uniforms and stay green for 1 and 3."""
import numpy as np
import pytest

import sampler_slices_cases as cases
import slices_ref as sr

pytestmark = pytest.mark.gpu

INPUTS = cases.inputs()
ROUTE_ENV = ("NHP_CHUNK", "NHP_SLICES", "NHP_SAMPLER", "NHP_SAMPLER_SLICES", "NHP_SAMPLER_EXPO_SLICES", "NHP_SAMPLER_CFG", "NHP_PLQ",
             "NHP_GROUP", "NHP_XCD", "NHP_SORT")
CFGS = (None, "256,8", "256,16", "512,8", "512,16")
OTHER_KERNELS = ({"NHP_SAMPLER_SLICES": "0", "NHP_SAMPLER_EXPO_SLICES": "0"}, {"NHP_SAMPLER": "1"})
PINNED = ("pairs", "n_items", "max_item", "max_window", "sl_rows", "n_slices", "sl_max_rows")


@pytest.fixture
def route(monkeypatch, nhp):
    def use(env):
        for key in ROUTE_ENV:
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, v)
    use({})
    yield use
    for key in ROUTE_ENV:
        monkeypatch.delenv(key, raising=False)
    nhp.invalidate_device_datasets()


def sliced_dataset(nhp, route, inp, columns=None, build="host"):
    """The dataset of an input with its item size; its scalars are the restated layout's, slices kept."""
    route({"NHP_CHUNK": str(inp.chunk)})
    ctx = nhp.default_context()
    ds = nhp.continuous.DeviceDataset(ctx, inp.data, inp.N, inp.dt_max, columns=columns, build=build)
    route({})
    nhp.invalidate_device_datasets()
    want = sr.layout(inp.times, inp.nodes, inp.N, inp.dt_max, inp.chunk, columns=columns)
    sc = ds.scalars()
    assert want.kept and sc["sl_rows"] > 0, (inp.name, sc)
    assert {f: sc[f] for f in PINNED} == want.scalars(), (inp.name, sc, want.scalars())
    assert sc["sl_nb"] == want.sl_nb
    return ds, want


def same_bits(a, b):
    """Equal bit for bit, a NaN (a pair of nodes without a drawn parent) standing where the other has one."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    m = ~np.isnan(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[m].view(np.uint64), b[m].view(np.uint64))


def oracle_draws(orc, om, inp, u):
    return orc.resample_parents(om, inp.times, inp.nodes, u, flags=orc.MATH_DET)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def check_input(nhp, orc, route, inp, kind, network, lgcp, cfgs=CFGS):
    ds, lay = sliced_dataset(nhp, route, inp)
    proc, om = cases.models(inp, kind, network, lgcp, nhp=nhp, orc=orc)
    M = len(inp.times)
    u = cases.uniforms(M)
    want_u = oracle_draws(orc, om, inp, u)
    want_s = oracle_draws(orc, om, inp, orc.uniform_stream(3, 9, M))
    cases.check_planted_uniforms(inp, kind, network, lay.window, u, *want_u)
    assert want_u[0][0] == 0 and want_u[1][0] == 0
    # uniforms on the oracle's own thresholds and one double below: a last-bit difference in a sum or a share shows
    u_at, u_below, found = cases.thresholds(orc, inp, kind, network, lgcp, lay.window)
    want_at, want_below = oracle_draws(orc, om, inp, u_at), oracle_draws(orc, om, inp, u_below)
    assert np.all(want_at[0][found] != want_below[0][found])
    for cfg in cfgs:
        route({"NHP_SAMPLER_CFG": cfg} if cfg else {})
        assert same(nhp.resample_parents(proc, ds, u=u), want_u), (inp.name, kind, network, cfg, "u")
        assert same(nhp.resample_parents(proc, ds, seed=3, step=9), want_s), (inp.name, kind, network, cfg, "philox")
        assert same(nhp.resample_parents(proc, ds, u=u_at), want_at), (inp.name, kind, network, cfg, "on the thresholds")
        assert same(nhp.resample_parents(proc, ds, u=u_below), want_below), (inp.name, kind, network, cfg, "below the thresholds")
    for env in OTHER_KERNELS:
        route(env)
        assert same(nhp.resample_parents(proc, ds, u=u), want_u), (inp.name, kind, network, env, "u")
        assert same(nhp.resample_parents(proc, ds, seed=3, step=9), want_s), (inp.name, kind, network, env, "philox")
        assert same(nhp.resample_parents(proc, ds, u=u_at), want_at), (inp.name, kind, network, env, "on the thresholds")
        assert same(nhp.resample_parents(proc, ds, u=u_below), want_below), (inp.name, kind, network, env, "below the thresholds")
    route({})
    return ds, proc, om


@pytest.mark.parametrize("network,lgcp", cases.VARIANTS)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", cases.MAIN)
def test_indices_equal_the_oracle_on_sliced_data(nhp, orc, route, name, kind, network, lgcp):
    check_input(nhp, orc, route, INPUTS[name], kind, network, lgcp)


@pytest.mark.parametrize("name,kind", [("D-1023", "exponential"), ("D-1024", "exponential"), ("D-1025", "exponential"),
                                       ("D-1024", "logitnormal")])
def test_bursts_on_either_side_of_the_pairwise_sum(nhp, orc, route, name, kind):
    """The longest window has B - 1 parents: B weights with the baseline.  B = 1024 is the most the slice kernel takes (1024
    weights summed in sequence, as Julia's sum does up to there); at B = 1025 sl_max_rows + 1 > 1024 hands the dataset to the
    single-lane kernel, which sums pairwise above the threshold.  The route is not observable: the scalars on either side of
    the rule are pinned here, the indices must equal the oracle's on both."""
    inp = INPUTS[name]
    B = int(name.split("-")[1])
    ds, _, _ = check_input(nhp, orc, route, inp, kind, False, False)
    sc = ds.scalars()
    assert sc["sl_max_rows"] == B - 1 and sc["max_window"] == B - 1 and sc["sl_rows"] > 0


@pytest.mark.parametrize("chunk", [256, 4096])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_statistics_on_sliced_data(nhp, orc, route, kind, chunk):
    inp = INPUTS[f"A-{chunk}"]
    ds, _ = sliced_dataset(nhp, route, inp)
    proc, om = cases.models(inp, kind, True, False, nhp=nhp, orc=orc)
    t, nodes, N, M = inp.times, inp.nodes, inp.N, len(inp.times)
    want = oracle_draws(orc, om, inp, orc.uniform_stream(5, 2, M))
    for cfg in CFGS:
        route({"NHP_SAMPLER_CFG": cfg} if cfg else {})
        p, pn, st = nhp.resample_parents(proc, ds, seed=5, step=2, with_stats=True)
        assert same((p, pn), want), cfg
        assert np.array_equal(st["cnt0"], orc.baseline_node_counts(nodes, pn, N))
        assert np.array_equal(st["Mn"], orc.node_counts(nodes, N))
        assert np.array_equal(st["Mnm"], orc.parent_counts(nodes, pn, N))
        assert st["Mnm"].sum() + st["cnt0"].sum() == M
        if kind == "exponential":
            assert same_bits(st["Xnm"], orc.duration_mean(t, nodes, p, N))
        else:
            X, V = orc.log_duration_stats(t, nodes, p, N, inp.dt_max)
            assert np.array_equal(np.isnan(st["Xnm"]), np.isnan(X))
            m = ~np.isnan(X)
            assert np.allclose(st["Xnm"][m], X[m], rtol=1e-12, atol=1e-13)
            assert np.allclose(st["Vnm"], V, rtol=1e-11, atol=1e-12)
        none_p, none_pn, st2 = nhp.resample_parents(proc, ds, seed=5, step=2, with_stats=True, want_parents=False)
        assert none_p is None and none_pn is None
        for key in ("cnt0", "Mn", "Mnm", "Xnm", "Vnm"):
            assert same_bits(st2[key], st[key]), (cfg, key)
    route({})


@pytest.mark.parametrize("chunk", [256, 4096])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_column_shards_of_sliced_data(nhp, orc, route, kind, chunk):
    inp = INPUTS[f"A-{chunk}"]
    whole, _ = sliced_dataset(nhp, route, inp)
    proc, om = cases.models(inp, kind, True, True, nhp=nhp, orc=orc)
    M = len(inp.times)
    u = cases.uniforms(M)
    want = oracle_draws(orc, om, inp, u)
    assert same(nhp.resample_parents(proc, whole, u=u), want)
    total = [np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)]
    for columns in ((0, 3), (3, 9)):
        ds, _ = sliced_dataset(nhp, route, inp, columns=columns)
        foreign = (inp.nodes - 1 < columns[0]) | (inp.nodes - 1 >= columns[1])
        for cfg in CFGS:
            route({"NHP_SAMPLER_CFG": cfg} if cfg else {})
            p, pn = nhp.resample_parents(proc, ds, u=u)
            assert np.all(p[foreign] == 0) and np.all(pn[foreign] == 0), (columns, cfg)
            assert np.array_equal(p[~foreign], want[0][~foreign]) and np.array_equal(pn[~foreign], want[1][~foreign]), (columns, cfg)
        route({})
        total[0] += p
        total[1] += pn
    assert same(total, want)


@pytest.mark.parametrize("chunk", [256, 4096])
def test_device_built_sliced_data(nhp, orc, route, chunk):
    inp = INPUTS[f"A-{chunk}"]
    host, _ = sliced_dataset(nhp, route, inp)
    dev, _ = sliced_dataset(nhp, route, inp, build="device")
    assert dev.scalars() == host.scalars()
    for name in ("sl_row", "sl_item0", "child_w", "wpos", "items"):
        a, b = host.array(name), dev.array(name)
        assert len(a) > 0 and a.tobytes() == b.tobytes(), name
    M = len(inp.times)
    u = cases.uniforms(M)
    for kind in cases.KINDS:
        proc, om = cases.models(inp, kind, True, True, nhp=nhp, orc=orc)
        want = oracle_draws(orc, om, inp, u)
        assert same(nhp.resample_parents(proc, dev, u=u), want), kind
        assert same(nhp.resample_parents(proc, host, u=u), want), kind


@pytest.mark.parametrize("kind", cases.KINDS)
def test_error_flag_on_sliced_data(nhp, orc, route, kind):
    """λ0 = 0 and W = 0: no weight sums to a positive value.  k_sampler_slices reports it through the sampler's status word
    (no fault); the next call on the same dataset is judged on its own."""
    inp = INPUTS["A-4096"]
    ds, _ = sliced_dataset(nhp, route, inp)
    N = inp.N
    if kind == "exponential":
        imp = nhp.ExponentialImpulseResponse(np.ones((N, N)), 1.0, 1.0, inp.dt_max)
    else:
        imp = nhp.LogitNormalImpulseResponse(np.zeros((N, N)), np.ones((N, N)), inp.dt_max)
    bad = nhp.ContinuousStandardHawkesProcess(nhp.HomogeneousProcess(np.zeros(N)), imp, nhp.DenseWeightModel(np.zeros((N, N))))
    for cfg in CFGS:
        route({"NHP_SAMPLER_CFG": cfg} if cfg else {})
        with pytest.raises(nhp.DomainError, match="positive finite"):
            nhp.resample_parents(bad, ds, seed=1, step=0)
    route({})
    proc, om = cases.models(inp, kind, False, False, nhp=nhp, orc=orc)
    u = cases.uniforms(len(inp.times))
    assert same(nhp.resample_parents(proc, ds, u=u), oracle_draws(orc, om, inp, u))
