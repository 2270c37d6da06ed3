"""map_parents / cascades without a GPU: the entry points exist, their argument errors come before any device work, the
numpy restatement (tests/cascades_ref.py) is right on forests written out by hand and agrees with the pointer-doubling
recurrence the kernels use, and the generated parity cases have no near-ties (the condition the GPU comparison of the
arg-max rests on)."""
import numpy as np
import pytest

import cascades_ref as cf


def test_entry_points_exist(nhp):
    from nhp_amd import _lib
    lib = _lib.lib()
    for name in ("nhp_cont_map_parents", "nhp_cont_cascades"):
        assert hasattr(lib, name), name
    assert lib.nhp_abi_version() == 2
    assert callable(nhp.map_parents) and callable(nhp.cascades)
    assert nhp.Cascades.FIELDS == ("parents", "root", "generation", "descendants", "cascade_root", "cascade_size", "cascade_depth",
                                   "cascade_end", "immigrants", "offspring", "reach")


@pytest.fixture
def no_device(nhp, monkeypatch):
    """Any step towards the device fails the test."""
    from nhp_amd import _lib, parents

    def refuse(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(_lib, "default_context", refuse)
    monkeypatch.setattr(parents, "device_dataset", refuse)


def test_discrete_process_is_refused(nhp, no_device):
    proc = object.__new__(nhp.DiscreteStandardHawkesProcess)       # refused by its type, before anything is read from it
    data = np.zeros((2, 10), dtype=np.int64)
    for fn in (nhp.map_parents, nhp.cascades):
        with pytest.raises(TypeError, match="ContinuousStandardHawkesProcess.*ContinuousNetworkHawkesProcess"):
            fn(proc, data)


def test_bad_parents_are_refused_before_device_work(nhp, no_device):
    proc = cf.make_process(nhp, "exponential", 3, 1.0)
    data = (np.array([0.1, 0.2, 0.3, 0.4]), np.array([1, 2, 3, 1]), 1.0)
    with pytest.raises(ValueError, match='"map", "sample"'):
        nhp.cascades(proc, data, parents="mode")
    with pytest.raises(ValueError, match="expected length 4"):
        nhp.cascades(proc, data, parents=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="expected length 4"):
        nhp.cascades(proc, data, parents=np.zeros((4, 1), np.int64))
    with pytest.raises(ValueError, match="integers"):
        nhp.cascades(proc, data, parents=np.zeros(4))
    with pytest.raises(ValueError, match="integers"):
        nhp.cascades(proc, data, parents=[0.0, 1.0, 1.0, 2.0])


def _check(f, **want):
    for k, v in want.items():
        np.testing.assert_array_equal(getattr(f, k), np.asarray(v), err_msg=k)


def test_forest_ref_all_immigrants():
    t, n = np.array([1.0, 2.0, 3.0, 4.0]), np.array([2, 1, 2, 2])
    f = cf.forest_ref(np.zeros(4, np.int64), t, n, 3)
    _check(f, root=[1, 2, 3, 4], generation=[0, 0, 0, 0], descendants=[0, 0, 0, 0], cascade_root=[1, 2, 3, 4],
           cascade_size=[1, 1, 1, 1], cascade_depth=[0, 0, 0, 0], cascade_end=t, immigrants=[1, 3, 0], offspring=[0, 0, 0],
           reach=[[1, 0, 0], [0, 3, 0], [0, 0, 0]])


def test_forest_ref_chain():
    t, n = np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([1, 2, 1, 2, 1])
    f = cf.forest_ref(np.arange(5), t, n, 2)
    _check(f, root=[1] * 5, generation=[0, 1, 2, 3, 4], descendants=[4, 3, 2, 1, 0], cascade_root=[1], cascade_size=[5],
           cascade_depth=[4], cascade_end=[5.0], immigrants=[1, 0], offspring=[4 + 2 + 0, 3 + 1], reach=[[3, 2], [0, 0]])


def test_forest_ref_star():
    t, n = np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([2, 1, 1, 2, 1])
    f = cf.forest_ref(np.array([0, 1, 1, 1, 1]), t, n, 2)
    _check(f, root=[1] * 5, generation=[0, 1, 1, 1, 1], descendants=[4, 0, 0, 0, 0], cascade_root=[1], cascade_size=[5],
           cascade_depth=[1], cascade_end=[5.0], immigrants=[0, 1], offspring=[0, 4], reach=[[0, 0], [3, 2]])


def test_forest_ref_two_interleaved_trees():
    # tree A: 1 -> {3, 5}, 3 -> {6};  tree B: 2 -> {4, 7}
    par = np.array([0, 0, 1, 2, 1, 3, 2])
    t = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5])
    n = np.array([1, 2, 2, 3, 1, 3, 2])
    f = cf.forest_ref(par, t, n, 3)
    _check(f, root=[1, 2, 1, 2, 1, 1, 2], generation=[0, 0, 1, 1, 1, 2, 1], descendants=[3, 2, 1, 0, 0, 0, 0],
           cascade_root=[1, 2], cascade_size=[4, 3], cascade_depth=[2, 1], cascade_end=[3.0, 3.5], immigrants=[1, 1, 0],
           offspring=[3, 3, 0], reach=[[2, 1, 1], [0, 2, 1], [0, 0, 0]])
    assert f.reach.sum() == len(par)


def test_forest_ref_refuses_what_is_no_earlier_event():
    t, n = np.array([1.0, 2.0, 3.0]), np.array([1, 1, 1])
    for bad in ([0, 2, 0], [0, -1, 0], [0, 0, 4], [1, 0, 0]):
        with pytest.raises(ValueError, match="earlier event"):
            cf.forest_ref(np.array(bad), t, n, 1)


@pytest.mark.parametrize("M,p", [(3000, 0.3), (3000, 0.01), (1, 0.3), (0, 0.3)])
def test_doubling_recurrence_is_the_forest(M, p):
    par = cf.random_forest(M, seed=11, p_immigrant=p)
    t, n = cf.forest_data(M, 5)
    f = cf.forest_ref(par, t, n, 5)
    root, gen, desc, rounds = cf.doubling_ref(par)
    np.testing.assert_array_equal(root, f.root)
    np.testing.assert_array_equal(gen, f.generation)
    np.testing.assert_array_equal(desc, f.descendants)
    depth = int(gen.max()) if M else 0
    assert rounds == int(np.ceil(np.log2(depth + 1)))
    print(f"M={M} p={p}: depth {depth}, {rounds} rounds")


def test_doubling_recurrence_on_a_chain_and_a_star():
    for par, depth in ((np.arange(1000), 999), (np.r_[0, np.ones(999, np.int64)], 1)):
        t, n = cf.forest_data(1000, 3)
        f = cf.forest_ref(par, t, n, 3)
        root, gen, desc, rounds = cf.doubling_ref(par)
        np.testing.assert_array_equal(root, f.root)
        np.testing.assert_array_equal(gen, f.generation)
        np.testing.assert_array_equal(desc, f.descendants)
        assert rounds == int(np.ceil(np.log2(depth + 1)))


def test_generated_cases_have_no_near_ties_and_sum_to_the_oracle_intensity(nhp, orc):
    for (kind, N), cs in cf.generated_cases(nhp):
        ref, m, M = cs["ref"], cs["model"], len(cs["times"])
        kw = dict(theta=m.theta) if kind == "exponential" else dict(mu=m.mu, tau=m.tau)
        om = orc.ContModel(m.lam0, m.W, dt_max=m.dt_max, **kw)
        want = orc.total_intensity(om, cs["times"], cs["nodes"])
        err = np.max(np.abs(ref.total - want) / want)
        f = cf.forest_ref(ref.parents, cs["times"], cs["nodes"], N)
        print(f"{kind} N={N}: M={M} baseline share {np.mean(ref.parents == 0):.2f} deepest {f.generation.max()} "
              f"largest cascade {f.cascade_size.max()} smallest gap {ref.gap[1:].min():.1e} Σw vs oracle {err:.1e}")
        assert 1000 <= M <= 1800
        assert err <= 1e-12
        assert ref.gap[1:].min() >= 1e-6
        assert np.all(ref.prob > 0.0) and np.all(ref.prob <= 1.0) and ref.prob[0] == 1.0
        assert f.generation.max() >= 5 and np.mean(ref.parents == 0) < 0.7          # the cases exercise the window walk
