"""Every input of tests/test_sampler_slices_gpu.py keeps its child slices and holds what its case is named for -- shown on the
CPU, with the layout rule restated in numpy (tests/slices_ref.py) and the oracle's draws (flags = MATH_DET) for the censuses
of what the scan picks.  The GPU file compares the restated scalars with the dataset's own, so a rule restated wrongly fails
there; what is proved here is that the inputs reach the lines of k_sampler_slices they are meant for."""
import numpy as np
import pytest

import sampler_slices_cases as cases
import slices_ref as sr

INPUTS = cases.inputs()


def lay(name, columns=None):
    inp = INPUTS[name]
    return sr.layout(inp.times, inp.nodes, inp.N, inp.dt_max, inp.chunk, columns=columns)


def test_the_restatement_on_a_hand_made_input():
    # 5 events, Δtmax = 1: windows 0, 1, 2 (a tie is a parent), 0 (exactly Δtmax away: not one), 1
    t = np.array([0.0, 0.5, 0.5, 1.5, 2.0])
    n = np.array([1, 2, 1, 1, 2])
    L = sr.layout(t, n, 2, 1.0)
    assert list(L.window) == [0, 1, 2, 0, 1] and L.pairs == 4 and L.max_window == 2
    assert L.chunk == 32 and L.n_items == 2 and L.max_item == 3
    # node 1: events 0, 2, 3 sorted by window, stably: 2, 0, 3; node 2: events 1, 4 (both 1: time order)
    assert list(L.lane) == [1, 0, 0, 2, 1] and list(L.slice) == [0, 1, 0, 0, 1] and list(L.item) == [0, 1, 0, 0, 1]
    assert list(L.sl_row) == [0, 2, 3] and list(L.sl_item0) == [0, 1, 2] and L.rows_built == 3 and L.max_rows_built == 2
    assert L.kept and L.sl_rows == 3 and L.n_slices == 2 and L.sl_max_rows == 2 and L.sl_nb == 2
    assert sr.item_size(40000, 1024) == 51 and sr.item_size(7000, 9) == 32 and sr.item_size(10 ** 7, 9) == 4096
    assert sr.item_size(7000, 9, 256) == 256 and sr.item_size(7000, 9, 9999) == 4096
    # the keep rule: what the existing tests build with the default items is thrown away (the figure test_cont_grad_edges
    # records for N = 7 is of this kind)
    a = INPUTS["A-256"]
    d = sr.layout(a.times, a.nodes, a.N, a.dt_max)
    assert d.chunk == 32 and not d.kept and d.sl_rows == 0 and d.rows_built * 64 == 476672 and 2 * d.pairs + 4096 == 341676
    # nothing to slice, and an infinite window
    assert not sr.layout(np.arange(4.0), [1, 1, 2, 2], 2, 0.5).kept and not sr.layout(t, n, 2, np.inf).kept
    # a mean window of 192 goes to XCD time parts: refused
    dense = np.sort(np.random.default_rng(0).uniform(0.0, 1.0, 400))
    with pytest.raises(ValueError):
        sr.layout(dense, np.random.default_rng(1).integers(1, 9, 400), 8, 2.0)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_every_input_keeps_its_slices(name):
    L = lay(name)
    assert L.kept and L.sl_rows > 0 and L.n_slices > 0 and L.sl_rows * 64 <= 2 * L.pairs + 4096
    assert L.sl_max_rows == L.max_window                 # (whole datasets: the longest window sits in some slice)
    assert np.all(L.item >= 0) and np.all(L.slice_rows[L.slice] >= L.window)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_planted_uniforms_mean_the_first_parent_and_the_baseline(orc, name):
    """The oracle's own draws for the uniforms the GPU file uses: 0 and the largest double below 1 are there, 0 in front of
    windows that are not empty (where there are any to speak of), and they pick what they stand for."""
    inp, L = INPUTS[name], lay(name)
    u = cases.uniforms(len(inp.times))
    for kind in cases.KINDS:
        for network, lgcp in cases.VARIANTS:
            _, om = cases.models(inp, kind, network, lgcp, orc=orc)
            p, pn = orc.resample_parents(om, inp.times, inp.nodes, u, flags=orc.MATH_DET)
            first, last = cases.check_planted_uniforms(inp, kind, network, L.window, u, p, pn)
            assert (first >= 3 or len(u) < 200) and last >= 1, (first, last)      # (B-1 has 69 events: u = 0 at event 1 only)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_threshold_uniforms_sit_on_the_oracles_thresholds(orc, name):
    """For nearly every child with a parent (every one under a standard exponential model, whose weights are all positive) the
    oracle draws another index for u_at than for the double before it; past the cache too, where there are such windows."""
    inp, L = INPUTS[name], lay(name)
    idx = np.arange(len(inp.times))
    for kind in cases.KINDS:
        for network, lgcp in cases.VARIANTS:
            if name.startswith("D") and (network or (kind == "logitnormal" and name != "D-1024")):
                continue                                                # (not run on the GPU either)
            _, om = cases.models(inp, kind, network, lgcp, orc=orc)
            u_at, u_below, found = cases.thresholds(orc, inp, kind, network, lgcp, L.window)
            pa, _ = orc.resample_parents(om, inp.times, inp.nodes, u_at, flags=orc.MATH_DET)
            pb, _ = orc.resample_parents(om, inp.times, inp.nodes, u_below, flags=orc.MATH_DET)
            ka, kb = np.where(pa > 0, idx - pa, L.window), np.where(pb > 0, idx - pb, L.window)
            assert np.all(ka[found] > kb[found]) and np.array_equal(pa[~found], pb[~found])
            # (a mask takes about half the parents' weights to 0, and a child whose k leading weights are all 0 goes past them
            #  at u = 0 already; a logit-normal pdf is 0 at a delay of 0: most children, not all, have a threshold there)
            share = found.sum() / max(1, np.sum(L.window > 0))
            assert share == 1.0 if (kind == "exponential" and not network) else share > 0.4, (kind, network, share)
            for cache in (8, 16):
                if np.sum(L.window > cache + 1) >= 200:
                    assert np.sum(found & (kb >= cache)) >= 20, (kind, network, cache)


def test_a_has_long_items_short_last_slices_and_windows_past_the_cache():
    big, small = lay("A-4096"), lay("A-256")
    assert (big.pairs, big.n_items, big.n_slices, big.sl_rows * 64) == (168790, 9, 115, 191360)
    assert (small.n_items, small.n_slices) == (34, 135)
    assert big.item_slices.max() > 8                     # more slices than the 8 waves of a 512-thread workgroup
    assert small.item_slices.min() < 4                   # and fewer than the 4 waves of a 256-thread one
    for L in (big, small):
        last = L.sl_item0[1:][L.item_slices > 0] - 1
        assert np.any(L.slice_lanes[last] < 64)
        assert np.any(L.window == 0) and np.sum(L.window >= 33) >= 64
    # the column shards the GPU file builds keep theirs too
    for name in ("A-256", "A-4096"):
        whole = lay(name)
        parts = [lay(name, columns=c) for c in ((0, 3), (3, 9))]
        assert all(p.kept for p in parts) and sum(p.n_items for p in parts) == whole.n_items
        assert sum(p.sl_rows for p in parts) == whole.sl_rows and sum(p.n_slices for p in parts) == whole.n_slices
        node = INPUTS[name].nodes - 1
        assert np.all((parts[0].item >= 0) == (node < 3)) and np.all((parts[1].item >= 0) == (node >= 3))


@pytest.mark.parametrize("k", cases.WALK_K)
def test_b_has_k_k_and_no_slices(k):
    L = lay(f"B-{k}")
    assert list(L.item_slices) == [k, k, 0] and L.n_slices == 2 * k
    assert L.slice_lanes[k - 1] == 5 and np.all(np.delete(L.slice_lanes, k - 1) == 64)


def picks(orc, inp, kind, network, lgcp, u):
    _, om = cases.models(inp, kind, network, lgcp, orc=orc)
    p, _ = orc.resample_parents(om, inp.times, inp.nodes, u, flags=orc.MATH_DET)
    return np.where(p > 0, np.arange(len(p)) - p, -1), p     # weight index k: parent i - 1 - k (0-based) is p = i - k (1-based)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("network,lgcp", cases.VARIANTS)
def test_c_draws_the_weights_around_the_cache_edge(orc, kind, network, lgcp):
    inp, L = INPUTS["C"], lay("C")
    M = len(inp.times)
    for cache in (8, 16):
        for n in (cache - 1, cache, cache + 1):
            assert np.sum(L.window == n) >= 100
    for u in (cases.uniforms(M), orc.uniform_stream(3, 9, M)):
        k, p = picks(orc, inp, kind, network, lgcp, u)
        for cache in (8, 16):
            for q in (cache - 1, cache, cache + 1):
                assert np.sum(k == q) >= 10, (cache, q, int(np.sum(k == q)))
            assert np.sum((p == 0) & (L.window >= cache + 1)) >= 10, cache


def test_c_weights_are_nearly_flat(orc):
    """The census above holds because no weight of a window dwarfs the others: largest / smallest weight of the longest
    windows, and the baseline against their mean."""
    inp = INPUTS["C"]
    lib = orc.lib()
    for kind in cases.KINDS:
        p = cases.flat_parameters(inp, False, False)
        dts = np.linspace(0.03, 0.92, 24)
        if kind == "exponential":
            w = [lib.orc_impulse_exponential(float(p["theta"].max()), float(d), 1) for d in dts]
        else:
            w = [lib.orc_impulse_logitnormal(0.0, 0.5, 1.0, float(d), 1) for d in dts]
        assert max(w) / min(w) < 2.5 and 0.3 < 1.0 / np.mean(w) < 3.0, (kind, w)


@pytest.mark.parametrize("B", cases.BURSTS)
def test_d_puts_the_longest_window_on_either_side_of_the_threshold(B):
    L = lay(f"D-{B}")
    assert L.kept and L.sl_max_rows == B - 1 and L.max_window == B - 1
    # sl_max_rows + 1 weights with the baseline: 1024 is the most the slice kernel sums in sequence
    assert (L.sl_max_rows + 1 > 1024) == (B == 1025)


def test_e_is_far_from_the_origin_with_ties():
    inp, L = INPUTS["E"], lay("E")
    assert inp.times[0] > 5e5 and np.sum(np.diff(inp.times) == 0.0) >= 10
    assert np.spacing(inp.times[0]) > 2.0 ** -35         # a delay computed from these times has lost 19 bits
    assert L.item_slices.max() > 8


@pytest.mark.parametrize("name,share", [("F-9", 0.10), ("F-9-short", 0.25), ("F-1", 0.01), ("F-1-short", 0.25)])
def test_f_has_childless_windows_in_slices_with_rows(name, share):
    """Children are sorted by window length, so the parentless ones of an item share at most one slice with the others: those
    lanes walk rows that are all padding; the slices after it have no rows at all.  The two shapes test_derived_layouts uses
    (mean windows of 2 and 4.4) leave 13 % and 1.3 % of the children without a parent; the short twins more than a quarter."""
    L = lay(name)
    empty = L.window == 0
    assert np.mean(empty) > share, np.mean(empty)
    assert np.sum(empty & (L.slice_rows[L.slice] > 0)) >= 10
    if name.endswith("short") or name == "F-9":
        assert np.sum(L.slice_rows == 0) >= 1 and np.sum(L.slice_rows > 0) >= 1
    if name.startswith("F-9"):
        assert 0 in L.item_slices                        # the node without events
