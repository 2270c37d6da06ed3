"""tests/slices_ref.time_parts, the XCD time-part layout restated from its rule, held to the properties that make it a
partition -- on the inputs tests/test_time_parts_gpu.py runs the kernels on, so that what the dataset exports can be compared
with it entry for entry there.  No GPU.

On every case: each child lies in exactly one item of its own node; a node's items are contiguous, in time order and cut at
the event indices M·s/TP; each real node has exactly one item with `first & 1` (its s = 0 item) and none with bit 1; the
padding items are empty, not first, name node N - 1 and number ceil(N/(8/TP))·8 - N·TP; item b of a run of 8 sits on XCD
b % 8 = s·(8/TP) + c % (8/TP)."""
import functools

import numpy as np
import pytest

import cascades_ref as cf
import compensator_ref
import cont_grad_ref as cr
import slices_ref as sr

MAP_CASES = ("P4-exp", "P4-logit", "P4-net", "P2-exp")

EXPECT = {"P4-exp": (4, 40, 4), "P4-logit": (4, 40, 4), "P4-net": (4, 40, 4), "P2-exp": (2, 24, 4), "P2-logit": (2, 24, 4),
          "P2-inf": (2, 24, 4), "large": (4, 32, 0), "P4-exp XCD=8": (8, 72, 0)}
"""(TP, items, padding items) of every case."""


def data_of(name):
    if name == "large":
        t, n, T, N, dt_max = cr.large_item_data()
        return t, n, N, dt_max, None
    case = cr.prepared(name.split(" ")[0])[0]
    return case["times"], case["nodes"], case["N"], case["dt_max"], (8 if name.endswith("XCD=8") else None)


@functools.lru_cache(maxsize=None)
def map_reference(name):
    """(case, cascades_ref.MapRef) of a time-part case: the most likely parents, computed once."""
    case = cr.prepared(name)[0]
    expo = case["kind"] == "exponential"
    m = compensator_ref.Model(case["lam0"], case["W"], case["dt_max"], theta=case["theta"] if expo else None,
                              mu=None if expo else case["mu"], tau=None if expo else case["tau"], A=case["A"])
    return case, cf.map_parents_ref(m, case["times"], case["nodes"])


def split(items, N, TP):
    """(real items, padding items): a run of 8 items holds 8/TP nodes; the slots of nodes >= N are the padding."""
    per_run = 8 // TP
    b = np.arange(len(items))
    c = (b // 8) * per_run + (b % 8) % per_run
    return items[c < N], items[c >= N], c


@pytest.mark.parametrize("name", list(EXPECT))
def test_time_parts_are_a_partition(name):
    t, nodes, N, dt_max, parts = data_of(name)
    M = len(t)
    TP, items = sr.time_parts(t, nodes, N, dt_max, parts=parts)
    want_tp, want_items, want_pad = EXPECT[name]
    assert (TP, len(items)) == (want_tp, want_items)
    assert len(items) == -(-N // (8 // TP)) * 8
    real, pad, slot_node = split(items, N, TP)
    # padding: empty, not first, on node N - 1, as many as the last run has slots left
    assert len(pad) == want_pad == -(-N // (8 // TP)) * 8 - N * TP
    assert np.all(pad[:, 1] == pad[:, 2]) and np.all(pad[:, 3] == 0) and np.all(pad[:, 0] == N - 1)
    # the XCD of an item: time part s of the nodes with c % (8/TP) == g runs on XCD s·(8/TP) + g
    b = np.arange(len(items))
    s_of = (b % 8) // (8 // TP)
    assert np.array_equal(items[slot_node < N, 0], slot_node[slot_node < N])
    assert np.array_equal((b % 8), s_of * (8 // TP) + slot_node % (8 // TP))
    # the children in node order, time order inside a node: position k holds event order[k]
    n0 = np.asarray(nodes, dtype=np.int64) - 1
    order = np.argsort(n0, kind="stable")
    covered = np.zeros(M, dtype=np.int64)
    for c in range(N):
        mine = real[real[:, 0] == c]
        s_mine = s_of[slot_node == c]
        assert len(mine) == TP and np.array_equal(s_mine, np.arange(TP))           # in time order in the table
        assert (mine[:, 3] & 1).sum() == 1 and mine[0, 3] == 1 and np.all(mine[1:, 3] == 0)
        assert np.all((mine[:, 3] & 2) == 0)
        assert np.array_equal(mine[1:, 1], mine[:-1, 2])                            # contiguous
        assert mine[0, 1] == (n0 < c).sum() and mine[-1, 2] == (n0 <= c).sum()     # from the node's first child to its last
        for s, (_, kb, ke, _) in enumerate(mine):
            ev = order[kb:ke]
            assert np.all(n0[ev] == c) and np.all((ev >= M * s // TP) & (ev < M * (s + 1) // TP))
            covered[ev] += 1
    assert np.all(covered == 1)
    assert int((items[:, 2] - items[:, 1]).max()) > (4096 if name == "large" else 0)


@pytest.mark.parametrize("name", cr.TIME_PART_CASES)
def test_small_cases_have_an_empty_first_item_and_a_padded_last_node(name):
    case = cr.prepared(name)[0]
    N = case["N"]
    TP, items = sr.time_parts(case["times"], case["nodes"], N, case["dt_max"])
    real, pad, _ = split(items, N, TP)
    late = real[real[:, 0] == N - 2]                                     # node N-1 (1-based): 40 events in the last quarter
    assert late[0, 3] == 1 and late[0, 1] == late[0, 2] and (late[:, 2] - late[:, 1]).sum() == 40
    assert np.all(late[:TP * 3 // 4, 1] == late[:TP * 3 // 4, 2])
    last = real[real[:, 0] == N - 1]                                     # node N: no event, TP empty items, the first one `first`
    assert np.all(last[:, 1] == last[:, 2]) and last[:, 3].tolist() == [1] + [0] * (TP - 1)
    assert len(pad) >= 1 and np.all(pad[:, 0] == N - 1)
    single = real[real[:, 0] == N - 3]
    assert (single[:, 2] - single[:, 1]).sum() == 1


def test_column_shards_keep_their_own_items():
    case = cr.prepared("P4-exp")[0]
    N = case["N"]
    args = (case["times"], case["nodes"], N, case["dt_max"])
    TP, whole = sr.time_parts(*args)
    shards = [sr.time_parts(*args, columns=cols)[1] for cols in ((0, 4), (4, 9))]
    assert sorted(map(tuple, np.concatenate(shards))) == sorted(map(tuple, whole))
    assert np.all(shards[0][:, 0] < 4) and np.all(shards[1][:, 0] >= 4)
    TP1, only = sr.time_parts(*args, columns=(8, 9))                     # the empty node: its four items and the padding
    assert TP1 == TP == 4 and len(only) == 8 and np.all(only[:, 1] == only[:, 2]) and only[:, 3].sum() == 1


def test_the_rule_gives_no_time_parts_elsewhere():
    for name in ("W-exp", "D", "L-exp"):                                # N = 7, 3, 2: below N = 8
        case = cr.prepared(name)[0]
        assert sr.time_parts(case["times"], case["nodes"], case["N"], case["dt_max"]) is None
    case = cr.prepared("P4-exp")[0]
    t, n = case["times"], case["nodes"]
    assert sr.time_parts(t[:143], n[:143], 9, 1.0) is None             # M < 16·N
    assert sr.time_parts(t, n, 9, 2.0 ** -6) is None                    # short windows: sliced, a mean window below 24
    assert sr.time_part_count(161 * 1000, 1000, 9, 1.0) == 2 and sr.time_part_count(160 * 1000, 1000, 9, 1.0) == 0
    assert sr.time_part_count(192 * 1000, 1000, 9, 1.0) == 4 and sr.time_part_count(24 * 1000, 1000, 9, np.inf) == 2
    with pytest.raises(ValueError):                                      # layout() keeps refusing what goes to time parts
        sr.layout(t, n, 9, 1.0)


@pytest.mark.parametrize("name", MAP_CASES)
def test_most_likely_parents_have_no_near_ties(name):
    """The condition the GPU comparison of the arg-max rests on (tests/test_cascades_host.py): no event whose two largest
    category weights lie within 1e-6 relative -- the planted ties of the times are on different nodes for this."""
    case, ref = map_reference(name)
    gap = float(ref.gap[1:].min())
    print(f"{name}: baseline share {np.mean(ref.parents == 0):.2f}, smallest gap {gap:.1e}")
    assert gap >= 1e-6 and np.all(ref.prob > 0.0) and np.all(ref.prob <= 1.0) and ref.prob[0] == 1.0
    assert 0.02 < np.mean(ref.parents == 0) < 0.98                      # parents and the baseline both win somewhere
