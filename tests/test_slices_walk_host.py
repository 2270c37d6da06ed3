"""How an item's child slices are dealt to the waves of its workgroup (csrc/nhp_internal.h: nhp_slice_of, snake order),
through the library's own function (nhp_debug_slice_of), without a GPU.  The kernels walk `j = slice_of(0, w)`, then
`slice_of(1, w)`, ... while j < ns: what that loop visits is restated here wave by wave."""
import ctypes as C

import numpy as np
import pytest

NWS = (1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def slice_of(nhp):
    from nhp_amd import _lib
    fn = _lib.lib().nhp_debug_slice_of
    fn.restype = C.c_int32
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    return fn


def visits(slice_of, w, nw, ns):
    """The slices wave w takes from an item of ns slices: the kernels' `while (j < ns)`."""
    out, r = [], 0
    j = slice_of(0, w, nw)
    while j < ns:
        out.append(j)
        r += 1
        j = slice_of(r, w, nw)
    return out


@pytest.mark.parametrize("nw", NWS)
def test_every_slice_once(slice_of, nw):
    for ns in range(0, 5 * nw + 2):
        seen = [j for w in range(nw) for j in visits(slice_of, w, nw, ns)]
        assert sorted(seen) == list(range(ns)), (nw, ns, seen)


@pytest.mark.parametrize("nw", NWS)
def test_round_zero_is_the_identity(slice_of, nw):
    # the kernels' heads request the rows of slice `w` before the column is staged
    assert [slice_of(0, w, nw) for w in range(nw)] == list(range(nw))


@pytest.mark.parametrize("nw", NWS)
def test_a_wave_never_returns_once_it_is_past_the_last_slice(slice_of, nw):
    # the loop stops at the first j >= ns: every later slice of that wave must lie past the end too, for every ns
    for w in range(nw):
        js = [slice_of(r, w, nw) for r in range(8)]
        assert all(b > a for a, b in zip(js, js[1:])), (nw, w, js)
        assert all(r * nw <= j < (r + 1) * nw for r, j in enumerate(js)), (nw, w, js)


@pytest.mark.parametrize("nw", NWS)
def test_longest_wave_is_never_longer_than_under_forward_dealing(slice_of, nw):
    """Children are sorted longest window first, so rows per slice fall with j.  Forward dealing (j = w, w + nw, ...) gives
    wave 0 the longest slice of every round; under the snake the longest wave carries at most as many rows."""
    rng = np.random.default_rng(12)
    profiles = [lambda ns: np.arange(ns, 0, -1), lambda ns: np.full(ns, 7), lambda ns: np.r_[np.full(ns // 2, 90), np.ones(ns - ns // 2)],
                lambda ns: np.sort(rng.integers(0, 200, ns))[::-1], lambda ns: np.sort(rng.geometric(0.1, ns))[::-1]]
    strictly = 0
    for ns in range(0, 5 * nw + 2):
        for make in profiles:
            rows = np.asarray(make(ns), dtype=np.int64)
            assert np.all(np.diff(rows) <= 0)
            snake = max(int(rows[visits(slice_of, w, nw, ns)].sum()) for w in range(nw))
            forward = max(int(rows[w::nw].sum()) for w in range(nw))
            assert snake <= forward, (nw, ns, rows, snake, forward)
            strictly += snake < forward
    assert strictly > 0 or nw == 1                  # (one wave takes everything either way)
