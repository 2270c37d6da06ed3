"""Which result slots owe a deferred sum (csrc/nhp_internal.h: nhp_pending), through the library's own bookkeeping
(nhp_debug_pending_*), without a GPU: an enqueue marks its slot with the number of partial pairs and the workgroup size of its
launch, a launch that writes the slot's value itself clears the mark, and the join drains every slot still marked."""
import ctypes as C

import pytest


class Pending:
    def __init__(self, lib, slots):
        self.lib, self.S = lib, slots
        self.h = lib.nhp_debug_pending_new()
        assert self.h

    def mark(self, slot, n, block=512):
        return self.lib.nhp_debug_pending_mark(self.h, slot, n, block)

    def clear(self, slot):
        return self.lib.nhp_debug_pending_clear(self.h, slot)

    def drain(self):
        a, b, c = ((C.c_int32 * self.S)() for _ in range(3))
        n = self.lib.nhp_debug_pending_drain(self.h, a, b, c)
        assert 0 <= n <= self.S
        return [(a[i], b[i], c[i]) for i in range(n)]

    def free(self):
        self.lib.nhp_debug_pending_free(self.h)


@pytest.fixture
def pending(nhp):
    from nhp_amd import _lib
    lib = _lib.lib()
    i32, vp = C.c_int32, C.c_void_p
    ip = C.POINTER(C.c_int32)
    lib.nhp_debug_pending_new.restype, lib.nhp_debug_pending_new.argtypes = vp, []
    lib.nhp_debug_pending_free.restype, lib.nhp_debug_pending_free.argtypes = None, [vp]
    lib.nhp_debug_pending_mark.restype, lib.nhp_debug_pending_mark.argtypes = i32, [vp, i32, i32, i32]
    lib.nhp_debug_pending_clear.restype, lib.nhp_debug_pending_clear.argtypes = i32, [vp, i32]
    lib.nhp_debug_pending_drain.restype, lib.nhp_debug_pending_drain.argtypes = i32, [vp, ip, ip, ip]
    p = Pending(lib, _lib.MAX_SLOTS)
    yield p
    p.free()


def test_nothing_marked_nothing_drained(pending):
    assert pending.drain() == []
    assert pending.clear(5) == 0
    assert pending.drain() == []


def test_mark_and_drain_in_order_of_first_mark(pending):
    for slot, n, block in ((7, 1024, 512), (0, 3, 64), (4095, 2, 256)):
        assert pending.mark(slot, n, block) == 0
    assert pending.drain() == [(7, 1024, 512), (0, 3, 64), (4095, 2, 256)]
    assert pending.drain() == []                        # the join leaves none marked


def test_the_later_launch_into_a_slot_replaces_the_earlier(pending):
    pending.mark(3, 1024, 512)
    pending.mark(4, 8, 128)
    pending.mark(3, 3, 64)                              # another dataset into the same slot
    assert pending.drain() == [(3, 3, 64), (4, 8, 128)]


def test_clear_on_overwrite(pending):
    pending.mark(1, 10)
    pending.mark(2, 20)
    pending.clear(1)                                    # a launch that writes slot 1 itself
    assert pending.drain() == [(2, 20, 512)]
    pending.mark(1, 10)
    pending.clear(1)
    pending.mark(1, 30)                                 # ... and a deferred one after it: listed once
    assert pending.drain() == [(1, 30, 512)]
    pending.clear(1)
    assert pending.drain() == []


def test_every_slot(pending):
    S = pending.S
    for s in range(S):
        pending.mark(s, s + 1)
    for s in range(0, S, 2):
        pending.clear(s)
    assert pending.drain() == [(s, s + 1, 512) for s in range(1, S, 2)]
    for s in reversed(range(S)):                        # the marks of the drained round are gone
        pending.mark(s, 2)
    assert pending.drain() == [(s, 2, 512) for s in reversed(range(S))]


def test_arguments_out_of_range(pending):
    S = pending.S
    assert pending.mark(-1, 4) == -1 and pending.mark(S, 4) == -1 and pending.mark(0, 0) == -1
    assert pending.clear(-1) == -1 and pending.clear(S) == -1
    assert pending.drain() == []
