"""CPU: the recycling of solve()'s page-locked output blocks
(ffddp.solver._RecycledPinned) with a stand-in allocator in place of
ffddp_host_alloc / ffddp_host_free (no GPU needed): fresh arrays while the
caller holds earlier ones, the block reused once they are gone, the
page-locked cap, and the frees at close."""
from __future__ import annotations

import ctypes as C
import gc
import threading

import numpy as np
import pytest

from ffddp import solver as S


class _FakeLib:
    def __init__(self):
        self.live = {}
        self.allocs = 0
        self.frees = 0

    def ffddp_host_alloc(self, n, pp):
        buf = C.create_string_buffer(int(n))
        self.live[C.addressof(buf)] = buf
        pp._obj.value = C.addressof(buf)
        self.allocs += 1
        return 0

    def ffddp_host_free(self, p):
        self.live.pop(p.value)
        self.frees += 1
        return 0


@pytest.fixture
def fake(monkeypatch):
    lib = _FakeLib()
    monkeypatch.setattr(S._abi, "load", lambda: lib)
    return lib


SPECS = dict(xs=((4, 3, 2), np.float64), it=((4,), np.int32), ok=((4,), np.uint8))


def test_fresh_while_held_and_reused_after_release(fake):
    pool = S._RecycledPinned(cap=10 ** 6)
    a = pool.arrays(SPECS)
    a["xs"][...] = 1.0
    b = pool.arrays(SPECS)  # a is still held: another block
    assert not np.shares_memory(a["xs"], b["xs"]) and fake.allocs == 2
    addr = a["xs"].ctypes.data
    del a
    c = pool.arrays(SPECS)  # a's block comes back, no new allocation
    assert c["xs"].ctypes.data == addr and fake.allocs == 2
    assert c["xs"].shape == (4, 3, 2) and c["it"].dtype == np.int32 and c["ok"].dtype == np.uint8
    pool.close()
    assert fake.frees == 0  # both blocks are still viewed by b and c
    del b, c
    assert fake.frees == 2 and not fake.live


def test_cap_falls_back(fake):
    pool = S._RecycledPinned(cap=256)  # one block of these specs (3 fields x 256 B) does not fit
    assert pool.arrays(SPECS) is None and fake.allocs == 0
    pool = S._RecycledPinned(cap=768)
    first = pool.arrays(SPECS)
    assert first is not None
    assert pool.arrays(SPECS) is None  # the second would exceed the cap
    pool.close()
    del first
    assert fake.frees == 1 and not fake.live


def test_views_keep_the_block(fake):
    pool = S._RecycledPinned(cap=10 ** 6)
    a = pool.arrays(SPECS)
    view = a["xs"][1:]
    addr = a["xs"].ctypes.data
    del a
    b = pool.arrays(SPECS)  # the view still holds the first block
    assert b["xs"].ctypes.data != addr
    del view
    c = pool.arrays(SPECS)
    assert c["xs"].ctypes.data == addr
    pool.close()


class _GcWhileLocked:
    """Stand-in for the pool's lock: the cyclic collector is enabled exactly
    while the lock is held, so a pending cycle is collected at the first
    allocation inside a locked region, not somewhere before it."""

    def __init__(self):
        self._lock = threading.Lock()

    def __enter__(self):
        self._lock.acquire()
        gc.enable()

    def __exit__(self, *exc):
        gc.disable()
        self._lock.release()


def test_finalizer_inside_a_locked_region_does_not_deadlock(fake):
    """A block whose arrays sit in an unreachable reference cycle is given back
    by a cyclic GC pass, which starts at any container allocation, also one
    made while the pool's lock is held by the same thread (give-back of
    another block, close()).  Neither may block, and every block is freed
    once."""
    was_enabled, thresholds = gc.isenabled(), gc.get_threshold()
    gc.disable()
    try:
        pool = S._RecycledPinned(cap=10 ** 6)
        pool.lock = _GcWhileLocked()
        a = pool.arrays(SPECS)
        b = pool.arrays(SPECS)
        assert fake.allocs == 2
        cycle = [a]
        cycle.append(cycle)
        del a, cycle  # block 1: unreachable, pending until a GC pass
        held = [b]
        del b
        gc.set_threshold(1, 1, 1)
        # daemon threads: a deadlock fails the joins below instead of hanging the suite
        drop = threading.Thread(target=held.clear, daemon=True)  # the last reference to block 2
        drop.start()
        drop.join(5.0)
        close = threading.Thread(target=pool.close, daemon=True)
        close.start()
        close.join(5.0)
        assert not drop.is_alive() and not close.is_alive()
        gc.collect()  # block 1's cycle, had no pass collected it yet
        assert fake.frees == 2 and not fake.live
    finally:
        gc.set_threshold(*thresholds)
        if was_enabled:
            gc.enable()
        else:
            gc.disable()
