"""kad_sr_try_insert_tick's and kad_sr_plan_round's entry points: symbols, constants and signatures,
and every argument check documented in include/kadgpu.h in its order, against a zeroed buffer standing in for a set of no
searches. CPU only; the checks that need a real set (the slab limit) are in test_sr_tick.py."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

INVALID = _lib.KAD_ERR_INVALID
CONSTANTS = {"KAD_SR_TICK_LEFT": 0, "KAD_SR_TICK_SKIPPED": 1, "KAD_SR_TICK_APPLIED": 2, "KAD_SR_PLAN_SKIPPED": 0,
             "KAD_SR_PLAN_READY": 1, "KAD_SR_PLAN_DEFERRED": 2}
p = _lib.ptr


def test_symbols_constants_and_signatures():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n, nargs in (("kad_sr_try_insert_tick", 15), ("kad_sr_plan_round", 12)):
        assert hasattr(L, n) and f"int {n}(" in hdr
        assert _lib.SIGNATURES[n][0] is C.c_int and len(_lib.SIGNATURES[n][1]) == nargs
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert f"#define {name} {val}u" in hdr, name
    assert "} kad_sr_tick_stats;" in hdr and C.sizeof(_lib.sr_tick_stats) == 32
    assert callable(opendht_amd.try_search_insert_tick) and callable(opendht_amd.plan_round)
    assert callable(opendht_amd.DeviceSearches.try_insert_tick)


def outputs(q):
    return [np.full(q, 0xAA, np.uint8), np.full(q, 0xAAAAAAAA, np.uint32), np.full(q, 0xAAAAAAAA, np.uint32),
            np.full(q, 0xAAAAAAAA, np.uint32), np.full(q, 0xAAAAAAAA, np.uint32), np.full(q, 0xAA, np.uint8),
            np.full(q, 0xAA, np.uint8)]


def test_argument_checks_in_order_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)  # a set of no searches
    q = 3
    ids, fl = np.zeros((q, 20), np.uint8), np.zeros(q, np.uint8)
    bad_fl = np.array([0, 1, 2], np.uint8)
    outs = outputs(q)
    over, n_over = np.full(4, 0xAAAAAAAA, np.uint32), C.c_uint32(77)
    st = _lib.sr_tick_stats()

    def call(ss, i=ids, f=fl, n=q, o=None, ov=over, nov=C.byref(n_over), stats=C.byref(st)):
        o = outs if o is None else o
        return L.kad_sr_try_insert_tick(ss, p(i), p(f), n, 0, *[p(a) for a in o], p(ov), nov, stats)

    untouched = lambda: all((a == a.dtype.type(0xAAAAAAAA >> (32 - 8 * a.itemsize))).all() for a in outs + [over])
    # 1. NULL ss first, whatever else is wrong
    assert call(None, i=None, f=bad_fl, ov=None) == INVALID and b"NULL search set" in L.kad_last_error()
    # 2. NULL cand_ids or any per-candidate output with q > 0, before the overflow outputs and the flags
    assert call(p(fake), i=None, f=bad_fl, ov=None) == INVALID and b"NULL candidate or output" in L.kad_last_error()
    for k in range(7):
        o = list(outs)
        o[k] = None
        assert call(p(fake), o=o, f=bad_fl, nov=None) == INVALID and b"NULL candidate or output" in L.kad_last_error()
    # 3. NULL out_overflow / out_n_overflow, before the flags
    assert call(p(fake), f=bad_fl, ov=None) == INVALID and b"NULL overflow" in L.kad_last_error()
    assert call(p(fake), f=bad_fl, nov=None) == INVALID and b"NULL overflow" in L.kad_last_error()
    assert call(p(fake), n=0, i=None, o=[None] * 7, ov=None) == INVALID and b"NULL overflow" in L.kad_last_error()
    # 4. a flag byte with another bit, before the empty set answers
    assert call(p(fake), f=bad_fl) == INVALID and b"KAD_SN_BAD" in L.kad_last_error()
    assert untouched() and n_over.value == 77
    # 5. S == 0: every candidate SKIPPED with a zero verdict; NULL flags and NULL stats are allowed
    for f, stats in ((fl, C.byref(st)), (None, None), (np.array([1, 0, 1], np.uint8), C.byref(st))):
        for a in outs:
            a[:] = a.dtype.type(0xAAAAAAAA >> (32 - 8 * a.itemsize))
        n_over.value = 77
        assert call(p(fake), f=f, stats=stats) == 0
        assert (outs[0] == _lib.KAD_SR_TICK_SKIPPED).all() and all(not a.any() for a in outs[1:])
        assert n_over.value == 0
    assert (st.rounds, st.skipped, st.applied, st.left, st.pairs, st.overflowed) == (0, q, 0, 0, 0, 0)
    assert st.verdict_ms == 0.0 and st.insert_ms == 0.0
    # q == 0: the candidate arrays may be NULL
    assert call(p(fake), n=0, i=None, f=None, o=[None] * 7) == 0 and n_over.value == 0 and st.skipped == 0
    assert (over == 0xAAAAAAAA).all()


def test_plan_round_null_checks():
    L = _lib.lib()
    a32, a8, n = np.zeros(2, np.uint32), np.zeros(2, np.uint8), C.c_uint32(5)
    assert L.kad_sr_plan_round(4, 2, p(a32), p(a32), p(a32), p(a8), p(a8), p(a8), p(a32), p(a32), p(a8), None) == INVALID
    assert L.kad_sr_plan_round(4, 2, None, p(a32), p(a32), p(a8), p(a8), p(a8), p(a32), p(a32), p(a8), C.byref(n)) == INVALID
    assert L.kad_sr_plan_round(4, 2, p(a32), p(a32), p(a32), p(a8), p(a8), p(a8), None, p(a32), p(a8), C.byref(n)) == INVALID
    assert L.kad_sr_plan_round(4, 0, None, None, None, None, None, None, None, None, None, C.byref(n)) == 0 and n.value == 0
