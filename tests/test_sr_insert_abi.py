"""kad_sr_insert's entry points: symbols, constants and signatures; the argument checks that need no
real handle run without a GPU (a zeroed buffer stands in for a set of no searches), and on the GPU every refusal
documented in include/kadgpu.h answers in its order and leaves the set as exported before, the slab limit of 64 entries
included."""
import ctypes as C
import os

import numpy as np
import pytest

import insert_ref as I
import opendht_amd
from opendht_amd import DeviceSearches, KadError, _lib

INVALID, UNSUPPORTED = _lib.KAD_ERR_INVALID, _lib.KAD_ERR_UNSUPPORTED
CONSTANTS = {"KAD_SR_INSERT_OK": 0, "KAD_SR_INSERT_OVERFLOW": 1}
p = _lib.ptr


def test_symbols_constants_and_signatures():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n, nargs in (("kad_sr_insert", 8), ("kad_sr_insert_kernel_ms", 2)):
        assert hasattr(L, n) and f"int {n}(" in hdr
        assert _lib.SIGNATURES[n][0] is C.c_int and len(_lib.SIGNATURES[n][1]) == nargs
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert f"#define {name} {val}u" in hdr, name
    assert I.INSERT_OVERFLOW == _lib.KAD_SR_INSERT_OVERFLOW and I.SN_BAD == _lib.KAD_SN_BAD
    assert callable(opendht_amd.try_search_insert_device) and callable(opendht_amd.plan_insert_round)
    assert callable(opendht_amd.DeviceSearches.insert) and callable(opendht_amd.DeviceSearches.insert_kernel_ms)


def test_null_and_order_checks_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)  # a set of no searches
    which, off = np.array([0], np.uint32), np.array([0, 1], np.uint32)
    ids, fl = np.zeros((1, 20), np.uint8), np.zeros(1, np.uint8)
    ins, st = np.full(1, 0xAA, np.uint8), np.full(1, 0xAA, np.uint8)
    for m in (1, 0):
        assert L.kad_sr_insert(None, m, p(which), p(off), p(ids), p(fl), p(ins), p(st)) == INVALID
        assert b"NULL" in L.kad_last_error()
    for args in ((None, p(off), p(ids), p(fl), p(ins), p(st)), (p(which), None, p(ids), p(fl), p(ins), p(st)),
                 (p(which), p(off), p(ids), p(fl), p(ins), None), (p(which), p(off), None, p(fl), p(ins), p(st)),
                 (p(which), p(off), p(ids), p(fl), None, p(st))):
        assert L.kad_sr_insert(p(fake), 1, *args) == INVALID
        assert b"NULL" in L.kad_last_error()
    # a set of no searches: every index is out of range; NULL flags are allowed
    assert L.kad_sr_insert(p(fake), 1, p(which), p(off), p(ids), None, p(ins), p(st)) == INVALID
    assert b"strictly ascending and below S" in L.kad_last_error()
    # no candidates: the candidate arrays may be NULL, and `which` is still checked
    assert L.kad_sr_insert(p(fake), 1, p(which), p(np.zeros(2, np.uint32)), None, None, None, p(st)) == INVALID
    assert b"strictly ascending and below S" in L.kad_last_error()
    assert L.kad_sr_insert(p(fake), 0, None, None, None, None, None, None) == 0
    assert L.kad_sr_insert_kernel_ms(None, C.byref(C.c_float())) == INVALID
    assert L.kad_sr_insert_kernel_ms(p(fake), None) == INVALID
    ms = C.c_float(1.0)
    assert L.kad_sr_insert_kernel_ms(p(fake), C.byref(ms)) == 0 and ms.value == 0.0
    assert (ins == 0xAA).all() and (st == 0xAA).all()


def _export_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_refusals_in_order_leave_the_set(gpu):
    L = _lib.lib()
    c = I.case("s65_cap14")
    S = len(c["searches"])
    off_all = I.csr(c["lists"])[0]
    took = [k for k in range(S) if c["status"][k] == I.INSERT_OK and c["ins"][off_all[k]:off_all[k + 1]].any()]
    good = np.array(took[:3], np.uint32)  # three searches an insert changes (which = all: position = index)
    lists = [c["lists"][int(s)] for s in good]
    off, ids, fl = I.csr(lists)
    T = int(off[-1])
    ins, st = np.zeros(T, np.uint8), np.zeros(3, np.uint8)
    with DeviceSearches(*I.snapshot(c["searches"]), cap=c["cap"], device=0) as DS:
        before = DS.export()

        def call(ss, m, w, o=off, i=ids, f=fl, r=ins, s=st):
            return L.kad_sr_insert(ss, m, p(w), p(o), p(i), p(f), p(r), p(s))

        unsorted = good[[1, 0, 2]].copy()
        bad_off = off.copy()
        bad_off[1], bad_off[2] = off[2], off[1]
        bad_fl = fl.copy()
        bad_fl[-1] = 2
        # NULL handle first, even with a bad list
        assert call(None, 3, unsorted) == INVALID and b"NULL" in L.kad_last_error()
        # NULL arrays before the order of `which`
        assert call(DS._h, 3, None) == INVALID and b"NULL" in L.kad_last_error()
        assert call(DS._h, 3, unsorted, o=None) == INVALID and b"NULL" in L.kad_last_error()
        assert call(DS._h, 3, unsorted, s=None) == INVALID and b"NULL" in L.kad_last_error()
        assert call(DS._h, 3, unsorted, i=None) == INVALID and b"NULL" in L.kad_last_error()
        assert call(DS._h, 3, unsorted, r=None) == INVALID and b"NULL" in L.kad_last_error()
        # `which` before the offsets: descending, repeated, out of range
        for w in (unsorted, good[[0, 0, 2]].copy(), np.array([good[0], good[1], S], np.uint32)):
            assert call(DS._h, 3, w, o=bad_off, f=bad_fl) == INVALID
            assert b"strictly ascending and below S" in L.kad_last_error()
        # the offsets before the flags: not starting at 0, descending, too many
        for o in (off + np.uint32(1), bad_off, np.array([0, 1, 2, 0x7FFFFFFF], np.uint32)):
            assert call(DS._h, 3, good, o=o, f=bad_fl if o is not None and int(o[-1]) <= T else None) == INVALID
            assert b"offsets" in L.kad_last_error() or b"too many" in L.kad_last_error()
        # a flag byte with another bit
        assert call(DS._h, 3, good, f=bad_fl) == INVALID and b"KAD_SN_BAD" in L.kad_last_error()
        # m == 0 is OK with anything behind it
        assert call(DS._h, 0, good) == 0 and L.kad_sr_insert(DS._h, 0, None, None, None, None, None, None) == 0
        assert _export_equal(before, DS.export())
        assert (ins == 0).all() and (st == 0).all()
        assert call(DS._h, 3, good) == 0
        k = np.concatenate([np.arange(off_all[int(s)], off_all[int(s) + 1]) for s in good]).astype(np.int64)
        assert np.array_equal(ins, c["ins"][k]) and np.array_equal(st, c["status"][good])
        assert not _export_equal(before, DS.export())


@pytest.mark.gpu
def test_slabs_of_more_than_64_entries_are_unsupported(gpu):
    """The insert kernel holds one list entry per lane: cap 64 works (test_sr_insert.py), cap 65 answers
    KAD_ERR_UNSUPPORTED after every other check and leaves the set; m == 0 is still KAD_OK."""
    c = I.case("s3_cap64")
    off, ids, fl = I.csr(c["lists"])
    with DeviceSearches(*I.snapshot(c["searches"]), cap=65, device=0) as DS:
        before = DS.export()
        with pytest.raises(KadError) as e:
            DS.insert(c["which"], off, ids, fl)
        assert e.value.code == UNSUPPORTED
        with pytest.raises(KadError) as e:  # the order of `which` is checked first
            DS.insert(c["which"][::-1].copy(), off, ids, fl)
        assert e.value.code == INVALID
        ins, st = DS.insert(np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros((0, 20), np.uint8))
        assert ins.size == 0 and st.size == 0
        assert _export_equal(before, DS.export())
