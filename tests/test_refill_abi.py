"""kad_sr_refill's entry points: symbols, constants and signatures; the argument checks that need
no real handle run without a GPU (a zeroed buffer stands in for a set of no searches and is never dereferenced as a
table), and on the GPU every refusal documented in include/kadgpu.h answers in its order and leaves the set as
exported before, the slab limit of 64 entries included."""
import ctypes as C
import os

import numpy as np
import pytest

import opendht_amd
import refill_ref as F
from opendht_amd import DeviceSearches, DeviceTable, KadError, _lib

INVALID, UNSUPPORTED, NOT_SORTED = _lib.KAD_ERR_INVALID, _lib.KAD_ERR_UNSUPPORTED, _lib.KAD_ERR_NOT_SORTED
CONSTANTS = {"KAD_SN_REMOVABLE": 2, "KAD_SR_REFILL_OK": 0, "KAD_SR_REFILL_OVERFLOW": 1}
p = _lib.ptr


def test_symbols_constants_and_signatures():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n, nargs in (("kad_sr_refill", 8), ("kad_sr_refill_kernel_ms", 2)):
        assert hasattr(L, n) and f"int {n}(" in hdr
        assert _lib.SIGNATURES[n][0] is C.c_int and len(_lib.SIGNATURES[n][1]) == nargs
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert any(f"#define {name} {lit}" in hdr for lit in (f"{val}u", f"0x{val:02X}u")), name
    assert F.SN_REMOVABLE == _lib.KAD_SN_REMOVABLE and F.REFILL_OVERFLOW == _lib.KAD_SR_REFILL_OVERFLOW
    assert callable(opendht_amd.refill_searches) and callable(opendht_amd.DeviceSearches.refill)


def test_null_and_order_checks_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)  # as a set: S == 0; as a table it is never reached by these checks
    which = np.array([0], np.uint32)
    rows = np.full((1, 14), 0xAAAAAAAA, np.uint32)
    cnt, st = np.full(1, 0xAA, np.uint8), np.full(1, 0xAA, np.uint8)
    ins = np.full(1, 0xAAAA, np.uint16)
    for m in (1, 0):
        assert L.kad_sr_refill(None, p(fake), m, p(which), p(rows), p(cnt), p(ins), p(st)) == INVALID
        assert b"NULL" in L.kad_last_error()
        assert L.kad_sr_refill(p(fake), None, m, p(which), p(rows), p(cnt), p(ins), p(st)) == INVALID
        assert b"NULL" in L.kad_last_error()
    assert L.kad_sr_refill(p(fake), p(fake), 1, None, p(rows), p(cnt), p(ins), p(st)) == INVALID
    assert L.kad_sr_refill(p(fake), p(fake), 1, p(which), p(rows), None, p(ins), p(st)) == INVALID
    assert L.kad_sr_refill(p(fake), p(fake), 1, p(which), p(rows), p(cnt), None, p(st)) == INVALID
    assert L.kad_sr_refill(p(fake), p(fake), 1, p(which), p(rows), p(cnt), p(ins), None) == INVALID
    assert b"NULL" in L.kad_last_error()
    # a set of no searches: every index is out of range, before the table is looked at
    assert L.kad_sr_refill(p(fake), p(fake), 1, p(which), None, p(cnt), p(ins), p(st)) == INVALID
    assert b"strictly ascending and below S" in L.kad_last_error()
    assert L.kad_sr_refill_kernel_ms(None, C.byref(C.c_float())) == INVALID
    assert L.kad_sr_refill_kernel_ms(p(fake), None) == INVALID
    assert (rows == 0xAAAAAAAA).all() and (cnt == 0xAA).all() and (ins == 0xAAAA).all() and (st == 0xAA).all()


def _export_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_refusals_in_order_leave_the_set(gpu):
    L = _lib.lib()
    c = F.case("n40_s65_cap14")
    ids, status = c["cache"].table_arrays()
    S = len(c["searches"])
    rows = np.zeros((3, 14), np.uint32)
    cnt, st, ins = np.zeros(3, np.uint8), np.zeros(3, np.uint8), np.zeros(3, np.uint16)
    first = np.zeros((1, 20), np.uint8)
    with DeviceTable(ids, status, device=0, sorted=True) as NC, \
            DeviceTable(ids, status, first, np.array([0, len(ids)], np.uint32), device=0) as RT, \
            DeviceSearches(*F.snapshot(c["searches"], F.NOW), cap=c["cap"], device=0) as DS:
        before = DS.export()

        def call(ss, nc, m, which, r=rows, n=cnt, i=ins, s=st):
            return L.kad_sr_refill(ss, nc, m, p(which) if which is not None else None, p(r), p(n), p(i), p(s))

        good = c["which"][(c["ins"] != 0) & (c["status"] == F.REFILL_OK)][:3].copy()  # three searches a refill changes
        assert good.shape == (3,)
        unsorted = good[[1, 0, 2]].copy()
        # NULL handles first, even with a bad list
        assert call(None, NC.handle, 3, unsorted) == INVALID and b"NULL" in L.kad_last_error()
        assert call(DS._h, None, 3, unsorted) == INVALID and b"NULL" in L.kad_last_error()
        # NULL arrays before the order of `which`
        assert call(DS._h, RT.handle, 3, unsorted, n=None) == INVALID and b"NULL" in L.kad_last_error()
        assert call(DS._h, RT.handle, 3, None) == INVALID and b"NULL" in L.kad_last_error()
        # `which` before the table's flags: descending, repeated, out of range
        for w in (unsorted, good[[0, 0, 2]].copy(), np.array([good[0], good[1], S], np.uint32)):
            assert call(DS._h, RT.handle, 3, w) == INVALID
            assert b"strictly ascending and below S" in L.kad_last_error()
        # a table without KAD_TABLE_SORTED, also with m == 0
        assert call(DS._h, RT.handle, 3, good) == NOT_SORTED
        assert call(DS._h, RT.handle, 0, good) == NOT_SORTED
        if torch_devices() > 1:  # a table on another device
            with DeviceTable(ids, status, device=1, sorted=True) as other:
                assert call(DS._h, other.handle, 3, good) == INVALID and b"device" in L.kad_last_error()
                assert call(DS._h, other.handle, 0, good) == INVALID
        assert call(DS._h, NC.handle, 0, good) == 0 and call(DS._h, NC.handle, 0, None, n=None, i=None, s=None) == 0
        assert _export_equal(before, DS.export())
        assert call(DS._h, NC.handle, 3, good, r=None) == 0  # out_rows may be NULL: the other outputs are as with it
        k = np.searchsorted(c["which"], good)
        assert np.array_equal(cnt, c["cnt"][k]) and np.array_equal(ins, c["ins"][k]) and np.array_equal(st, c["status"][k])
        assert not _export_equal(before, DS.export())


def torch_devices():
    import torch

    return torch.cuda.device_count()


@pytest.mark.gpu
def test_slabs_of_more_than_64_entries_are_unsupported(gpu):
    """The refill kernel holds one list entry per lane: cap 64 works (test_refill.py), cap 65 answers
    KAD_ERR_UNSUPPORTED after every other check and leaves the set; m == 0 is still KAD_OK."""
    c = F.case("n40_s3_cap64")
    ids, status = c["cache"].table_arrays()
    with DeviceTable(ids, status, device=0, sorted=True) as NC, \
            DeviceSearches(*F.snapshot(c["searches"], F.NOW), cap=65, device=0) as DS:
        before = DS.export()
        with pytest.raises(KadError) as e:
            DS.refill(NC, np.array([0, 2], np.uint32))
        assert e.value.code == UNSUPPORTED
        with pytest.raises(KadError) as e:  # the order of `which` is checked first
            DS.refill(NC, np.array([2, 0], np.uint32))
        assert e.value.code == INVALID
        rows, cnt, ins, st = DS.refill(NC, np.zeros(0, np.uint32))
        assert rows.shape == (0, 14) and cnt.size == 0
        assert _export_equal(before, DS.export())
