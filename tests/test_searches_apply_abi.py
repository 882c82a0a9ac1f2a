"""kad_searches_apply's entry points: the symbol, its signature and the Python surface; the argument
checks of include/kadgpu.h in their documented order, each against a call that violates that check and every later
one. They run before any device work, so a zeroed buffer stands in for a set of no searches (S == 0, cap == 0) and no
GPU is needed; the one check such a set cannot fail (new_cap below cap) is ordered on a live set in
test_searches_apply.py."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

INVALID = _lib.KAD_ERR_INVALID
p = _lib.ptr
GUARD = 0xA5A5A5A5


def test_symbol_signature_and_python_surface():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    assert hasattr(L, "kad_searches_apply") and "int kad_searches_apply(" in hdr
    restype, args = _lib.SIGNATURES["kad_searches_apply"]
    assert restype is C.c_int and len(args) == 9
    for f in (opendht_amd.DeviceSearches.apply, opendht_amd.DeviceSearches.grow, opendht_amd.start_searches,
              opendht_amd.expire_searches):
        assert callable(f)
    assert "start_searches" in opendht_amd.__all__ and "expire_searches" in opendht_amd.__all__
    assert "peak" in hdr[hdr.index("Adds and erases searches"):hdr.index("int kad_searches_apply(")]


def test_checks_in_order_on_a_set_of_no_searches():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)
    erase_bad = np.array([0], np.uint32)             # check 3: nothing is below S == 0
    dup = np.zeros((2, 20), np.uint8)                # check 6: two equal inserted IDs
    one = np.arange(20, dtype=np.uint8).reshape(1, 20)
    flags_bad = np.array([2, 0], np.uint8)           # check 5: a bit other than KAD_SR_EXPIRED
    huge = 0x7FFFFFFF                                # check 7: S' x cap' with one search
    remap = np.full(3, GUARD, np.uint32)
    new_index = np.full(4, GUARD, np.uint32)

    def call(ss, erase, n_erase, ins, fl, n_ins, cap):
        rc = L.kad_searches_apply(ss, p(erase), n_erase, p(ins), p(fl), n_ins, cap, p(remap[1:2]), p(new_index[1:3]))
        return rc, L.kad_last_error()

    # 1: a NULL set, with everything after it wrong as well
    rc, msg = call(None, None, 1, None, flags_bad, 2, huge)
    assert rc == INVALID and b"NULL search set" in msg
    # 2: NULL arrays with a count
    rc, msg = call(p(fake), None, 1, dup, flags_bad, 2, huge)
    assert rc == INVALID and b"NULL argument" in msg
    rc, msg = call(p(fake), erase_bad, 1, None, flags_bad, 2, huge)
    assert rc == INVALID and b"NULL argument" in msg
    # 3: any erase on a set of no searches
    rc, msg = call(p(fake), erase_bad, 1, dup, flags_bad, 2, huge)
    assert rc == INVALID and b"strictly ascending and below S" in msg
    rc, msg = call(p(fake), erase_bad, 1, None, None, 0, 0)
    assert rc == INVALID and b"strictly ascending and below S" in msg
    # (4 cannot fail with cap == 0)  5: an unknown flag bit
    rc, msg = call(p(fake), None, 0, dup, flags_bad, 2, huge)
    assert rc == INVALID and b"unknown search flag" in msg
    # 6: inserted IDs not distinct
    rc, msg = call(p(fake), None, 0, dup, np.array([1, 0], np.uint8), 2, huge)
    assert rc == INVALID and b"equal" in msg
    rc, msg = call(p(fake), None, 0, dup, None, 2, huge)
    assert rc == INVALID and b"equal" in msg
    # 7: the size limit of kad_searches_create
    rc, msg = call(p(fake), None, 0, one, None, 1, huge)
    assert rc == INVALID and b"too large" in msg
    # 8: nothing to do, with and without the output arrays
    assert L.kad_searches_apply(p(fake), None, 0, None, None, 0, 0, p(remap[1:2]), p(new_index[1:3])) == 0
    assert L.kad_searches_apply(p(fake), None, 0, None, None, 0, 0, None, None) == 0
    # counts of 0: the arrays are not read
    assert L.kad_searches_apply(p(fake), p(erase_bad), 0, p(one), p(flags_bad), 0, 0, None, None) == 0
    assert (remap == GUARD).all() and (new_index == GUARD).all()
    assert not fake.any()
