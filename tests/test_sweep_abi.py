"""CPU tests of the whole-table sweep entry points (kad_table_sweep, _host, kad_table_expire): the symbols, constants
and DeviceTable methods exist, and the argument checks documented in include/kadgpu.h answer before any device work, so
they can be exercised without a GPU (a zeroed block stands in for a table handle: the checks read at most its host
fields, where "no times uploaded" is a NULL pointer). A refused call leaves its output buffers untouched."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

INVALID = _lib.KAD_ERR_INVALID
FIELDS = ("good", "dubious", "expired", "incoming", "changed_buckets", "empty_buckets", "flags", "reserved")


def _args():
    fake = np.zeros(1 << 16, np.uint8)  # stands in for a table without times: the checks return before the device
    tot = np.full(8, 0xAAAAAAAA, np.uint32)
    nodes = np.full(16, 0xAAAAAAAA, np.uint32)
    buckets = np.full(16, 0xAAAAAAAA, np.uint32)
    return fake, tot, nodes, buckets


def _calls(L):
    return ((L.kad_table_sweep, (None,)), (L.kad_table_sweep_host, ()))


def _untouched(*arrays):
    return all((a == 0xAAAAAAAA).all() for a in arrays)


def test_symbols_constants_methods():
    L = _lib.lib()
    for n in ("kad_table_sweep", "kad_table_sweep_host", "kad_table_expire"):
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    assert _lib.KAD_SWEEP_INCOMING == 1 and opendht_amd.KAD_SWEEP_INCOMING == 1
    assert "#define KAD_SWEEP_INCOMING 1u" in hdr
    for decl in ("int kad_table_sweep(", "int kad_table_sweep_host(", "int kad_table_expire(", "} kad_sweep_totals;"):
        assert decl in hdr, decl
    body = hdr[hdr.index("typedef struct kad_sweep_totals"):hdr.index("} kad_sweep_totals;")]
    pos = [body.index(f"uint32_t {f};") for f in FIELDS]
    assert pos == sorted(pos)  # the header's field order
    assert tuple(f for f, _ in _lib.sweep_totals._fields_) == FIELDS and C.sizeof(_lib.sweep_totals) == 32
    for m in ("sweep", "sweep_host", "expire"):
        assert callable(getattr(opendht_amd.DeviceTable, m))


def test_signatures():
    res, args = _lib.SIGNATURES["kad_table_sweep"]
    assert res is C.c_int and len(args) == 8 and args.count(C.c_uint32) == 3
    res, args = _lib.SIGNATURES["kad_table_sweep_host"]
    assert res is C.c_int and len(args) == 7 and args.count(C.c_uint32) == 3
    res, args = _lib.SIGNATURES["kad_table_expire"]
    assert res is C.c_int and len(args) == 8 and args.count(C.c_uint32) == 2


def test_null_arguments():
    L = _lib.lib()
    fake, tot, nodes, buckets = _args()
    p = _lib.ptr
    for fn, tail in _calls(L):
        assert fn(None, 0, p(tot), p(nodes), 16, p(buckets), 16, *tail) == INVALID
        assert b"NULL table" in L.kad_last_error()
        assert fn(p(fake), 0, None, p(nodes), 16, p(buckets), 16, *tail) == INVALID
        assert b"NULL totals" in L.kad_last_error()
        # a NULL list is "not wanted" only with cap 0
        assert fn(p(fake), 0, p(tot), None, 16, p(buckets), 16, *tail) == INVALID
        assert fn(p(fake), 0, p(tot), p(nodes), 16, None, 1, *tail) == INVALID
        assert b"cap" in L.kad_last_error()
    assert _untouched(tot, nodes, buckets)


def test_unknown_flags():
    L = _lib.lib()
    fake, tot, nodes, buckets = _args()
    p = _lib.ptr
    for fn, tail in _calls(L):
        for flags in (2, 3, 0x80000000, 0x80000001):
            assert fn(p(fake), flags, p(tot), p(nodes), 16, p(buckets), 16, *tail) == INVALID
            assert b"flags" in L.kad_last_error()
            assert fn(p(fake), flags, p(tot), None, 0, None, 0, *tail) == INVALID
    assert _untouched(tot, nodes, buckets)


def test_incoming_needs_times():
    L = _lib.lib()
    fake, tot, nodes, buckets = _args()
    p = _lib.ptr
    for fn, tail in _calls(L):
        assert fn(p(fake), _lib.KAD_SWEEP_INCOMING, p(tot), p(nodes), 16, p(buckets), 16, *tail) == INVALID
        assert b"kad_table_set_times" in L.kad_last_error()
        assert fn(p(fake), _lib.KAD_SWEEP_INCOMING, p(tot), None, 0, None, 0, *tail) == INVALID
    assert _untouched(tot, nodes, buckets)


def test_expire_arguments():
    """NULL table, a NULL list with a cap, and a handle without buckets (the zeroed block: n_buckets == 0) are refused
    before any device work."""
    L = _lib.lib()
    fake, tot, nodes, buckets = _args()
    p = _lib.ptr
    nr = np.full(1, 0xAAAAAAAA, np.uint32)
    nb = np.full(1, 0xAAAAAAAA, np.uint32)
    assert L.kad_table_expire(None, None, p(nodes), 16, p(nr), p(buckets), 16, p(nb)) == INVALID
    assert L.kad_table_expire(p(fake), None, None, 16, p(nr), p(buckets), 16, p(nb)) == INVALID
    assert L.kad_table_expire(p(fake), None, p(nodes), 16, p(nr), None, 16, p(nb)) == INVALID
    assert L.kad_table_expire(p(fake), None, p(nodes), 16, p(nr), p(buckets), 16, p(nb)) == INVALID
    assert b"RoutingTable" in L.kad_last_error()
    assert _untouched(nodes, buckets, nr, nb)
