"""CPU tests of the onNewNode triage entry points (kad_rt_triage_batch, _host): the symbols and constants exist,
and the argument checks documented in include/kadgpu.h answer before the table is read or any device work starts,
so they can be exercised without a GPU (a table handle that is never dereferenced stands in where a non-NULL one
is needed)."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

NAMES = ("kad_rt_triage_batch", "kad_rt_triage_batch_host")
INVALID = _lib.KAD_ERR_INVALID
CONSTANTS = {"KAD_NN_NONE": 0, "KAD_NN_KNOWN": 1, "KAD_NN_REPLACE": 2, "KAD_NN_INSERT": 3, "KAD_NN_SPLIT": 4,
             "KAD_NN_FULL": 5, "KAD_NN_KIND_MASK": 0x0F, "KAD_NN_MYBUCKET": 0x10, "KAD_NN_BOOTSTRAP": 1}


def _args():
    fake = np.zeros(1 << 16, np.uint8)  # stands in for a table: the checks below return before reading it
    sid = np.arange(20, dtype=np.uint8)
    ids = np.zeros((4, 20), np.uint8)
    verdict = np.full(4, 0xAA, np.uint8)
    node = np.full(4, 0xAAAAAAAA, np.uint32)
    bucket = np.full(4, 0xAAAAAAAA, np.uint32)
    return fake, sid, ids, verdict, node, bucket


def _calls(L):
    return ((L.kad_rt_triage_batch, (None,)), (L.kad_rt_triage_batch_host, ()))


def test_symbols_and_constants():
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert any(f"#define {name} {lit}" in hdr for lit in (f"{val}u", f"0x{val:02X}u")), name
    assert "int kad_rt_triage_batch(" in hdr and "int kad_rt_triage_batch_host(" in hdr
    assert callable(opendht_amd.ingest)
    for m in ("rt_triage", "rt_triage_host"):
        assert callable(getattr(opendht_amd.DeviceTable, m))


def test_signatures():
    res, args = _lib.SIGNATURES["kad_rt_triage_batch"]
    assert res is C.c_int and len(args) == 9 and args.count(C.c_uint32) == 2
    res, args = _lib.SIGNATURES["kad_rt_triage_batch_host"]
    assert res is C.c_int and len(args) == 8 and args.count(C.c_uint32) == 2


def test_null_arguments():
    L = _lib.lib()
    fake, sid, ids, verdict, node, bucket = _args()
    p = _lib.ptr
    for fn, tail in _calls(L):
        assert fn(None, p(sid), p(ids), 4, 0, p(verdict), p(node), p(bucket), *tail) == INVALID
        assert b"NULL table" in L.kad_last_error()
        assert fn(p(fake), p(sid), None, 4, 0, p(verdict), p(node), p(bucket), *tail) == INVALID
        assert b"NULL buffer" in L.kad_last_error()
        assert fn(p(fake), p(sid), p(ids), 4, 0, None, p(node), p(bucket), *tail) == INVALID
        assert fn(p(fake), p(sid), p(ids), 4, 0, p(verdict), None, p(bucket), *tail) == INVALID
        # the same with q == 0
        assert fn(None, p(sid), p(ids), 0, 0, p(verdict), p(node), p(bucket), *tail) == INVALID
        assert fn(p(fake), p(sid), None, 0, 0, p(verdict), p(node), p(bucket), *tail) == INVALID
        assert fn(p(fake), p(sid), p(ids), 0, 0, None, p(node), p(bucket), *tail) == INVALID
        assert fn(p(fake), p(sid), p(ids), 0, 0, p(verdict), None, p(bucket), *tail) == INVALID
    assert (verdict == 0xAA).all() and (node == 0xAAAAAAAA).all() and (bucket == 0xAAAAAAAA).all()


def test_unknown_flags():
    L = _lib.lib()
    fake, sid, ids, verdict, node, bucket = _args()
    p = _lib.ptr
    for fn, tail in _calls(L):
        for flags in (2, 0x80000000, 3):
            for q in (4, 0):
                assert fn(p(fake), p(sid), p(ids), q, flags, p(verdict), p(node), p(bucket), *tail) == INVALID
                assert b"flags" in L.kad_last_error()
    assert (verdict == 0xAA).all() and (node == 0xAAAAAAAA).all() and (bucket == 0xAAAAAAAA).all()


def test_empty_batch():
    """q == 0 with valid pointers: KAD_OK, with or without self_id and bucket, either flag value."""
    L = _lib.lib()
    fake, sid, ids, verdict, node, bucket = _args()
    p = _lib.ptr
    for fn, tail in _calls(L):
        for flags in (0, 1):
            assert fn(p(fake), p(sid), p(ids), 0, flags, p(verdict), p(node), p(bucket), *tail) == 0
            assert fn(p(fake), None, p(ids), 0, flags, p(verdict), p(node), None, *tail) == 0
    assert (verdict == 0xAA).all() and (node == 0xAAAAAAAA).all() and (bucket == 0xAAAAAAAA).all()
