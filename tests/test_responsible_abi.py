"""CPU tests of the storage-responsibility entry points (kad_rt_responsible_batch, _dual, _host): the symbols
exist, and the argument checks documented in include/kadgpu.h answer before the table is read or any device
work starts, so they can be exercised without a GPU (a table handle that is never dereferenced stands in
where a non-NULL one is needed)."""
import ctypes as C
import os

import numpy as np

from opendht_amd import KAD_MAX_COUNT, KAD_RESP_FAR, KAD_RESP_FAR4, KAD_RESP_FAR6, _lib

NAMES = ("kad_rt_responsible_batch", "kad_rt_responsible_batch_dual", "kad_rt_responsible_batch_host")
INVALID, UNSUPPORTED = _lib.KAD_ERR_INVALID, _lib.KAD_ERR_UNSUPPORTED


def _args():
    fake = np.zeros(1 << 16, np.uint8)  # stands in for a table: the checks below return before reading it
    sid = np.arange(20, dtype=np.uint8)
    tg = np.zeros((4, 20), np.uint8)
    out = np.full(4, 0xAA, np.uint8)
    return fake, sid, tg, out


def test_symbols_and_constants():
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    assert (KAD_RESP_FAR, KAD_RESP_FAR4, KAD_RESP_FAR6) == (1, 1, 2)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for d in ("#define KAD_RESP_FAR 1u", "#define KAD_RESP_FAR4 1u", "#define KAD_RESP_FAR6 2u"):
        assert d in hdr, d


def test_null_arguments():
    L = _lib.lib()
    fake, sid, tg, out = _args()
    p = _lib.ptr
    for fn, tail in ((L.kad_rt_responsible_batch, (None,)), (L.kad_rt_responsible_batch_host, ())):
        assert fn(None, p(sid), p(tg), 4, 8, 1, p(out), *tail) == INVALID
        assert b"NULL table" in L.kad_last_error()
        assert fn(p(fake), None, p(tg), 4, 8, 1, p(out), *tail) == INVALID
        assert fn(p(fake), p(sid), None, 4, 8, 1, p(out), *tail) == INVALID
        assert fn(p(fake), p(sid), p(tg), 4, 8, 1, None, *tail) == INVALID
        assert fn(None, p(sid), p(tg), 0, 8, 1, p(out), *tail) == INVALID  # a NULL table even with q == 0
    d = L.kad_rt_responsible_batch_dual
    assert d(None, None, p(sid), p(tg), 4, 8, 1, p(out), None) == INVALID
    assert b"both tables NULL" in L.kad_last_error()
    assert d(None, None, p(sid), p(tg), 0, 8, 1, p(out), None) == INVALID
    assert d(p(fake), None, None, p(tg), 4, 8, 1, p(out), None) == INVALID
    assert d(None, p(fake), p(sid), None, 4, 8, 1, p(out), None) == INVALID
    assert d(p(fake), None, p(sid), p(tg), 4, 8, 1, None, None) == INVALID
    assert (out == 0xAA).all()


def test_empty_batch_and_count_limit():
    L = _lib.lib()
    fake, sid, tg, out = _args()
    p = _lib.ptr
    big = KAD_MAX_COUNT + 1
    assert L.kad_rt_responsible_batch(p(fake), p(sid), p(tg), 0, 8, 1, p(out), None) == 0
    assert L.kad_rt_responsible_batch(p(fake), p(sid), p(tg), 0, big, 1, p(out), None) == 0
    assert L.kad_rt_responsible_batch_host(p(fake), p(sid), p(tg), 0, 8, 1, p(out)) == 0
    assert L.kad_rt_responsible_batch_dual(p(fake), None, p(sid), p(tg), 0, 8, 1, p(out), None) == 0
    assert L.kad_rt_responsible_batch_dual(None, p(fake), p(sid), p(tg), 0, 8, 1, p(out), None) == 0
    assert L.kad_rt_responsible_batch(p(fake), p(sid), p(tg), 4, big, 1, p(out), None) == UNSUPPORTED
    assert b"KAD_MAX_COUNT" in L.kad_last_error()
    assert L.kad_rt_responsible_batch_host(p(fake), p(sid), p(tg), 4, big, 1, p(out)) == UNSUPPORTED
    assert L.kad_rt_responsible_batch_dual(p(fake), None, p(sid), p(tg), 4, big, 1, p(out), None) == UNSUPPORTED
    assert L.kad_rt_responsible_batch_dual(None, p(fake), p(sid), p(tg), 4, 0xFFFFFFFF, 1, p(out), None) == UNSUPPORTED
    assert (out == 0xAA).all()


def test_signatures_take_three_uint32():
    for n in NAMES:
        res, args = _lib.SIGNATURES[n]
        assert res is C.c_int and args.count(C.c_uint32) == 3, n
