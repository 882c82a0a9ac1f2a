"""CPU tests of the bucket-time entry points (kad_table_set/patch/get_bucket_times, kad_table_touch_buckets, _host,
kad_table_maintenance, _host, kad_maint_scan_host): the symbols, constants, structs and DeviceTable methods exist, and
the argument checks documented in include/kadgpu.h answer in their order before any device work, so they run without a
GPU (a zeroed block stands in for a table handle: the checks read only its host fields, where it has no buckets). A
refused call leaves its output buffers untouched."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

INVALID = _lib.KAD_ERR_INVALID
FIELDS = ("candidates", "stale", "empty", "sure", "maybe", "never", "first_sure", "reserved")
NAMES = ("kad_table_set_bucket_times", "kad_table_patch_bucket_times", "kad_table_get_bucket_times",
         "kad_table_touch_buckets", "kad_table_touch_buckets_host", "kad_table_maintenance",
         "kad_table_maintenance_host", "kad_maint_scan_host")
NOW = 10**15
TOO_EARLY = -(1 << 63) + 600 * 10**9 - 1


def _args():
    fake = np.zeros(1 << 16, np.uint8)
    tot = np.full(8, 0xAAAAAAAA, np.uint32)
    rec = np.full(32, 0xAAAAAAAA, np.uint32)
    return fake, tot, rec


def _untouched(*arrays):
    return all((a == 0xAAAAAAAA).all() for a in arrays)


def test_symbols_constants_methods():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
        assert f"int {n}(" in hdr, n
    for name, val in (("STALE", 1), ("EMPTY", 2), ("HAS_NEXT", 4), ("NEXT_EMPTY", 8), ("HAS_PREV", 16),
                      ("PREV_EMPTY", 32), ("CLASS_SHIFT", 6), ("NEVER", 0), ("MAYBE", 1), ("SURE", 2), ("BIT_SHIFT", 8)):
        assert getattr(_lib, "KAD_MAINT_" + name) == val == getattr(opendht_amd, "KAD_MAINT_" + name)
        assert f"#define KAD_MAINT_{name} 0x{val:02x}u" in hdr or f"#define KAD_MAINT_{name} {val}u" in hdr, name
    assert _lib.KAD_MAINT_STALE_NS == 600 * 10**9 and "#define KAD_MAINT_STALE_NS 600000000000ll" in hdr
    body = hdr[hdr.index("typedef struct kad_maint_totals"):hdr.index("} kad_maint_totals;")]
    pos = [body.index(f"uint32_t {f};") for f in FIELDS]
    assert pos == sorted(pos)
    assert tuple(f for f, _ in _lib.maint_totals._fields_) == FIELDS and C.sizeof(_lib.maint_totals) == 32
    body = hdr[hdr.index("typedef struct kad_maint_rec"):hdr.index("} kad_maint_rec;")]
    assert body.index("uint32_t bucket;") < body.index("uint32_t kind;")
    assert np.dtype(_lib.MAINT_REC_DTYPE).itemsize == 8
    for m in ("set_bucket_times", "patch_bucket_times", "bucket_times", "touch_buckets", "maintenance",
              "maintenance_host"):
        assert callable(getattr(opendht_amd.DeviceTable, m))
    assert callable(opendht_amd.maint_scan_host)


def test_signatures():
    S = _lib.SIGNATURES
    for n, nargs, n32, n64 in (("kad_table_set_bucket_times", 2, 0, 0), ("kad_table_patch_bucket_times", 4, 1, 0),
                               ("kad_table_get_bucket_times", 2, 0, 0), ("kad_table_touch_buckets", 6, 1, 1),
                               ("kad_table_touch_buckets_host", 5, 1, 1), ("kad_table_maintenance", 7, 2, 1),
                               ("kad_table_maintenance_host", 6, 2, 1), ("kad_maint_scan_host", 9, 3, 1)):
        res, args = S[n]
        assert res is C.c_int and len(args) == nargs and args.count(C.c_uint32) == n32 and args.count(C.c_int64) == n64, n


def test_maintenance_checks_in_order():
    L = _lib.lib()
    fake, tot, rec = _args()
    p = _lib.ptr
    for fn, tail in ((L.kad_table_maintenance, (None,)), (L.kad_table_maintenance_host, ())):
        # every later fault is present as well: the earliest one answers
        assert fn(None, TOO_EARLY, 1, None, None, 4, *tail) == INVALID
        assert b"NULL table" in L.kad_last_error()
        assert fn(p(fake), TOO_EARLY, 1, None, None, 4, *tail) == INVALID
        assert b"NULL totals" in L.kad_last_error()
        assert fn(p(fake), TOO_EARLY, 1, p(tot), None, 4, *tail) == INVALID
        assert b"cap" in L.kad_last_error()
        assert fn(p(fake), TOO_EARLY, 1, p(tot), p(rec), 4, *tail) == INVALID
        assert b"INT64_MIN" in L.kad_last_error()
        assert fn(p(fake), TOO_EARLY, 1, p(tot), None, 0, *tail) == INVALID
        assert b"INT64_MIN" in L.kad_last_error()
        assert fn(p(fake), NOW, 1, p(tot), p(rec), 4, *tail) == INVALID
        assert b"first_bucket 1" in L.kad_last_error() and b"0 buckets" in L.kad_last_error()
    # the device form wants aligned buffers
    assert L.kad_table_maintenance(p(fake), NOW, 0, C.c_void_p(tot.ctypes.data + 2), p(rec), 4, None) == INVALID
    assert L.kad_table_maintenance(p(fake), NOW, 0, p(tot), C.c_void_p(rec.ctypes.data + 4), 4, None) == INVALID
    assert b"aligned" in L.kad_last_error()
    assert _untouched(tot, rec)


def test_bucket_time_checks():
    L = _lib.lib()
    fake, tot, rec = _args()
    p = _lib.ptr
    times = np.full(4, 0x2AAAAAAAAAAAAAAA, np.int64)
    idx = np.zeros(4, np.uint32)
    ids = np.zeros((4, 20), np.uint8)
    out = np.full(4, 0xAAAAAAAA, np.uint32)
    assert L.kad_table_set_bucket_times(None, p(times)) == INVALID and b"NULL table" in L.kad_last_error()
    assert L.kad_table_get_bucket_times(None, p(times)) == INVALID and b"NULL table" in L.kad_last_error()
    assert L.kad_table_patch_bucket_times(None, 4, None, None) == INVALID and b"NULL table" in L.kad_last_error()
    assert L.kad_table_patch_bucket_times(p(fake), 4, None, p(times)) == INVALID and b"NULL list" in L.kad_last_error()
    assert L.kad_table_patch_bucket_times(p(fake), 4, p(idx), None) == INVALID and b"NULL list" in L.kad_last_error()
    assert L.kad_table_patch_bucket_times(p(fake), 4, p(idx), p(times)) == INVALID
    assert b"bucket 0 (entry 0)" in L.kad_last_error() and b"0 buckets" in L.kad_last_error()
    assert L.kad_table_patch_bucket_times(p(fake), 0, None, None) == 0
    # a table without buckets has no times to set or read
    assert L.kad_table_set_bucket_times(p(fake), p(times)) == 0
    assert L.kad_table_get_bucket_times(p(fake), p(times)) == 0
    assert (times == 0x2AAAAAAAAAAAAAAA).all()
    for fn, tail in ((L.kad_table_touch_buckets, (None,)), (L.kad_table_touch_buckets_host, ())):
        assert fn(None, None, 4, NOW, p(out), *tail) == INVALID and b"NULL table" in L.kad_last_error()
        # B == 0 answers before q == 0 and before the NULL buffer
        assert fn(p(fake), None, 0, NOW, None, *tail) == INVALID and b"RoutingTable" in L.kad_last_error()
        assert fn(p(fake), None, 4, NOW, p(out), *tail) == INVALID and b"RoutingTable" in L.kad_last_error()
        assert fn(p(fake), p(ids), 4, NOW, p(out), *tail) == INVALID and b"RoutingTable" in L.kad_last_error()
    assert _untouched(out)
