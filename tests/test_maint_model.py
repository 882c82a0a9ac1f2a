"""kad_maint_scan_host, the host twin of kad_table_maintenance (the same kadmaint::kind_of as the kernels), against the
yardstick of tests/maint_ref.py: the loop of Dht::bucketMaintenance one bucket at a time, the class by enumerating the
four trial outcomes. Every comparison is exact: totals and record bytes. CPU only."""
import ctypes as C

import numpy as np
import pytest

import maint_ref as R
import tables as TB
from opendht_amd import KadError, maint_scan_host
from opendht_amd import _lib
from opendht_amd._lib import lib, ptr

NOW = 10**15


def _same(got, want, what=""):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    assert got["records"].tobytes() == want["records"].tobytes(), (what, got["records"], want["records"])


def _first_with_bit(bit):
    """A 20-byte first whose lowbit is bit - 1 (bit 0: all zero)."""
    x = 0 if bit == 0 else (1 << (160 - bit)) | (1 << 159 if bit > 1 else 0)
    return np.frombuffer(x.to_bytes(20, "big"), np.uint8)


def test_every_small_table():
    cases = R.small_cases(NOW)
    assert len(R.width_patterns()) == 30 and len(cases) == 340
    lows, classes = set(), set()
    want_all = []
    for w, t in cases:
        _, first, off = R.table_of_widths(w)
        want = R.scan(off, first, t, NOW)
        want_all.append((off, first, t, want))
        for k in want["records"]["kind"]:
            lows.add(int(k) & 0x3F)
            classes.add((int(k) >> 6) & 3)
    assert len(lows) == 27 and classes == {R.NEVER, R.MAYBE, R.SURE}, (sorted(lows), classes)
    for off, first, t, want in want_all:
        _same(maint_scan_host(off, first, np.array(t, np.int64), NOW), want, (off, t))


def test_time_boundaries():
    _, first, off = R.table_of_widths((2, 2, 2, 2))
    t = np.array([NOW - R.TEN_MIN - 1, NOW - R.TEN_MIN, NOW - R.TEN_MIN + 1, R.INT64_MIN], np.int64)
    want = R.scan(off, first, t, NOW)
    assert list(want["records"]["bucket"]) == [0, 3]
    _same(maint_scan_host(off, first, t, NOW), want)
    # the smallest `now` the call takes: only INT64_MIN could be stale, and nothing is below it
    lo = R.INT64_MIN + R.TEN_MIN
    want = R.scan(off, first, t, lo)
    assert want["totals"]["candidates"] == 0
    _same(maint_scan_host(off, first, t, lo), want)
    want = R.scan(off, first, t, lo + 1)
    assert list(want["records"]["bucket"]) == [3]
    _same(maint_scan_host(off, first, t, lo + 1), want)
    # no times at all: every bucket at INT64_MIN
    _same(maint_scan_host(off, first, None, NOW), R.scan(off, first, None, NOW))
    _same(maint_scan_host(off, first, None, NOW), R.scan(off, first, [R.INT64_MIN] * 4, NOW))


@pytest.mark.parametrize("bit", [0, 1, 7, 8, 9, 63, 64, 65, 159, 160])
def test_random_id_bit(bit):
    """The bit of a bucket comes from its own first or from the next one's, whichever reaches lower."""
    zero = np.zeros(20, np.uint8)
    f = _first_with_bit(bit)
    assert R.lowbit(f) == bit - 1
    top = np.full(20, 0xFF, np.uint8)
    tables = [np.stack([f]), np.stack([zero, f]) if bit else np.stack([zero])]
    if 1 < bit < 160:
        tables.append(np.stack([zero, f, top]))
    for first in tables:
        B = first.shape[0]
        off = np.zeros(B + 1, np.uint32)
        want = R.scan(off, first, None, NOW)
        got = maint_scan_host(off, first, None, NOW)
        _same(got, want, bit)
        bits = [int(k) >> 8 for k in got["records"]["kind"]]
        assert bits == [R.random_id_bit(first, b) for b in range(B)]
    one = maint_scan_host(np.zeros(2, np.uint32), np.stack([f]), None, NOW)  # the last bucket has no next
    assert int(one["records"]["kind"][0]) >> 8 == bit
    allzero = maint_scan_host(np.zeros(2, np.uint32), np.stack([zero]), None, NOW)
    assert int(allzero["records"]["kind"][0]) >> 8 == 0


def test_all_small_tables():
    seen = 0
    for k, t in enumerate(TB.all_small_tables()):
        if t["first"] is None:
            continue
        B = t["first"].shape[0]
        tm = R.draw_times(B, NOW, 0xB0 + k)
        want = R.scan(t["off"], t["first"], tm, NOW)
        _same(maint_scan_host(t["off"], t["first"], tm, NOW), want, t["name"])
        seen += want["totals"]["candidates"]
    assert seen > 1000


def _nine():
    w = (2, 0, 0, 2, 2, 0, 2, 0, 2)
    ids, first, off = R.table_of_widths(w)
    tm = np.array([NOW, NOW, R.INT64_MIN, NOW - R.TEN_MIN - 1, NOW, NOW, R.INT64_MIN, NOW, NOW], np.int64)
    return first, off, tm


def test_caps_and_canary():
    first, off, tm = _nine()
    full = R.scan(off, first, tm, NOW)
    count = full["totals"]["candidates"]
    assert count >= 5
    L = lib()
    for cap in (0, 1, count - 1, count, count + 1):
        rec = np.full(count + 4, 0xAAAAAAAAAAAAAAAA, np.uint64)
        tot = _lib.maint_totals()
        rc = L.kad_maint_scan_host(9, ptr(off), ptr(first), ptr(tm), C.c_int64(NOW), 0, C.byref(tot),
                                   ptr(rec) if cap else None, cap)
        assert rc == 0
        assert {f: int(getattr(tot, f)) for f, _ in tot._fields_} == full["totals"]
        m = min(cap, count)
        assert rec[:m].tobytes() == full["records"][:m].tobytes()
        assert (rec[m:] == 0xAAAAAAAAAAAAAAAA).all()


def test_first_bucket_and_resume():
    first, off, tm = _nine()
    full = R.scan(off, first, tm, NOW)
    for fb in range(10):
        want = R.scan(off, first, tm, NOW, first_bucket=fb)
        keep = full["records"][full["records"]["bucket"] >= fb]
        assert want["records"].tobytes() == keep.tobytes()
        _same(maint_scan_host(off, first, tm, NOW, first_bucket=fb), want, fb)
    got, fb = [], 0
    while True:
        r = maint_scan_host(off, first, tm, NOW, first_bucket=fb, cap=2)
        got.extend(r["records"].tolist())
        if r["totals"]["candidates"] <= 2:
            break
        fb = int(r["records"]["bucket"][-1]) + 1
    assert got == full["records"].tolist()


def test_invalid_arguments():
    first, off, tm = _nine()
    L = lib()
    tot = _lib.maint_totals()
    rec = np.zeros(9, np.uint64)
    ok = (9, ptr(off), ptr(first), ptr(tm), C.c_int64(NOW), 0, C.byref(tot), ptr(rec), 9)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.kad_maint_scan_host(*a)

    assert call() == 0
    assert call(a1=None) == _lib.KAD_ERR_INVALID
    assert call(a2=None) == _lib.KAD_ERR_INVALID
    assert call(a6=None) == _lib.KAD_ERR_INVALID
    assert call(a7=None) == _lib.KAD_ERR_INVALID
    assert call(a7=None, a8=0) == 0
    assert call(a4=C.c_int64(R.INT64_MIN + R.TEN_MIN - 1)) == _lib.KAD_ERR_INVALID
    assert call(a4=C.c_int64(R.INT64_MIN + R.TEN_MIN)) == 0
    assert call(a5=10) == _lib.KAD_ERR_INVALID
    assert call(a5=9) == 0 and tot.candidates == 0 and tot.first_sure == 0xFFFFFFFF
    # B == 0: zero totals, NULL arrays are fine
    assert L.kad_maint_scan_host(0, None, None, None, C.c_int64(NOW), 0, C.byref(tot), None, 0) == 0
    assert [int(getattr(tot, f)) for f, _ in tot._fields_] == [0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0]
    with pytest.raises(KadError):
        maint_scan_host(off, first, tm, NOW, first_bucket=10)
