"""kad_sr_step_full's, kad_sr_mark_due's, kad_search_step_full's and kad_search_step_full_batch's entry points
(DESIGN.md §7.20): symbols, constants and signatures, and every argument check documented in include/kadgpu.h in its
order, against a zeroed buffer standing in for a set of no searches. CPU only; the checks that need a real set (a mode or a
pair's search against S > 0, the slab limit) are in test_sr_stepfull.py and test_sr_stepfull_due.py, and against the host
plan directly in tests/cpp/sr_stepfull_san.cpp."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

INVALID = _lib.KAD_ERR_INVALID
CONSTANTS = {"KAD_SN_LISTEN_DUE": 0x40, "KAD_SN_ANNOUNCE_DUE": 0x80, "KAD_STEP_LISTEN": 0x10, "KAD_STEP_ANNOUNCE": 0x20,
             "KAD_STEP_PROBE_BLOCKS": 0x40}
p = _lib.ptr


def poisoned(n):
    """n kad_step_full_out records with every byte 0xAA."""
    return np.frombuffer(bytearray(b"\xAA" * (32 * n)), np.dtype(_lib.STEP_FULL_OUT_DTYPE))


def test_symbols_constants_and_signatures():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n, nargs in (("kad_sr_step_full", 6), ("kad_sr_mark_due", 7), ("kad_search_step_full", 5),
                     ("kad_search_step_full_batch", 6)):
        assert hasattr(L, n) and f"int {n}(" in hdr
        assert _lib.SIGNATURES[n][0] is C.c_int and len(_lib.SIGNATURES[n][1]) == nargs
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert f"#define {name} 0x{val:02x}u" in hdr, name
    assert "} kad_step_full_out;" in hdr and C.sizeof(_lib.step_full_out) == 32
    assert np.dtype(_lib.STEP_FULL_OUT_DTYPE).itemsize == 32
    assert [np.dtype(_lib.STEP_FULL_OUT_DTYPE).fields[f][1] for f in ("picks", "listen", "announce", "counts", "bits")] == \
        [0, 8, 16, 24, 28]
    assert "} kad_sr_step_full_stats;" in hdr and C.sizeof(_lib.sr_step_full_stats) == 28
    for f in ("step_searches_full", "search_step_full", "search_step_full_batch"):
        assert callable(getattr(opendht_amd, f))
    assert callable(opendht_amd.DeviceSearches.step_full) and callable(opendht_amd.DeviceSearches.mark_due)
    # the byte is full: the two record bits, the four step bits and the two due bits
    assert _lib.KAD_SN_LISTEN_DUE | _lib.KAD_SN_ANNOUNCE_DUE == 0xC0
    assert 0x03 | 0x3C | 0xC0 == 0xFF


def test_step_full_argument_checks_in_order_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)  # a set of no searches
    out = poisoned(4)
    which, mode = np.array([0, 1], np.uint32), np.zeros(2, np.uint8)
    st = _lib.sr_step_full_stats()
    st.picks = st.listens = 77
    for bad in (0x80, 0x04 | 0x10, 0x04 | 0x20, 0x40, 0x40 | 0x10):
        bad_mode = np.array([0, bad], np.uint8)
        # 1. NULL ss or out first, whatever else is wrong, also with m == 0
        assert L.kad_sr_step_full(None, 2, None, p(bad_mode), p(out), None) == INVALID and b"NULL search set" in L.kad_last_error()
        assert L.kad_sr_step_full(p(fake), 2, p(which), p(bad_mode), None, None) == INVALID
        assert b"NULL search set or output" in L.kad_last_error()
        # 2. which == NULL steps every search: m must be S (0 here), before the mode bytes are looked at
        assert L.kad_sr_step_full(p(fake), 2, None, p(bad_mode), p(out), C.byref(st)) == INVALID
        assert b"m must be S" in L.kad_last_error()
        # 3. which out of range (S == 0: every index is), before the mode bytes
        assert L.kad_sr_step_full(p(fake), 2, p(which), p(bad_mode), p(out), C.byref(st)) == INVALID
        assert b"ascending" in L.kad_last_error()
        # 5. m == 0 is KAD_OK and reads no mode
        assert L.kad_sr_step_full(p(fake), 0, p(which), p(bad_mode), p(out), None) == 0
    assert L.kad_sr_step_full(p(fake), 0, None, None, None, None) == INVALID
    assert L.kad_sr_step_full(p(fake), 1, p(which), p(mode), p(out), C.byref(st)) == INVALID and b"ascending" in L.kad_last_error()
    assert st.picks == 77 and st.listens == 77 and (out["bits"] == 0xAAAAAAAA).all()
    # m == 0: nothing to do; NULL stats are allowed, given ones are zeroed
    assert L.kad_sr_step_full(p(fake), 0, None, None, p(out), C.byref(st)) == 0
    assert (st.synced, st.expired, st.skipped, st.picks, st.listens, st.announces, st.kernel_ms) == (0, 0, 0, 0, 0, 0, 0.0)
    assert (out["bits"] == 0xAAAAAAAA).all() and not fake.any()


def test_mark_due_argument_checks_in_order_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)
    pw, ids = np.array([0, 0], np.uint32), np.zeros((2, 20), np.uint8)
    ids[1, 19] = 1
    ok, wide, found = np.array([0x40, 0x80], np.uint8), np.array([0x40, 0x20], np.uint8), np.full(2, 0xAA, np.uint8)
    both = np.array([0x80, 0xC0], np.uint8)

    def call(ss, w=pw, i=ids, c=None, s=None, f=found, n=2):
        return L.kad_sr_mark_due(ss, n, p(w), p(i), p(c), p(s), p(f))

    # 1. NULL ss first
    assert call(None, w=None, c=wide) == INVALID and b"NULL search set" in L.kad_last_error()
    # 2. NULL pair arrays with p > 0, before the bits
    assert call(p(fake), w=None, c=wide) == INVALID and b"NULL pair arrays" in L.kad_last_error()
    assert call(p(fake), i=None, s=wide) == INVALID and b"NULL pair arrays" in L.kad_last_error()
    # 3. a bit outside 0xC0, in either array, before clear & set: every bit of 0x3C and the two record bits
    assert call(p(fake), c=wide, s=both) == INVALID and b"clear_bits outside" in L.kad_last_error()
    assert call(p(fake), c=both, s=wide) == INVALID and b"set_bits outside" in L.kad_last_error()
    for bit in (0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x3C):
        assert call(p(fake), s=np.array([0, bit], np.uint8)) == INVALID and b"set_bits outside the due bits" in L.kad_last_error()
        assert call(p(fake), c=np.array([bit, 0], np.uint8)) == INVALID and b"clear_bits outside the due bits" in L.kad_last_error()
    # 4. a bit both cleared and set, before the searches are looked at
    assert call(p(fake), c=ok, s=both) == INVALID and b"both cleared and set" in L.kad_last_error()
    # 5. pair_which[k] >= S (S == 0: every pair), before equal pairs are looked for
    same = np.zeros((2, 20), np.uint8)
    assert call(p(fake), i=same, c=ok) == INVALID and b"not below S" in L.kad_last_error()
    assert call(p(fake), c=ok) == INVALID and b"not below S" in L.kad_last_error()
    assert (found == 0xAA).all()
    # p == 0: nothing to do, NULL arrays allowed
    assert call(p(fake), w=None, i=None, f=None, n=0) == 0
    assert not fake.any()


def test_step_full_batch_checks():
    L = _lib.lib()
    out = poisoned(3)
    fl, off = np.zeros(70, np.uint8), np.array([0, 2, 5], np.uint32)
    assert L.kad_search_step_full_batch(0, None, None, None, None, None) == 0
    assert L.kad_search_step_full_batch(2, None, p(fl), None, None, p(out)) == INVALID
    assert L.kad_search_step_full_batch(2, p(off), p(fl), None, None, None) == INVALID
    assert L.kad_search_step_full_batch(2, p(off), None, None, None, p(out)) == INVALID
    assert L.kad_search_step_full_batch(2, p(np.array([0, 5, 2], np.uint32)), p(fl), None, None, p(out)) == INVALID
    assert L.kad_search_step_full_batch(2, p(np.array([0, 65, 70], np.uint32)), p(fl), None, None, p(out)) == INVALID
    for bad in (0x80, 0x14, 0x24, 0x40, 0x50):
        assert L.kad_search_step_full_batch(2, p(off), p(fl), None, p(np.array([0, bad], np.uint8)), p(out)) == INVALID
    assert (out["bits"] == 0xAAAAAAAA).all()  # nothing is written before every check passed
    assert L.kad_search_step_full_batch(2, p(np.array([0, 0, 0], np.uint32)), None, None, None, p(out)) == 0
    assert L.kad_search_step_full_batch(2, p(np.array([0, 64, 70], np.uint32)), p(fl), None,
                                        p(np.array([0x70, 0x7B], np.uint8)), p(out)) == 0
    assert list(out["counts"][:2] & 0xFF) == [64, 6] and out["bits"][2] == 0xAAAAAAAA
    assert not out["listen"][:2].any() and not out["announce"][:2].any()
