"""kad_sr_step's, kad_sr_mark_entries', kad_search_step's and kad_search_step_batch's entry points:
symbols, constants and signatures, and every argument check documented in include/kadgpu.h in its order, against a zeroed
buffer standing in for a set of no searches. CPU only; the checks that need a real set (a mode bit or a pair's search
against S > 0, the slab limit) are in test_sr_step.py and test_sr_step_entries.py, and against the host plan directly in
tests/cpp/sr_step_san.cpp."""
import ctypes as C
import os

import numpy as np

import opendht_amd
from opendht_amd import _lib

INVALID = _lib.KAD_ERR_INVALID
CONSTANTS = {"KAD_SN_CANDIDATE": 0x04, "KAD_SN_PENDING": 0x08, "KAD_SN_SYNCED": 0x10, "KAD_SN_NOGET": 0x20,
             "KAD_STEP_APPLY": 0x01, "KAD_STEP_NO_SEND": 0x02, "KAD_STEP_DONE_IF_SYNCED": 0x04, "KAD_STEP_NO_EXPIRE": 0x08,
             "KAD_STEP_SKIPPED": 0x01, "KAD_STEP_SHORT": 0x02, "KAD_STEP_SYNCED": 0x04, "KAD_STEP_DONE": 0x08,
             "KAD_STEP_EXHAUSTED": 0x10, "KAD_STEP_EXPIRE": 0x20}
p = _lib.ptr


def poisoned(n):
    """n kad_step_out records with every byte 0xAA."""
    return np.frombuffer(bytearray(b"\xAA" * (16 * n)), np.dtype(_lib.STEP_OUT_DTYPE))


def test_symbols_constants_and_signatures():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n, nargs in (("kad_sr_step", 6), ("kad_sr_mark_entries", 7), ("kad_search_step", 5), ("kad_search_step_batch", 6)):
        assert hasattr(L, n) and f"int {n}(" in hdr
        assert _lib.SIGNATURES[n][0] is C.c_int and len(_lib.SIGNATURES[n][1]) == nargs
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert f"#define {name} 0x{val:02x}u" in hdr, name
    assert "} kad_step_out;" in hdr and C.sizeof(_lib.step_out) == 16 and np.dtype(_lib.STEP_OUT_DTYPE).itemsize == 16
    assert "} kad_sr_step_stats;" in hdr and C.sizeof(_lib.sr_step_stats) == 20
    for f in ("step_searches", "search_step", "search_step_batch"):
        assert callable(getattr(opendht_amd, f))
    assert callable(opendht_amd.DeviceSearches.step) and callable(opendht_amd.DeviceSearches.mark_entries)
    # the step bits lie beside the two the record depends on, and all six fit the byte create and export carry
    assert _lib.KAD_SN_BAD | _lib.KAD_SN_REMOVABLE == 0x03
    assert _lib.KAD_SN_CANDIDATE | _lib.KAD_SN_PENDING | _lib.KAD_SN_SYNCED | _lib.KAD_SN_NOGET == 0x3C


def test_step_argument_checks_in_order_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)  # a set of no searches
    out = poisoned(4)
    which, mode, bad_mode = np.array([0, 1], np.uint32), np.zeros(2, np.uint8), np.array([0, 0x10], np.uint8)
    st = _lib.sr_step_stats()
    st.picks = 77
    # 1. NULL ss or out first, whatever else is wrong, also with m == 0
    assert L.kad_sr_step(None, 2, None, p(bad_mode), p(out), None) == INVALID and b"NULL search set" in L.kad_last_error()
    assert L.kad_sr_step(p(fake), 2, p(which), p(bad_mode), None, None) == INVALID and b"NULL search set or output" in L.kad_last_error()
    assert L.kad_sr_step(p(fake), 0, None, None, None, None) == INVALID
    # 2. which == NULL steps every search: m must be S (0 here), before the mode bytes are looked at
    assert L.kad_sr_step(p(fake), 2, None, p(bad_mode), p(out), C.byref(st)) == INVALID and b"m must be S" in L.kad_last_error()
    # 3. which out of range (S == 0: every index is), before the mode bytes
    assert L.kad_sr_step(p(fake), 2, p(which), p(bad_mode), p(out), C.byref(st)) == INVALID and b"ascending" in L.kad_last_error()
    assert L.kad_sr_step(p(fake), 1, p(which), p(mode), p(out), C.byref(st)) == INVALID and b"ascending" in L.kad_last_error()
    assert st.picks == 77 and (out["bits"] == 0xAAAAAAAA).all()
    # 5. m == 0: nothing to do; NULL stats are allowed, given ones are zeroed
    assert L.kad_sr_step(p(fake), 0, None, None, p(out), None) == 0
    assert L.kad_sr_step(p(fake), 0, p(which), p(bad_mode), p(out), C.byref(st)) == 0
    assert (st.synced, st.expired, st.skipped, st.picks, st.kernel_ms) == (0, 0, 0, 0, 0.0)
    assert (out["bits"] == 0xAAAAAAAA).all() and not fake.any()


def test_mark_entries_argument_checks_in_order_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)
    pw, ids = np.array([0, 0], np.uint32), np.zeros((2, 20), np.uint8)
    ids[1, 19] = 1
    ok, wide, found = np.array([0x04, 0x20], np.uint8), np.array([0x04, 0x01], np.uint8), np.full(2, 0xAA, np.uint8)
    both = np.array([0x08, 0x24], np.uint8)

    def call(ss, w=pw, i=ids, c=None, s=None, f=found, n=2):
        return L.kad_sr_mark_entries(ss, n, p(w), p(i), p(c), p(s), p(f))

    # 1. NULL ss first
    assert call(None, w=None, c=wide) == INVALID and b"NULL search set" in L.kad_last_error()
    # 2. NULL pair arrays with p > 0, before the bits
    assert call(p(fake), w=None, c=wide) == INVALID and b"NULL pair arrays" in L.kad_last_error()
    assert call(p(fake), i=None, s=wide) == INVALID and b"NULL pair arrays" in L.kad_last_error()
    # 3. a bit outside 0x3C, in either array, before clear & set
    assert call(p(fake), c=wide, s=both) == INVALID and b"clear_bits outside" in L.kad_last_error()
    assert call(p(fake), c=both, s=wide) == INVALID and b"set_bits outside" in L.kad_last_error()
    for bit in (0x01, 0x02, 0x40, 0x80):
        assert call(p(fake), s=np.array([0, bit], np.uint8)) == INVALID and b"set_bits outside" in L.kad_last_error()
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


def test_step_batch_checks():
    L = _lib.lib()
    out = poisoned(3)
    fl, off = np.zeros(70, np.uint8), np.array([0, 2, 5], np.uint32)
    assert L.kad_search_step_batch(0, None, None, None, None, None) == 0
    assert L.kad_search_step_batch(2, None, p(fl), None, None, p(out)) == INVALID
    assert L.kad_search_step_batch(2, p(off), p(fl), None, None, None) == INVALID
    assert L.kad_search_step_batch(2, p(off), None, None, None, p(out)) == INVALID
    assert L.kad_search_step_batch(2, p(np.array([0, 5, 2], np.uint32)), p(fl), None, None, p(out)) == INVALID
    assert L.kad_search_step_batch(2, p(np.array([0, 65, 70], np.uint32)), p(fl), None, None, p(out)) == INVALID
    assert L.kad_search_step_batch(2, p(off), p(fl), None, p(np.array([0, 0x10], np.uint8)), p(out)) == INVALID
    assert (out["bits"] == 0xAAAAAAAA).all()  # nothing is written before every check passed
    assert L.kad_search_step_batch(2, p(np.array([0, 0, 0], np.uint32)), None, None, None, p(out)) == 0
    assert L.kad_search_step_batch(2, p(np.array([0, 64, 70], np.uint32)), p(fl), None, None, p(out)) == 0
    assert list(out["counts"][:2] & 0xFF) == [64, 6] and out["bits"][2] == 0xAAAAAAAA
