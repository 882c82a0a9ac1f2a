"""CPU tests of the search-set entry points (kad_searches_*, kad_sr_try_insert_batch, _host, kad_search_trim): the
symbols and constants exist, the argument checks documented in include/kadgpu.h answer in their order before any
device work (so they run without a GPU; a handle that is never dereferenced stands in where a non-NULL one is
needed), and kad_search_trim equals the restated trim of Search::insertNode."""
import ctypes as C
import itertools
import os

import numpy as np

import opendht_amd
import searches_ref as R
from opendht_amd import _lib

NAMES = ("kad_search_trim", "kad_searches_create", "kad_searches_patch", "kad_searches_info", "kad_searches_export",
         "kad_searches_destroy", "kad_sr_try_insert_batch", "kad_sr_try_insert_batch_host")
INVALID, UNSUPPORTED = _lib.KAD_ERR_INVALID, _lib.KAD_ERR_UNSUPPORTED
CONSTANTS = {"KAD_SR_EXPIRED": 1, "KAD_SN_BAD": 1, "KAD_SR_STOP_END": 0, "KAD_SR_STOP_KNOWN": 1, "KAD_SR_STOP_FAR": 2,
             "KAD_SR_STOP_FAR_EXPIRED": 3}
p = _lib.ptr


def test_symbols_and_constants():
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val and getattr(opendht_amd, name) == val, name
        assert any(f"#define {name} {lit}" in hdr for lit in (f"{val}u", f"0x{val:02X}u")), name
    for n in NAMES:
        assert f"int {n}(" in hdr, n
    assert _lib.KAD_SEARCH_NODES == 14 == R.SEARCH_NODES
    assert callable(opendht_amd.try_search_insert)
    for m in ("patch", "export", "try_insert", "try_insert_host"):
        assert callable(getattr(opendht_amd.DeviceSearches, m))


def test_signatures():
    sig = _lib.SIGNATURES
    assert all(sig[n][0] is C.c_int for n in NAMES)
    assert [len(sig[n][1]) for n in NAMES] == [5, 9, 7, 4, 8, 1, 8, 7]


def _set(S=3, n=(2, 0, 3), cap=14):
    """A valid small set: ids ascending, lists ascending in distance."""
    rng = np.random.default_rng(5)
    sids = sorted(int.from_bytes(rng.bytes(20), "big") for _ in range(S))
    lists = [R.make_list(rng, sids[s], n[s]) for s in range(S)]
    off = np.zeros(S + 1, np.uint32)
    off[1:] = np.cumsum(n)
    nid = R.id_bytes([v for l in lists for v in l])
    return dict(S=S, cap=cap, ids=R.id_bytes(sids), flags=np.zeros(S, np.uint8), off=off, nid=nid,
                nfl=np.zeros(nid.shape[0], np.uint8))


def _create(L, a, out=True, **kw):
    a = dict(a, **kw)
    h = C.c_void_p()
    rc = L.kad_searches_create(C.byref(h) if out else None, 0, a["S"], a["cap"], p(a["ids"]), p(a["flags"]),
                               p(a["off"]), p(a["nid"]), p(a["nfl"]))
    assert not h.value
    return rc


def test_create_validation_in_order():
    L = _lib.lib()
    a = _set()
    assert _create(L, a, out=False) == INVALID
    for k in ("ids", "flags", "off", "nid", "nfl"):
        assert _create(L, a, **{k: None}) == INVALID, k
        assert b"NULL" in L.kad_last_error()
    # cap below KAD_SEARCH_NODES, before the order checks (the IDs here are not ascending either)
    assert _create(L, a, cap=13, ids=a["ids"][::-1].copy()) == INVALID
    assert b"cap" in L.kad_last_error()
    # search IDs: descending, then equal neighbours; before the list checks (the first list is unsorted too)
    bad_nid = a["nid"].copy()
    bad_nid[[0, 1]] = bad_nid[[1, 0]]
    assert _create(L, a, ids=a["ids"][::-1].copy(), nid=bad_nid) == INVALID
    assert b"search IDs" in L.kad_last_error()
    dup = a["ids"].copy()
    dup[1] = dup[0]
    assert _create(L, a, ids=dup) == INVALID and b"search IDs" in L.kad_last_error()
    # a list not strictly ascending in distance, and a duplicate node; before the length check (list 2 is over cap)
    long = _set(n=(2, 0, 15))
    swapped = long["nid"].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert _create(L, long, nid=swapped) == INVALID and b"distance" in L.kad_last_error()
    same = long["nid"].copy()
    same[1] = same[0]
    assert _create(L, long, nid=same) == INVALID and b"distance" in L.kad_last_error()
    assert _create(L, a, off=np.array([0, 2, 1, 5], np.uint32)) == INVALID
    # a list longer than cap: the caller recreates with a larger cap
    assert _create(L, long) == UNSUPPORTED and b"cap" in L.kad_last_error()


def test_patch_and_query_null_checks():
    L = _lib.lib()
    a = _set()
    fake = np.zeros(1 << 12, np.uint8)  # never dereferenced by the checks below
    which = np.array([0], np.uint32)
    assert L.kad_searches_patch(None, 1, p(which), p(a["flags"]), p(a["off"]), p(a["nid"]), p(a["nfl"])) == INVALID
    assert L.kad_searches_patch(p(fake), 1, None, p(a["flags"]), p(a["off"]), p(a["nid"]), p(a["nfl"])) == INVALID
    assert L.kad_searches_patch(p(fake), 1, p(which), None, p(a["off"]), p(a["nid"]), p(a["nfl"])) == INVALID
    assert L.kad_searches_patch(p(fake), 1, p(which), p(a["flags"]), None, p(a["nid"]), p(a["nfl"])) == INVALID
    assert L.kad_searches_patch(p(fake), 1, p(which), p(a["flags"]), p(a["off"]), None, p(a["nfl"])) == INVALID
    assert L.kad_searches_info(None, None, None, None) == INVALID
    assert L.kad_searches_export(None, None, None, None, None, None, None, None) == INVALID
    assert L.kad_searches_destroy(None) == 0
    ids = np.zeros((4, 20), np.uint8)
    lb, fwd, back = (np.full(4, 0xAAAAAAAA, np.uint32) for _ in range(3))
    stop = np.full(4, 0xAA, np.uint8)
    for fn, tail in ((L.kad_sr_try_insert_batch, (None,)), (L.kad_sr_try_insert_batch_host, ())):
        for q in (4, 0):
            assert fn(None, p(ids), q, p(lb), p(fwd), p(back), p(stop), *tail) == INVALID
            assert b"NULL search set" in L.kad_last_error()
            assert fn(p(fake), None, q, p(lb), p(fwd), p(back), p(stop), *tail) == INVALID
            assert b"NULL buffer" in L.kad_last_error()
            assert fn(p(fake), p(ids), q, p(lb), None, p(back), p(stop), *tail) == INVALID
            assert fn(p(fake), p(ids), q, p(lb), p(fwd), None, p(stop), *tail) == INVALID
            assert fn(p(fake), p(ids), q, p(lb), p(fwd), p(back), None, *tail) == INVALID
        assert fn(p(fake), p(ids), 0, p(lb), p(fwd), p(back), p(stop), *tail) == 0
        assert fn(p(fake), p(ids), 0, None, p(fwd), p(back), p(stop), *tail) == 0  # out_lb may be NULL
    assert (lb == 0xAAAAAAAA).all() and (fwd == 0xAAAAAAAA).all() and (back == 0xAAAAAAAA).all() and (stop == 0xAA).all()


def _trim(L, fl, sf):
    fl = np.ascontiguousarray(fl, np.uint8)
    full, t = C.c_uint32(7), C.c_uint32(7)
    assert L.kad_search_trim(fl.shape[0], p(fl) if fl.shape[0] else None, sf, C.byref(full), C.byref(t)) == 0
    return bool(full.value), t.value


def _trim_by_insert(fl, sf):
    """(full, t) as Search::insertNode's own trim leaves them, read off a search built from the flag bytes: a
    candidate farther than every entry is refused iff the search is full, and the refusal trims the list to t."""
    sid = 0
    s = R.Search(sid, bool(sf & R.SR_EXPIRED),
                 [R.SearchNode(R.Node(i + 1), candidate=bool(f & R.SN_BAD)) for i, f in enumerate(fl)])
    ok = s.insert_node(R.Node(R.MAX_ID), 0.0)
    return (not ok), (len(s.nodes) if not ok else None)


def test_search_trim_against_the_restatement():
    L = _lib.lib()
    assert L.kad_search_trim(3, None, 0, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == INVALID
    assert L.kad_search_trim(0, None, 0, None, C.byref(C.c_uint32())) == INVALID
    for sf in (0, R.SR_EXPIRED):
        for n in range(13):
            for mask in itertools.product((0, 1), repeat=n):
                assert _trim(L, mask, sf) == R.trim(mask, sf) == (False, n)
    rng = np.random.default_rng(11)
    fulls = moved = 0
    for _ in range(2000):
        n = int(rng.integers(0, 41))
        fl = (rng.random(n) < rng.random()).astype(np.uint8)
        for sf in (0, R.SR_EXPIRED):
            got = _trim(L, fl, sf)
            assert got == R.trim(list(fl), sf)
            full, t = _trim_by_insert(list(fl), sf)
            assert full == got[0] and (t is None or t == got[1])
            fulls += got[0]
            moved += got[1] < n
    assert fulls > 200 and moved > 200
