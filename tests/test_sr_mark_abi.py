"""kad_sr_mark_nodes' entry points: symbols, constants and signatures; every argument check in the
order include/kadgpu.h documents, on a zeroed buffer standing in for a set of no searches and on exact-size arrays,
without a GPU; and on the GPU the same refusals against a real set, each leaving the set as exported before, the slab
limit of 64 entries included, and kad_searches_info unchanged on a set that never marked."""
import ctypes as C
import os

import numpy as np
import pytest

import insert_ref as I
import mark_ref as M
import opendht_amd
import searches_ref as R
from opendht_amd import DeviceSearches, KadError, _lib

INVALID, UNSUPPORTED = _lib.KAD_ERR_INVALID, _lib.KAD_ERR_UNSUPPORTED
p = _lib.ptr


def test_symbols_constants_and_signatures():
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for n, nargs in (("kad_sr_mark_nodes", 14), ("kad_sr_mark_kernel_ms", 3)):
        assert hasattr(L, n) and f"int {n}(" in hdr
        assert _lib.SIGNATURES[n][0] is C.c_int and len(_lib.SIGNATURES[n][1]) == nargs
    assert _lib.KAD_SR_MARK_MAX_NODES == opendht_amd.KAD_SR_MARK_MAX_NODES == 1 << 20
    assert "#define KAD_SR_MARK_MAX_NODES (1u << 20)" in hdr
    assert M.SN_BAD == _lib.KAD_SN_BAD and M.SN_REMOVABLE == _lib.KAD_SN_REMOVABLE
    assert callable(opendht_amd.mark_search_nodes)
    assert callable(opendht_amd.DeviceSearches.mark_nodes) and callable(opendht_amd.DeviceSearches.mark_kernel_ms)


class Args:
    """Exact-size arrays of a valid call: q nodes, pr pairs."""

    def __init__(self, q=3, pr=2, S=0):
        rng = np.random.default_rng(q + 10 * pr)
        self.q, self.pr = q, pr
        self.ids = rng.integers(0, 256, (q, 20), dtype=np.uint8)
        self.clear, self.set = np.full(q, 2, np.uint8), np.full(q, 1, np.uint8)
        self.pw = np.zeros(pr, np.uint32)
        self.pid = rng.integers(0, 256, (pr, 20), dtype=np.uint8)
        self.pfl = np.full(pr, 3, np.uint8)
        self.hits, self.found = np.full(q, 0xAAAAAAAA, np.uint32), np.full(pr, 0xAA, np.uint8)
        self.changed, self.counts = np.full(max(S, 1), 0xAAAAAAAA, np.uint32), np.full(4 * max(S, 1), 0xAA, np.uint8)
        self.n = C.c_uint32(0xAAAAAAAA)

    def call(self, L, ss, **kw):
        a = dict(ids=p(self.ids), clear=p(self.clear), set=p(self.set), pw=p(self.pw), pid=p(self.pid), pfl=p(self.pfl),
                 hits=p(self.hits), found=p(self.found), changed=p(self.changed), counts=p(self.counts),
                 n=C.byref(self.n), q=self.q, pr=self.pr)
        for k, v in kw.items():
            a[k] = p(v) if isinstance(v, np.ndarray) else v
        return L.kad_sr_mark_nodes(ss, a["q"], a["ids"], a["clear"], a["set"], a["pr"], a["pw"], a["pid"], a["pfl"],
                                   a["hits"], a["found"], a["changed"], a["counts"], a["n"])

    def untouched(self):
        return ((self.hits == 0xAAAAAAAA).all() and (self.found == 0xAA).all() and (self.changed == 0xAAAAAAAA).all()
                and (self.counts == 0xAA).all() and self.n.value == 0xAAAAAAAA)


def refusals(L, ss, S, A, in_range):
    """Every refusal in header order: each check is reached with every later one also violated."""
    q, pr = A.q, A.pr
    bad_clear, bad_set, bad_pfl = A.clear.copy(), A.set.copy(), A.pfl.copy()
    bad_clear[-1], bad_set[0], bad_pfl[-1] = 4, 0x80, 8
    both = A.set.copy()
    both[1] = 3  # clear 2, set 3: bit 2 both ways
    dup = A.ids.copy()
    dup[2] = dup[0]
    pw_out = A.pw.copy()
    pw_out[-1] = S
    pdup_w, pdup_i = A.pw.copy(), A.pid.copy()
    pdup_w[:] = in_range
    pdup_i[1] = pdup_i[0]
    later = dict(ids=dup, pw=pw_out)  # what a later check would refuse
    # NULLs: the handle, the outputs that may not be NULL, then the inputs
    assert A.call(L, None, clear=bad_clear) == INVALID and b"NULL" in L.kad_last_error()
    assert A.call(L, ss, changed=None, clear=bad_clear) == INVALID and b"NULL" in L.kad_last_error()
    assert A.call(L, ss, n=None, clear=bad_clear) == INVALID and b"NULL" in L.kad_last_error()
    assert A.call(L, ss, ids=None, clear=bad_clear) == INVALID and b"NULL node_ids" in L.kad_last_error()
    for k in ("pw", "pid", "pfl"):
        assert A.call(L, ss, clear=bad_clear, **{k: None}) == INVALID and b"NULL pair" in L.kad_last_error()
    # unknown bits, in clear_bits, set_bits, pair_flags
    assert A.call(L, ss, clear=bad_clear, set=bad_set, pfl=bad_pfl, **later) == INVALID
    assert b"clear_bits" in L.kad_last_error()
    assert A.call(L, ss, set=bad_set, pfl=bad_pfl, **later) == INVALID and b"set_bits" in L.kad_last_error()
    assert A.call(L, ss, pfl=bad_pfl, set=both, **later) == INVALID and b"pair_flags" in L.kad_last_error()
    # a bit both cleared and set
    assert A.call(L, ss, set=both, **later) == INVALID and b"both cleared and set" in L.kad_last_error()
    # equal node IDs before the pairs
    assert A.call(L, ss, **later) == INVALID and b"node IDs" in L.kad_last_error()
    # a pair's search out of range before equal pairs
    w = pdup_w.copy()
    w[-1] = S
    assert A.call(L, ss, pw=w, pid=pdup_i) == INVALID and b"not below S" in L.kad_last_error()
    assert A.call(L, ss, pw=np.full(pr, 0xFFFFFFFF, np.uint32)) == INVALID and b"not below S" in L.kad_last_error()
    if S:
        assert A.call(L, ss, pw=pdup_w, pid=pdup_i) == INVALID and b"are equal" in L.kad_last_error()
    assert A.untouched()


def test_checks_in_order_without_a_device():
    L = _lib.lib()
    fake = np.zeros(1 << 12, np.uint8)  # a set of no searches
    A = Args()
    refusals(L, p(fake), 0, A, 0)
    # NULL clear / set are all zero; without pairs a set of no searches answers OK and zeroes hits
    B = Args(q=4, pr=0)
    assert B.call(L, p(fake), clear=None, set=None, pw=None, pid=None, pfl=None, found=None) == 0
    assert B.n.value == 0 and (B.hits == 0).all() and (B.changed == 0xAAAAAAAA).all()
    B = Args(q=4, pr=0)
    assert B.call(L, p(fake), hits=None, counts=None) == 0 and B.n.value == 0
    B = Args(q=0, pr=0)
    assert B.call(L, p(fake), ids=None, clear=None, set=None, hits=None, found=None, counts=None) == 0 and B.n.value == 0
    # more than KAD_SR_MARK_MAX_NODES nodes: refused after the list checks, before "no searches" is OK
    big = Args(q=_lib.KAD_SR_MARK_MAX_NODES + 1, pr=0)
    assert big.call(L, p(fake)) == UNSUPPORTED and b"2^20" in L.kad_last_error() and big.untouched()
    big.ids[7] = big.ids[3]
    assert big.call(L, p(fake)) == INVALID and b"node IDs" in L.kad_last_error()
    edge = Args(q=_lib.KAD_SR_MARK_MAX_NODES, pr=0)
    assert edge.call(L, p(fake)) == 0 and edge.n.value == 0
    # the timing aid
    a, b = C.c_float(1.0), C.c_float(1.0)
    assert L.kad_sr_mark_kernel_ms(None, C.byref(a), C.byref(b)) == INVALID
    assert L.kad_sr_mark_kernel_ms(p(fake), None, C.byref(b)) == INVALID
    assert L.kad_sr_mark_kernel_ms(p(fake), C.byref(a), None) == INVALID
    assert L.kad_sr_mark_kernel_ms(p(fake), C.byref(a), C.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0
    # a zeroed set reports no device bytes: the new members are inert at zero
    nbytes = C.c_uint64(1)
    assert L.kad_searches_info(p(fake), None, None, C.byref(nbytes)) == 0 and nbytes.value == 0


def _export_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_refusals_in_order_leave_the_set(gpu):
    L = _lib.lib()
    c = M.case("s65_cap32_q65_p1")
    S = len(c["searches"])
    with DeviceSearches(*I.snapshot(c["searches"]), cap=c["cap"], device=0) as DS, \
            DeviceSearches(*I.snapshot(c["searches"]), cap=c["cap"], device=0) as never:
        before, nbytes = DS.export(), DS.device_bytes
        A = Args(q=3, pr=2, S=S)
        holders = {}
        for s in c["searches"]:
            for x, _ in s.ents:
                holders[x] = holders.get(x, 0) + 1
        held = [(i, s.ents[0][0]) for i, s in enumerate(c["searches"])
                if s.ents and s.ents[0][1] != 3 and holders[s.ents[0][0]] == 1][:2]
        A.ids[:2] = R.id_bytes([x for _, x in held])  # the valid call would change two searches
        A.pw[:] = [held[0][0], held[1][0]]
        A.pid[:] = A.ids[:2]
        refusals(L, DS._h, S, A, held[0][0])
        assert _export_equal(before, DS.export()) and DS.device_bytes == nbytes
        # nothing to do is OK and leaves the set and the scratch alone
        Z = Args(q=0, pr=0, S=S)
        assert Z.call(L, DS._h) == 0 and Z.n.value == 0 and DS.device_bytes == nbytes
        # the valid call: both searches change, and the scratch is counted from now on
        assert A.call(L, DS._h) == 0 and A.n.value == 2
        assert sorted(A.changed[:2]) == sorted(i for i, _ in held) and list(A.found) == [1, 1]
        assert A.hits[0] >= 1 and A.hits[1] >= 1 and A.hits[2] == 0
        assert not _export_equal(before, DS.export())
        assert DS.device_bytes == nbytes + 16 + 4 * ((S + 31) // 32) + 12 * S
        assert never.device_bytes == nbytes


@pytest.mark.gpu
def test_slabs_of_more_than_64_entries_are_unsupported(gpu):
    """The fix kernel holds one list entry per lane: cap 64 works (test_sr_mark.py), cap 65 answers KAD_ERR_UNSUPPORTED
    after every list check, also with nothing to do (the header's order), and leaves the set."""
    c = M.case("s3_cap64_q63")
    ids = R.id_bytes(c["nodes"])
    with DeviceSearches(*I.snapshot(c["searches"]), cap=65, device=0) as DS:
        before = DS.export()
        with pytest.raises(KadError) as e:
            DS.mark_nodes(ids, c["clear"], c["set"])
        assert e.value.code == UNSUPPORTED
        with pytest.raises(KadError) as e:  # the list checks come first
            DS.mark_nodes(ids, c["clear"], c["clear"] | 1)
        assert e.value.code == INVALID
        with pytest.raises(KadError) as e:  # the slab limit is checked before "nothing to do"
            DS.mark_nodes(np.zeros((0, 20), np.uint8))
        assert e.value.code == UNSUPPORTED
        assert _export_equal(before, DS.export())
