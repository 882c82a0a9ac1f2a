"""The kernels that finish a request, at their edges, bit-exact against the plain references of tests/wire_ref.py:
kad_buffer_nodes_batch over hand-built rows (ties, gaps, short rows, index_base, every lane count and a short last
block), kad_parse_nodes_batch over the isMartian boundaries and the IDs next to our own, the InfoHash primitives at
every bit position, and kad_infohash_get_batch over every (length, alignment) pair. The library is called directly
into buffers filled with 0xA5 and one element longer than asked for, so stale bytes and overruns show."""
import ctypes as C

import numpy as np
import pytest
import torch

import wire_ref as W
from opendht_amd import DeviceTable
from opendht_amd._lib import KAD_ERR_INVALID, KAD_ERR_UNSUPPORTED, lib, ptr

pytestmark = pytest.mark.gpu

GUARD = 0xA5
TABLES = {name: (t, base) for name, t, base in W.buffer_tables()}


def _stream(gpu):
    return C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _dev(a, gpu):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    return torch.from_numpy(a).to(gpu)


def _guarded(n_bytes, gpu):
    return torch.full((n_bytes,), GUARD, dtype=torch.uint8, device=gpu)


def _open(name, gpu):
    t, base = TABLES[name]
    return DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, index_base=base,
                       sorted=t["sorted"])


# ---------------------------------------------------------------------------------------------------------------
# kad_buffer_nodes_batch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("al", [6, 18], ids=["v4", "v6"])
def test_buffer_nodes_edges(gpu, al, table):
    t, base = TABLES[table]
    ids = t["ids"]
    addrs = W.make_addrs(ids.shape[0], al)
    row = W.SEND_NODES * (20 + al)
    L, st = lib(), _stream(gpu)
    start = 0
    with _open(table, gpu) as T:
        T.set_addrs(addrs)
        for k in W.BUFFER_KS:
            pool = W.buffer_cases(ids, base, k)
            ptg = np.stack([c.target for c in pool])
            pidx = np.stack([c.row for c in pool]).reshape(len(pool), k)
            pcnt = np.array([c.cnt for c in pool], np.uint8)
            refs = {True: W.buffer_nodes_ref(ptg, ids, addrs, pidx, pcnt, base),
                    False: W.buffer_nodes_ref(ptg, ids, addrs, pidx, None, base)}
            for q in W.BUFFER_QS:
                for use_cnt in (True, False):
                    sel = (start + np.arange(q)) % len(pool)  # q rows of the pool, from a start that moves on
                    start += 5
                    tg, idx = _dev(ptg[sel], gpu), _dev(pidx[sel], gpu)
                    cnt = _dev(pcnt[sel], gpu) if use_cnt else None
                    out, out_n = _guarded((q + 1) * row, gpu), _guarded(q + 1, gpu)
                    rc = L.kad_buffer_nodes_batch(T.handle, ptr(tg), q, ptr(idx) if k else None, ptr(cnt), k, ptr(out),
                                                  ptr(out_n), st)
                    assert rc == 0, L.kad_last_error()
                    got, gn = out.cpu().numpy().reshape(q + 1, row), out_n.cpu().numpy()
                    want, wn = refs[use_cnt]
                    what = f"{table} addr_len={al} q={q} cnt={'given' if use_cnt else 'NULL'}"
                    for i in range(q):
                        c = pool[sel[i]]
                        assert gn[i] == wn[sel[i]], f"{what} row {i} case {c.name}: n {gn[i]} != {wn[sel[i]]}"
                        assert np.array_equal(got[i], want[sel[i]]), f"{what} row {i} case {c.name}: records differ"
                    assert (got[q] == GUARD).all() and gn[q] == GUARD, f"{what}: wrote beyond row q"


def test_buffer_nodes_arguments(gpu):
    """The argument checks in the order kad_buffer_nodes_batch makes them, then a good call on the same table."""
    t, base = TABLES["base1000"]
    ids = t["ids"]
    n = ids.shape[0]
    L, st = lib(), _stream(gpu)
    a4, a6 = W.make_addrs(n, 6), W.make_addrs(n, 18)
    q, k, row = 4, 8, W.SEND_NODES * 26
    cases = W.buffer_cases(ids, base, k)[:q]
    tg = _dev(np.stack([c.target for c in cases]), gpu)
    idx_host = np.stack([c.row for c in cases])
    idx = _dev(idx_host, gpu)
    idx33 = _dev(np.full((q, 33), base, np.uint32), gpu)
    buf = _guarded(8 + (q + 1) * row, gpu)
    out, out_n = _guarded((q + 1) * row, gpu), _guarded(q + 1, gpu)

    def call(tg_, q_, idx_, k_, out_):
        return L.kad_buffer_nodes_batch(T.handle, ptr(tg_), q_, ptr(idx_), None, k_, ptr(out_), ptr(out_n), st)

    with _open("base1000", gpu) as T:
        assert call(None, 0, None, k, None) == KAD_ERR_INVALID  # before q == 0 is looked at
        assert b"kad_table_set_addrs was not called" in L.kad_last_error()
        assert call(tg, q, idx, k, out) == KAD_ERR_INVALID
        assert L.kad_table_set_addrs(T.handle, 5, ptr(a4)) == KAD_ERR_INVALID
        assert b"addr_len 5" in L.kad_last_error()
        assert call(tg, q, idx, k, out) == KAD_ERR_INVALID  # still none attached
        T.set_addrs(a4)
        assert L.kad_table_set_addrs(T.handle, 18, ptr(a6)) == KAD_ERR_INVALID
        assert b"address length changed" in L.kad_last_error()
        assert call(None, 0, None, k, None) == 0  # q == 0: nothing to read or write
        assert call(None, q, idx, k, out) == KAD_ERR_INVALID and b"NULL buffer" in L.kad_last_error()
        assert call(tg, q, None, k, out) == KAD_ERR_INVALID and b"NULL buffer" in L.kad_last_error()
        assert call(tg, q, idx, k, None) == KAD_ERR_INVALID and b"NULL buffer" in L.kad_last_error()
        odd = buf[8:]
        assert odd.data_ptr() % 16 == 8
        assert call(tg, q, idx, k, odd) == KAD_ERR_INVALID and b"16-byte aligned" in L.kad_last_error()
        assert call(tg, q, idx33, 33, out) == KAD_ERR_UNSUPPORTED and b"KAD_MAX_COUNT" in L.kad_last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == GUARD).all() and (buf.cpu().numpy() == GUARD).all(), "a refused call wrote"
        assert (out_n.cpu().numpy() == GUARD).all()
        # the table still holds the 6-byte addresses and answers; idx may be NULL at k = 0
        assert call(tg, q, idx, k, out) == 0, L.kad_last_error()
        want, wn = W.buffer_nodes_ref(tg.cpu().numpy(), ids, a4, idx_host, None, base)
        np.testing.assert_array_equal(out.cpu().numpy().reshape(q + 1, row)[:q], want)
        np.testing.assert_array_equal(out_n.cpu().numpy()[:q], wn)
        assert call(tg, q, None, 0, out) == 0, L.kad_last_error()
        got = out.cpu().numpy().reshape(q + 1, row)
        assert not got[:q].any() and (got[q] == GUARD).all()
        assert not out_n.cpu().numpy()[:q].any()
        assert L.kad_buffer_nodes_batch(T.handle, ptr(tg), q, ptr(idx), None, k, ptr(out), None, st) == 0  # out_n optional
        np.testing.assert_array_equal(out.cpu().numpy().reshape(q + 1, row)[:q], want)


# ---------------------------------------------------------------------------------------------------------------
# kad_parse_nodes_batch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec_len", [26, 38])
def test_parse_nodes_edges(gpu, rec_len):
    names, rec, myid = W.parse_cases(rec_len)
    want = W.parse_nodes_ref(rec, rec_len, myid)
    flat = rec.reshape(-1)
    m = len(names)
    L, st, dev = lib(), _stream(gpu), gpu.index or 0
    for off in range(4):  # the records follow a header of `off` bytes: nothing may assume an aligned record
        host = np.full(off + flat.size + 5, GUARD, np.uint8)
        host[off:off + flat.size] = flat
        buf = _dev(host, gpu)
        assert buf.data_ptr() % 4 == 0
        for n in (0, 1, 255, 256, 257, m):
            keep = _guarded(n + 1, gpu)
            rc = L.kad_parse_nodes_batch(C.c_void_p(buf.data_ptr() + off), n, rec_len, ptr(myid), ptr(keep), dev, st)
            assert rc == 0, L.kad_last_error()
            got = keep.cpu().numpy()
            for i in range(n):
                assert got[i] == want[i], f"rec_len={rec_len} offset={off} n={n}: case {names[i]}: keep {got[i]}"
            assert got[n] == GUARD, f"rec_len={rec_len} offset={off} n={n}: wrote beyond keep[n]"


def test_parse_nodes_arguments(gpu):
    L, st, dev = lib(), _stream(gpu), gpu.index or 0
    myid = np.zeros(20, np.uint8)
    rec, keep = _guarded(27 * 4, gpu), _guarded(4, gpu)
    for n in (0, 4):
        assert L.kad_parse_nodes_batch(ptr(rec), n, 27, ptr(myid), ptr(keep), dev, st) == KAD_ERR_INVALID
        assert b"rec_len 27" in L.kad_last_error()
    assert L.kad_parse_nodes_batch(None, 0, 27, None, None, dev, st) == KAD_ERR_INVALID
    assert L.kad_parse_nodes_batch(None, 0, 26, None, None, dev, st) == 0
    assert L.kad_parse_nodes_batch(None, 0, 38, None, None, dev, st) == 0
    for args in ((None, myid, keep), (rec, None, keep), (rec, myid, None)):
        assert L.kad_parse_nodes_batch(ptr(args[0]), 4, 26, ptr(args[1]), ptr(args[2]), dev, st) == KAD_ERR_INVALID
    torch.cuda.synchronize()
    assert (keep.cpu().numpy() == GUARD).all()


# ---------------------------------------------------------------------------------------------------------------
# InfoHash primitives
# ---------------------------------------------------------------------------------------------------------------
def _windows(m):
    """(start, n) for n in {1, 255, 256, 257} from the front and from the back of m cases, and all of them."""
    return [(s, n) for n in (1, 255, 256, 257) for s in (0, m - n)] + [(0, m)]


def test_xor_cmp_common_bits_edges(gpu):
    names, T, A, B = W.pair_cases()
    m = len(names)
    assert m >= 257
    want_x = np.array([W.xor_cmp_ref(t, a, b) for t, a, b in zip(T, A, B)], np.int8)
    want_c = np.array([W.common_bits_ref(a, b) for a, b in zip(A, B)], np.uint32)
    t, a, b = _dev(T, gpu), _dev(A, gpu), _dev(B, gpu)
    L, st = lib(), _stream(gpu)
    for s, n in _windows(m):
        ox, oc = _guarded(n + 1, gpu), _guarded(4 * (n + 1), gpu)
        assert L.kad_xor_cmp_batch(ptr(t[s:]), ptr(a[s:]), ptr(b[s:]), n, ptr(ox), st) == 0, L.kad_last_error()
        assert L.kad_common_bits_batch(ptr(a[s:]), ptr(b[s:]), n, ptr(oc), st) == 0, L.kad_last_error()
        gx, gc = ox.cpu().numpy().view(np.int8), oc.cpu().numpy().view(np.uint32)
        for i in range(n):
            assert gx[i] == want_x[s + i], f"xor_cmp start={s} n={n}: case {names[s + i]}: {gx[i]} != {want_x[s + i]}"
            assert gc[i] == want_c[s + i], f"common_bits start={s} n={n}: case {names[s + i]}: {gc[i]} != {want_c[s + i]}"
        assert gx.view(np.uint8)[n] == GUARD and gc[n] == 0xA5A5A5A5, f"start={s} n={n}: wrote beyond out[n]"
    # b as the first argument: the comparison is antisymmetric
    ox = _guarded(m + 1, gpu)
    assert L.kad_xor_cmp_batch(ptr(t), ptr(b), ptr(a), m, ptr(ox), st) == 0
    np.testing.assert_array_equal(ox.cpu().numpy().view(np.int8)[:m], -want_x)


def test_lowbit_edges(gpu):
    names, A = W.lowbit_cases()
    m = len(names)
    want = np.array([W.lowbit_ref(a) for a in A], np.uint32)
    a = _dev(A, gpu)
    L, st = lib(), _stream(gpu)
    for s, n in _windows(m):
        out = _guarded(4 * (n + 1), gpu)
        assert L.kad_lowbit_batch(ptr(a[s:]), n, ptr(out), st) == 0, L.kad_last_error()
        got = out.cpu().numpy().view(np.uint32)
        for i in range(n):
            assert got[i] == want[s + i], f"lowbit start={s} n={n}: case {names[s + i]}: {got[i]} != {want[s + i]}"
        assert got[n] == 0xA5A5A5A5, f"start={s} n={n}: wrote beyond out[n]"


def test_primitives_arguments(gpu):
    L, st = lib(), _stream(gpu)
    a, out = _guarded(40, gpu), _guarded(8, gpu)
    assert L.kad_xor_cmp_batch(None, None, None, 0, None, st) == 0
    assert L.kad_common_bits_batch(None, None, 0, None, st) == 0
    assert L.kad_lowbit_batch(None, 0, None, st) == 0
    assert L.kad_xor_cmp_batch(ptr(a), ptr(a), None, 2, ptr(out), st) == KAD_ERR_INVALID
    assert L.kad_common_bits_batch(ptr(a), None, 2, ptr(out), st) == KAD_ERR_INVALID
    assert L.kad_lowbit_batch(ptr(a), 2, None, st) == KAD_ERR_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()


# ---------------------------------------------------------------------------------------------------------------
# kad_infohash_get_batch
# ---------------------------------------------------------------------------------------------------------------
def test_infohash_edges(gpu):
    names, data, off = W.sha1_pack()
    keys = W.sha1_keys(data, off)
    m = len(keys)
    want = np.stack([np.frombuffer(W.sha1_ref(k), np.uint8) for k in keys])
    d, o = _dev(data, gpu), _dev(off, gpu)  # the allocation ends with the last key
    assert d.data_ptr() % 4 == 0 and d.numel() == int(off[-1])
    L, st, dev = lib(), _stream(gpu), gpu.index or 0
    for s, n in ((0, 0), (0, 1), (0, 257), (m - 257, 257), (m - 1, 1), (0, m)):
        out = _guarded(20 * (n + 1), gpu)
        rc = L.kad_infohash_get_batch(ptr(d), ptr(o[s:]), n, ptr(out), dev, st)
        assert rc == 0, L.kad_last_error()
        got = out.cpu().numpy().reshape(n + 1, 20)
        for i in range(n):
            assert np.array_equal(got[i], want[s + i]), (f"start={s} n={n}: key {names[s + i]} at offset "
                                                         f"{int(off[s + i])} ({int(off[s + i]) % 4} mod 4)")
        assert (got[n] == GUARD).all(), f"start={s} n={n}: wrote beyond out_ids[n]"


def test_infohash_empty_keys_and_arguments(gpu):
    L, st, dev = lib(), _stream(gpu), gpu.index or 0
    empty = np.frombuffer(W.sha1_ref(b""), np.uint8)
    d = _guarded(7, gpu)
    for at in (0, 3, 7):  # 300 empty keys at the start, inside, and at the very end of the buffer
        o = _dev(np.full(301, at, np.uint64), gpu)
        out = _guarded(20 * 301, gpu)
        assert L.kad_infohash_get_batch(ptr(d), ptr(o), 300, ptr(out), dev, st) == 0, L.kad_last_error()
        got = out.cpu().numpy().reshape(301, 20)
        assert (got[:300] == empty).all(), f"empty keys at offset {at}"
        assert (got[300] == GUARD).all()
    assert L.kad_infohash_get_batch(None, None, 0, None, dev, st) == 0
    o, out = _dev(np.zeros(2, np.uint64), gpu), _guarded(40, gpu)
    for args in ((None, o, out), (d, None, out), (d, o, None)):
        assert L.kad_infohash_get_batch(ptr(args[0]), ptr(args[1]), 1, ptr(args[2]), dev, st) == KAD_ERR_INVALID
        assert b"NULL buffer" in L.kad_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
