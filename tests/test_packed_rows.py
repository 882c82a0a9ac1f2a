"""The fused count-8 query kernels of owner routing's way back, kad_rt_closest_batch_packed and
kad_rt_closest_keys_packed (rt_ws_packed_kernel), called directly through the C ABI: no serve_owner around them, so
nothing answers a batch a second time. Every packed row is decoded with tests/route_ref.py and compared bit-exact with
the oracle's row (routing_table.cpp:67-111); a row the oracle says cannot be packed (span > 254) must be left unwritten
and must set the sticky escape word, and nothing else may set it.

Tables (all uniform, so all carry short window lines):
  edge    8 good nodes per bucket spanning 249 + b indices: spans 254 and 255 side by side in one batch
  short   the edge table with one bucket of 3 good nodes between all-bad buckets: rows gathered over several buckets
  few*    k = 1, 3, 7 good nodes in the whole table, spanning 254 (pack) or 255 (escape): the rows shorter than 8.
          The reference widens its window to the table's ends, so no single table mixes short and full rows
  all_bad no good node: every row empty
  dense   U(10) over 20,000 nodes, 80 % good: the line-answered common path
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import route_ref as R
import tables as TB
from opendht_amd import DeviceTable, _lib

p = _lib.ptr
SENT = 0xA5A5A5A5
PREFIXES = (1, 63, 64, 65, 255, 256, 257, 1025)
FEW = {"few1": (1, 0), "few3": (3, 254), "few7": (7, 254), "few3w": (3, 255), "few7w": (7, 255)}
CASES = ("edge", "short", "dense", "all_bad") + tuple(FEW)


@functools.lru_cache(maxsize=None)
def case(name):
    """(table, targets, oracle rows, oracle counts), computed once and never changed."""
    if name == "edge":
        t = R.edge_table()
    elif name == "short":
        t = R.short_table()
    elif name == "dense":
        t = TB.uniform_config(20_000, 10)
    elif name == "all_bad":
        t = TB.all_bad_table()
    else:
        t = R.few_table(*FEW[name])
    tg = TB.adversarial_targets(t, extra=2000) if name in ("dense", "all_bad") else R.bucket_targets(t)
    want, wcnt = O.flat_rt_closest(t["ids"], t["status"], t["first"], t["off"], tg, 8, nthreads=8)
    for a in (tg, want, wcnt):
        a.setflags(write=False)
    return t, tg, want, wcnt


def _spans(want, wcnt):
    live = np.arange(8)[None, :] < wcnt[:, None]
    w = want.astype(np.int64)
    return np.where(live, w, -1).max(1) - np.where(live, w, 1 << 40).min(1)


# ---- the fixtures, from the oracle alone (no GPU) ----------------------------------------------------------------
def test_edge_fixture_holds_the_254_255_edge():
    t, tg, want, wcnt = case("edge")
    assert tg.shape == (2064, 20) and (wcnt == 8).all()
    span = _spans(want, wcnt)
    u, n = np.unique(span, return_counts=True)
    assert u.tolist() == list(range(249, 265)) and n.min() >= 100  # every bucket's span, 253..256 among them
    for s in (253, 254, 255, 256):
        assert (span == s).sum() >= 100
    esc = R.escapes_rows(want, wcnt)
    assert np.array_equal(esc, span > 254) and esc.sum() >= 1000 and (~esc).sum() >= 600
    assert 0 < esc[:63].sum() < 63 and not esc[0]  # the short prefixes mix both classes too


def test_short_fixtures_hold_every_count():
    """cnt = 0 (all_bad: the reference's window never ends empty on a table with a good node), 0 < cnt < 8 (the few*
    tables), cnt = 8 (short, whose rows around the thinned bucket come from several buckets)."""
    _, _, want, wcnt = case("short")
    assert (wcnt == 8).all()
    span = _spans(want, wcnt)
    assert (span > 1000).sum() >= 100 and {254, 255} <= set(span.tolist())
    _, tg, want, wcnt = case("all_bad")
    assert tg.shape[0] > 257 and (wcnt == 0).all() and (want == R.NO_NODE).all()
    seen = set()
    for name, (k, s) in FEW.items():
        _, _, want, wcnt = case(name)
        assert (wcnt == k).all() and (_spans(want, wcnt) == s).all() and (want[:, k:] == R.NO_NODE).all()
        esc = R.escapes_rows(want, wcnt)
        assert esc.all() if s > 254 else not esc.any()
        seen.add(k)
    assert seen == {1, 3, 7}
    _, tg, want, wcnt = case("dense")
    assert tg.shape[0] >= 1025 and (wcnt == 8).all() and not R.escapes_rows(want, wcnt).any()


@pytest.mark.parametrize("name", CASES)
def test_fixture_nodes_have_distinct_top64(name):
    """So a key-only query can order every window: kad_rt_closest_keys_packed may never set the tail word on them."""
    k = R.top64(case(name)[0]["ids"])
    assert np.unique(k).size == k.size


def test_null_table_is_invalid():
    L = _lib.lib()
    buf = np.full(16, SENT, np.uint32)
    for q in (0, 1):
        assert L.kad_rt_closest_batch_packed(None, p(buf), q, 8, p(buf), p(buf), None) == _lib.KAD_ERR_INVALID
        assert L.kad_rt_closest_keys_packed(None, p(buf), q, 8, p(buf), p(buf), p(buf), None) == _lib.KAD_ERR_INVALID
    assert (buf == SENT).all()


# ---- the kernels --------------------------------------------------------------------------------------------------
def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class Dev:
    """One case on the GPU: its table, its targets and their keys."""

    def __init__(self, name, gpu):
        import torch

        t, tg, self.want, self.wcnt = case(name)
        self.name, self.gpu, self.tg = name, gpu, tg
        self.T = DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=0, sorted=t.get("sorted", False))
        self.targets = torch.from_numpy(tg.copy()).to(gpu)
        self.keys = torch.from_numpy(R.top64(tg).view(np.int64).copy()).to(gpu)

    def run(self, keys, sel=None, q=None, escape0=0):
        """One direct call on targets[sel][:q] from sentinel-filled rows and a zero tail word.
        Returns (packed words incl. 6 guard words, escape, tail, q)."""
        import torch

        L = _lib.lib()
        src = self.keys if keys else self.targets
        if sel is not None:
            src = src[torch.from_numpy(np.nonzero(sel)[0]).to(self.gpu)].contiguous()
        q = src.shape[0] if q is None else q
        packed = torch.from_numpy(np.full(3 * q + 6, SENT, np.uint32).view(np.int32)).to(self.gpu)
        esc = torch.full((1,), escape0, dtype=torch.int32, device=self.gpu)
        tail = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        if keys:
            rc = L.kad_rt_closest_keys_packed(self.T.handle, p(src), q, 8, p(packed), p(esc), p(tail), None)
        else:
            rc = L.kad_rt_closest_batch_packed(self.T.handle, p(src), q, 8, p(packed), p(esc), None)
        _lib.check(rc, "packed query")
        torch.cuda.synchronize()
        return _u32(packed), int(_u32(esc)[0]), int(_u32(tail)[0]), q


@pytest.fixture(scope="module", params=CASES)
def dev(request, gpu):
    d = Dev(request.param, gpu)
    yield d
    d.T.close()


def _compare(words, q, want, wcnt, where):
    """Rows the oracle says escape are untouched, every other row decodes to the oracle's, the guard is untouched."""
    esc = R.escapes_rows(want, wcnt)
    rows = words[:3 * q].reshape(q, 3)
    assert (rows[esc] == SENT).all(), f"{where}: a row that cannot be packed was written"
    got, gcnt = R.decode_rows(rows[~esc], 8)
    np.testing.assert_array_equal(gcnt, wcnt[~esc], err_msg=f"{where}: counts")
    np.testing.assert_array_equal(got, want[~esc], err_msg=f"{where}: rows")
    live = np.arange(8)[None, :] < wcnt[~esc][:, None]
    assert (np.where(live, want[~esc], R.NO_NODE) >= rows[~esc][:, :1]).all(), f"{where}: word 0 above an entry"
    assert (words[3 * q:] == SENT).all(), f"{where}: wrote past 3 * q words"
    return esc


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [False, True], ids=["targets", "keys"])
def test_packed_rows_against_the_oracle(dev, keys):
    assert dev.T.info()["flags"] & _lib.KAD_INFO_SHORT_LINES, "the fixture must carry short window lines"
    n = dev.tg.shape[0]
    for q in (n,) + tuple(x for x in PREFIXES if x < n):
        words, escape, tail, _ = dev.run(keys, q=q)
        where = f"{dev.name} {'keys' if keys else 'targets'} q={q}"
        esc = _compare(words, q, dev.want[:q], dev.wcnt[:q], where)
        assert (escape != 0) == bool(esc.any()), f"{where}: escape = {escape}, {int(esc.sum())} rows escape"
        assert tail == 0, f"{where}: a table of distinct top-64 bits set the tail word"


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [False, True], ids=["targets", "keys"])
def test_escape_is_sticky_and_never_spurious(dev, keys):
    """The batch of exactly the queries whose rows pack: escape stays 0 from 0 and stays 1 from 1, every row is
    written. The batch of exactly those that do not: nothing is written."""
    esc = R.escapes_rows(dev.want, dev.wcnt)
    where = f"{dev.name} {'keys' if keys else 'targets'}"
    if (~esc).any():
        for e0 in (0, 1):
            words, escape, tail, q = dev.run(keys, sel=~esc, escape0=e0)
            assert escape == e0 and tail == 0, f"{where}: escape {e0} -> {escape} on a batch that packs"
            _compare(words, q, dev.want[~esc], dev.wcnt[~esc], where + " packing rows")
    if esc.any():
        words, escape, tail, q = dev.run(keys, sel=esc)
        assert escape != 0 and tail == 0 and (words == SENT).all(), where + " escaping rows"


def _tie_case(name):
    """ties: tests/tables.py tie_table, every node in a group of 6 sharing its top 64 bits, so every window holds a
    tie. mixed: the same nodes among 4,000 of distinct top-64 bits, so that most windows hold none."""
    t = TB.tie_table()[0]
    if name == "mixed":
        from opendht_amd import synth as S

        ids, _ = S.sort_ids(np.concatenate([t["ids"], S.random_ids(4000, 0x71E5)]))
        st = np.where(np.random.default_rng(9).random(ids.shape[0]) < 0.85, 1, 0).astype(np.uint8)
        first, off = S.uniform_buckets(ids, 9)  # (~9 nodes per bucket: the lines answer most queries)
        t = TB.table(ids, st, first, off, sorted_=True, name="ties_mixed")
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties", "mixed"])
def test_key_only_ties_set_the_tail_word(gpu, name):
    """Nodes sharing their top 64 bits: a batch of targets equal to the tied heads must set the tail word, and a batch
    that leaves it zero must hold the oracle's rows (the rows of a batch that sets it are the caller's to answer
    again from full targets, and are not looked at). On `ties` every window holds a tie and a batch of 16 may never
    leave the word zero; on `mixed` some batch must, or the key-only rows went unchecked. From full targets the same
    batches never need a second answer."""
    import torch

    t = _tie_case(name)
    tied = TB.tie_table()[0]["ids"]
    _, n = np.unique(R.top64(t["ids"]), return_counts=True)
    assert n.max() >= 6 and ((n == 1).sum() >= 4000) == (name == "mixed")
    rng = np.random.default_rng(40)
    heads = tied[rng.integers(0, tied.shape[0], 300)].copy()
    heads[:, 8:] = rng.integers(0, 256, (300, 12), dtype=np.uint8)  # the tied heads with other tails
    tg = np.ascontiguousarray(np.concatenate([heads, TB.adversarial_targets(t, extra=2000, seed=0)]), np.uint8)
    want, wcnt = O.flat_rt_closest(t["ids"], t["status"], t["first"], t["off"], tg, 8, nthreads=8)
    assert not R.escapes_rows(want, wcnt).any()
    L = _lib.lib()
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=0, sorted=True) as T:
        assert T.info()["flags"] & _lib.KAD_INFO_SHORT_LINES
        keys = torch.from_numpy(R.top64(tg).view(np.int64).copy()).to(gpu)
        clean = 0
        for lo in [0] + list(range(300, tg.shape[0], 16)):
            q = 300 if lo == 0 else min(16, tg.shape[0] - lo)
            packed = torch.from_numpy(np.full(3 * q + 6, SENT, np.uint32).view(np.int32)).to(gpu)
            flags = torch.zeros(2, dtype=torch.int32, device=gpu)
            _lib.check(L.kad_rt_closest_keys_packed(T.handle, C.c_void_p(keys.data_ptr() + 8 * lo), q, 8, p(packed),
                                                    p(flags), C.c_void_p(flags.data_ptr() + 4), None), "keys_packed")
            torch.cuda.synchronize()
            escape, tail = _u32(flags).tolist()
            assert escape == 0
            if lo == 0:
                assert tail != 0, "targets equal to tied heads must ask for the full targets"
            if tail == 0:
                clean += 1
                _compare(_u32(packed), q, want[lo:lo + q], wcnt[lo:lo + q], f"{name} batch at {lo}")
        print(f"{name}: {clean} of {1 + len(range(300, tg.shape[0], 16))} key-only batches left the tail word zero")
        if name == "mixed":
            assert clean >= 1, "no batch left the tail word zero: the rows of the key-only path went unchecked"
        d = torch.from_numpy(tg).to(gpu)
        packed = torch.from_numpy(np.full(3 * tg.shape[0] + 6, SENT, np.uint32).view(np.int32)).to(gpu)
        flags = torch.zeros(1, dtype=torch.int32, device=gpu)
        _lib.check(L.kad_rt_closest_batch_packed(T.handle, p(d), tg.shape[0], 8, p(packed), p(flags), None), "packed")
        torch.cuda.synchronize()
        assert int(_u32(flags)[0]) == 0
        _compare(_u32(packed), tg.shape[0], want, wcnt, f"{name} from full targets")


@pytest.mark.gpu
def test_native_executor_flags_without_a_second_answer(gpu):
    """kad_route_run at world 1 without a communicator, called once per case through comm.NativeRoute.run (the bare
    binding: serve_native, which runs a flagged batch again, is not used): the four flag words of include/kadgpu.h
    after a single run, the rows of that single run, and the set's counters left zero. Edge table: batches of rows that
    all pack, and a batch holding one row that spans 255."""
    import torch

    from opendht_amd.comm import NativeRoute

    t, tg, want, wcnt = case("edge")
    esc = R.escapes_rows(want, wcnt)
    q = 600
    ok, bad = np.nonzero(~esc)[0], np.nonzero(esc & (R.spans_rows(want, wcnt) == 255))[0]
    clean = [ok[:q], ok[-q:][::-1].copy()]
    dirty = [ok[:q], np.concatenate([ok[:q - 1], bad[:1]])]
    need = R.SUBS * q  # one owner, one workgroup: every query in sub-block 0, and 8 sub-blocks of that size needed

    def run(sel, cap, packed, keys):
        # shard_bits 2: the owner answers its whole block, the padding records past each sub-block's count included
        # (sharded.pad_blocks: a target in the middle of the shard); theirs is then 20 00 .. 00 in bucket 2, whose row
        # spans 251 and packs (at shard_bits 0 it is 80 00 .. 00 in bucket 8, whose row spans 257)
        route = NativeRoute(q, 8, 1, 2, gpu, cap=cap, n_sets=1, packed=packed, keys=keys)
        assert route.cap == cap and route.packed == packed and route.keys == keys
        batches = [torch.from_numpy(tg[x].copy()).to(gpu) for x in sel]
        outs = [(torch.from_numpy(np.full((q, 8), SENT, np.uint32).view(np.int32)).to(gpu),
                 torch.full((q,), 0xA5, dtype=torch.uint8, device=gpu)) for _ in sel]
        route.run(T, batches, outs)
        torch.cuda.synchronize()
        assert not _u32(route.sets[0].ctr).any(), "the set's counters must be left zero"
        return _u32(route.acc).tolist(), [(_u32(o[0]).reshape(q, 8), o[1].cpu().numpy()) for o in outs]

    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=0, sorted=True) as T:
        for packed, keys in ((True, True), (True, False), (False, False)):
            where = f"packed {packed} keys {keys}"
            flags, outs = run(clean, need, packed, keys)
            assert flags == [0, 0, 0, need], f"{where}: flags {flags} after batches that fit, pack and need no low bits"
            for x, (oi, oc) in zip(clean, outs):
                np.testing.assert_array_equal(oc, wcnt[x], err_msg=where)
                np.testing.assert_array_equal(oi, want[x], err_msg=where)
            flags, outs = run(dirty, need, packed, keys)
            assert flags[0] == 0 and (flags[1] != 0) == packed and flags[2:] == [0, need], f"{where}: {flags}"
            if not packed:  # rows and counts travel whole: the row spanning 255 too
                for x, (oi, oc) in zip(dirty, outs):
                    np.testing.assert_array_equal(oc, wcnt[x], err_msg=where)
                    np.testing.assert_array_equal(oi, want[x], err_msg=where)
            flags, _ = run(clean, R.SUBS, packed, keys)  # blocks of one record per sub-block
            assert flags[0] != 0 and flags[3] == need, f"{where}: flags {flags} after blocks that overflow"


@pytest.mark.gpu
def test_error_returns_touch_nothing(gpu):
    """Every refusal of include/kadgpu.h, before any launch: the rows, escape and tail stay as they were."""
    import torch

    L = _lib.lib()
    INVALID, UNSUPPORTED = _lib.KAD_ERR_INVALID, _lib.KAD_ERR_UNSUPPORTED
    t, tg, _, _ = case("dense")
    s = TB.split_config(4000)
    q = 64
    d = torch.from_numpy(tg[:q + 1].copy()).to(gpu)
    keys = torch.from_numpy(R.top64(tg[:q + 1]).view(np.int64).copy()).to(gpu)
    packed = torch.from_numpy(np.full(3 * q + 6, SENT, np.uint32).view(np.int32)).to(gpu)
    flags = torch.zeros(2, dtype=torch.int32, device=gpu)
    esc, tail = p(flags), C.c_void_p(flags.data_ptr() + 4)

    def off(x, n):
        return C.c_void_p(x.data_ptr() + n)

    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=0, sorted=True) as T, \
            DeviceTable(s["ids"], s["status"], s["first"], s["off"], device=0) as S:
        assert T.info()["flags"] & _lib.KAD_INFO_SHORT_LINES and not S.info()["flags"] & _lib.KAD_INFO_SHORT_LINES
        h = T.handle
        for count in (0, 1, 7, 9, 14, 32):
            assert L.kad_rt_closest_batch_packed(h, p(d), q, count, p(packed), esc, None) == UNSUPPORTED
            assert L.kad_rt_closest_keys_packed(h, p(keys), q, count, p(packed), esc, tail, None) == UNSUPPORTED
        assert L.kad_rt_closest_batch_packed(S.handle, p(d), q, 8, p(packed), esc, None) == UNSUPPORTED
        assert L.kad_rt_closest_keys_packed(S.handle, p(keys), q, 8, p(packed), esc, tail, None) == UNSUPPORTED
        assert b"short window lines" in L.kad_last_error()
        for a in ((None, p(packed), esc), (p(d), None, esc), (p(d), p(packed), None),
                  (off(d, 1), p(packed), esc), (off(d, 2), p(packed), esc), (p(d), off(packed, 2), esc)):
            assert L.kad_rt_closest_batch_packed(h, a[0], q, 8, a[1], a[2], None) == INVALID
        for a in ((None, p(packed), esc, tail), (p(keys), None, esc, tail), (p(keys), p(packed), None, tail),
                  (p(keys), p(packed), esc, None), (off(keys, 4), p(packed), esc, tail),
                  (p(keys), off(packed, 1), esc, tail)):
            assert L.kad_rt_closest_keys_packed(h, a[0], q, 8, a[1], a[2], a[3], None) == INVALID
        # q = 0 is KAD_OK, with or without buffers, and launches nothing
        assert L.kad_rt_closest_batch_packed(h, p(d), 0, 8, p(packed), esc, None) == 0
        assert L.kad_rt_closest_batch_packed(h, None, 0, 8, None, None, None) == 0
        assert L.kad_rt_closest_keys_packed(h, p(keys), 0, 8, p(packed), esc, tail, None) == 0
        assert L.kad_rt_closest_keys_packed(h, None, 0, 8, None, None, None, None) == 0
        torch.cuda.synchronize()
        assert (_u32(packed) == SENT).all() and _u32(flags).tolist() == [0, 0]
