"""Storage-responsibility verdicts (kad_rt_responsible_batch): Dht::maintainStorage and
Dht::onAnnounce ask of findClosestNodes(h, now, count) only whether its last node is closer to h than self_id.

Expected bytes come from the oracle's rows and counts plus a big-integer xor compare done here. Random targets
against a random self_id are almost always "far", so every batch also holds, for each self_id and each c in
0..159, 8 targets sharing exactly c leading bits with it, and self_id itself: those put self_id inside the
answer's window, where no line decides and the kernel has to load the node's key (and, on the tie tables, its
tail). Every case with count <= 8 that can hold both verdicts must hold at least 32 of each before anything is
compared. A case cannot hold a "far" when fewer than max(min_nodes, 1) nodes can come back (empty,
one_empty_bucket and all_bad always; S1 and S3 with min_nodes 8; any table with count < min_nodes) or when
self_id is a good node and the count takes every good node (S1, S3 with self_id one of theirs): there the
expected bytes must be all zero instead. Checked with the oracle alone: every other case of the tables below
holds both verdicts at least 32 times.
"""
import functools

import numpy as np
import pytest
import torch

import oracle as O
import tables as TB
from opendht_amd import DeviceTable, rt_responsible_dual
from opendht_amd import synth as S
from opendht_amd._lib import KAD_INFO_SHORT_LINES, KAD_INFO_SLOT_LINES

pytestmark = pytest.mark.gpu

COUNTS = (1, 5, 8, 14, 32)
MIN_NODES = (1, 8)
NAMES = ("empty", "one_empty_bucket", "S1", "S3", "S50", "S257", "S10000", "U10_10000", "all_bad", "sparse_good",
         "ties", "dups", "ties48", "dups48", "offset_first", "collisions")
ALL_ZERO = ("empty", "one_empty_bucket", "all_bad")  # no good node
SELF = np.random.default_rng(0x5E1F).integers(0, 256, size=20, dtype=np.uint8)  # drawn once


def _collision_table(n=40_000, depth=10, keys_per_bucket=3, seed=0xC011):
    """The recipe of test_short_lines._collision_table: U(depth) whose nodes take ID bits [depth, depth+16) from a
    few values per bucket (fallback short lines), a quarter of them tying on all 21 line key bits (exact path)."""
    rng = np.random.default_rng(seed)
    ids = S.random_ids(n, seed)
    hi = np.frombuffer(ids[:, :8].tobytes(), dtype=">u8").astype(np.uint64)
    bucket = hi >> np.uint64(64 - depth)
    vals = rng.integers(0, 1 << 16, size=(1 << depth, keys_per_bucket), dtype=np.uint64)
    pick = vals[bucket.astype(np.int64), rng.integers(0, keys_per_bucket, size=n)]
    sh = np.uint64(64 - depth - 16)
    hi = (hi & ~(np.uint64(0xFFFF) << sh)) | (pick << sh)
    tie = rng.random(n) < 0.25
    sh5 = np.uint64(64 - depth - 21)
    hi = np.where(tie, (hi & ~(np.uint64(0x1F) << sh5)) | ((bucket & np.uint64(0x1F)) << sh5), hi)
    ids = ids.copy()
    ids[:, :8] = np.frombuffer(hi.astype(">u8").tobytes(), dtype=np.uint8).reshape(n, 8)
    ids, _ = S.sort_ids(ids)
    st = S.random_status(n, S.SEED_STATUS ^ seed, 80, 10)
    first, off = S.uniform_buckets(ids, depth)
    return TB.table(ids, st, first, off, sorted_=True, name="collisions")


@functools.lru_cache(maxsize=None)
def _tables():
    ts = {t["name"]: t for t in TB.all_small_tables()}
    ts["collisions"] = _collision_table()
    assert set(ts) == set(NAMES), set(ts) ^ set(NAMES)
    return ts


def near_targets(self_id, rng, copies=8):
    """For each c in 0..159, `copies` targets sharing exactly c leading bits with self_id, then self_id."""
    s = int.from_bytes(self_id.tobytes(), "big")
    out = []
    for c in range(160):
        low = 159 - c
        for _ in range(copies):
            r = int.from_bytes(rng.bytes(20), "big") & ((1 << low) - 1)
            out.append(((((s >> low) ^ 1) << low) | r).to_bytes(20, "big"))
    out.append(s.to_bytes(20, "big"))
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 20)


def self_ids(t):
    """The random self_id; on tables with a good node, that node's ID (the equality case); on the tie and
    duplicate tables, an ID sharing its first 8 bytes with a node group (the tail compare decides)."""
    out = [SELF]
    good = np.flatnonzero(t["status"] & 1)
    if good.size:
        out.append(t["ids"][good[good.size // 2]].copy())
    if t["name"].startswith(("ties", "dups")):
        s = t["ids"][t["ids"].shape[0] // 3].copy()
        s[8:] = np.random.default_rng(11).integers(0, 256, size=12, dtype=np.uint8)
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _batch(name):
    t = _tables()[name]
    rng = np.random.default_rng(0xBA7C)
    parts = [TB.adversarial_targets(t, extra=2048)] + [near_targets(s, rng) for s in self_ids(t)]
    targets = np.ascontiguousarray(np.concatenate(parts), np.uint8)
    targets.setflags(write=False)
    return targets


@functools.lru_cache(maxsize=None)
def _rows(name, count):
    t = _tables()[name]
    return O.flat_rt_closest(t["ids"], t["status"], t["first"], t["off"], _batch(name), count, nthreads=8)


def expected(ids, targets, rows, cnt, self_id, min_nodes):
    """far = n >= max(min_nodes, 1) and (id(R[n-1]) ^ h) < (self_id ^ h), as 160-bit integers."""
    s = int.from_bytes(self_id.tobytes(), "big")
    out = np.zeros(targets.shape[0], np.uint8)
    need = max(min_nodes, 1)
    for i in range(targets.shape[0]):
        n = int(cnt[i])
        if n < need:
            continue
        h = int.from_bytes(targets[i].tobytes(), "big")
        a = int.from_bytes(ids[rows[i, n - 1]].tobytes(), "big")
        out[i] = 1 if (a ^ h) < (s ^ h) else 0
    return out


def want_of(name, count, self_id, min_nodes):
    t = _tables()[name]
    rows, cnt = _rows(name, count)
    w = expected(t["ids"], _batch(name), rows, cnt, self_id, min_nodes)
    good = t["ids"][(t["status"] & 1) != 0]
    need = max(min_nodes, 1)
    # no "far" can exist: fewer than `need` nodes can come back, or self_id is a good node and every good node
    # comes back (the last one is then self_id itself or a node farther than it)
    forced = good.shape[0] < need or count < need or (count >= good.shape[0] and (good == self_id).all(1).any())
    assert forced or name not in ALL_ZERO
    if forced:
        assert not w.any(), f"{name} k={count} min={min_nodes}: a far verdict where none can be"
    elif count <= 8:
        ones = int(w.sum())
        assert ones >= 32 and w.size - ones >= 32, f"{name} k={count} min={min_nodes}: {ones} far of {w.size}"
    return w


def _make(t, gpu, **kw):
    return DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, sorted=t["sorted"], **kw)


@pytest.mark.parametrize("name", NAMES)
def test_verdicts(gpu, name, monkeypatch):
    """Every count and threshold on every table: the default kernels (one line per query for count <= 8 where the
    table has short or slot lines, a wave per query otherwise), the wave-per-query kernel forced for count <= 8
    (KAD_RT_KERNEL=lane), and the host-pointer call, all equal to the expected bytes."""
    t = _tables()[name]
    targets = _batch(name)
    tg = torch.from_numpy(targets.copy()).to(gpu)
    with _make(t, gpu) as T:
        for sid in self_ids(t):
            for k in COUNTS:
                for mn in MIN_NODES:
                    want = want_of(name, k, sid, mn)
                    got = T.rt_responsible(tg, sid, k, mn)
                    torch.cuda.synchronize()
                    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{name} k={k} min={mn}")
                    if k <= 8:
                        monkeypatch.setenv("KAD_RT_KERNEL", "lane")
                        got2 = T.rt_responsible(tg, sid, k, mn)
                        monkeypatch.delenv("KAD_RT_KERNEL")
                        torch.cuda.synchronize()
                        np.testing.assert_array_equal(got2.cpu().numpy(), want, err_msg=f"{name} k={k} min={mn} wave")
            for k, mn in ((8, 1), (14, 8)):
                np.testing.assert_array_equal(T.rt_responsible_host(targets, sid, k, mn), want_of(name, k, sid, mn),
                                              err_msg=f"{name} k={k} min={mn} host")
        assert np.array_equal(T.rt_responsible(tg, SELF, 0, 1).cpu().numpy(), np.zeros(targets.shape[0], np.uint8))


def test_line_kernels_in_use(gpu):
    """The tables above reach both line forms: short lines on the uniform ones, slot lines on the split ones."""
    with _make(_tables()["U10_10000"], gpu) as T:
        assert T.info()["flags"] & KAD_INFO_SHORT_LINES
    with _make(_tables()["S10000"], gpu) as T:
        assert T.info()["flags"] & KAD_INFO_SLOT_LINES


@pytest.mark.parametrize("count,min_nodes", [(8, 1), (14, 8)])
def test_dual(gpu, count, min_nodes):
    """Both families answer every target: a U(9) v4 table and a split v6 table, then either one missing."""
    t4 = TB.uniform_config(5000, 9, seed=0xD4)
    t6 = TB.split_config(3000, seed=0xD6)
    rng = np.random.default_rng(0xD0A1)
    targets = np.ascontiguousarray(np.concatenate([TB.adversarial_targets(t4, extra=1024),
                                                   TB.adversarial_targets(t6, extra=64), near_targets(SELF, rng)]))
    tg = torch.from_numpy(targets).to(gpu)
    want = []
    for t in (t4, t6):
        rows, cnt = O.flat_rt_closest(t["ids"], t["status"], t["first"], t["off"], targets, count, nthreads=8)
        want.append(expected(t["ids"], targets, rows, cnt, SELF, min_nodes))
    assert min(want[0].sum(), (1 - want[0]).sum(), want[1].sum(), (1 - want[1]).sum()) >= 32
    with _make(t4, gpu) as T4, _make(t6, gpu) as T6:
        one4 = T4.rt_responsible(tg, SELF, count, min_nodes).cpu().numpy()
        one6 = T6.rt_responsible(tg, SELF, count, min_nodes).cpu().numpy()
        np.testing.assert_array_equal(one4, want[0])
        np.testing.assert_array_equal(one6, want[1])
        both = rt_responsible_dual(T4, T6, tg, SELF, count, min_nodes).cpu().numpy()
        np.testing.assert_array_equal(both, one4 | (one6 << 1))
        np.testing.assert_array_equal(rt_responsible_dual(T4, None, tg, SELF, count, min_nodes).cpu().numpy(), one4)
        np.testing.assert_array_equal(rt_responsible_dual(None, T6, tg, SELF, count, min_nodes).cpu().numpy(),
                                      one6 << 1)


def test_index_base(gpu, monkeypatch):
    """A shard's rows carry index_base; the verdict subtracts it before reading the node's key and tail."""
    name = "U10_10000"
    t = _tables()[name]
    tg = torch.from_numpy(_batch(name).copy()).to(gpu)
    with _make(t, gpu, index_base=0x7FFF0000) as T:
        for k in (8, 14):
            want = want_of(name, k, SELF, 1)
            np.testing.assert_array_equal(T.rt_responsible(tg, SELF, k, 1).cpu().numpy(), want)
        monkeypatch.setenv("KAD_RT_KERNEL", "lane")
        got = T.rt_responsible(tg, SELF, 8, 1).cpu().numpy()
        monkeypatch.delenv("KAD_RT_KERNEL")
        np.testing.assert_array_equal(got, want_of(name, 8, SELF, 1))


@pytest.mark.parametrize("name", ["U10_10000", "S10000"])
def test_after_status_patch(gpu, name):
    """A verdict taken after patch_status follows the new snapshot."""
    t = _tables()[name]
    targets = _batch(name)
    tg = torch.from_numpy(targets.copy()).to(gpu)
    rng = np.random.default_rng(5)
    st = t["status"].copy()
    with _make(t, gpu) as T:
        before = T.rt_responsible(tg, SELF, 8, 1).cpu().numpy()
        nodes = rng.choice(st.shape[0], size=st.shape[0] // 2, replace=False).astype(np.uint32)
        st[nodes] = rng.choice(np.array([0, 2], np.uint8), size=nodes.shape[0])
        T.patch_status(nodes, st[nodes])
        for k in (8, 14):
            rows, cnt = O.flat_rt_closest(t["ids"], st, t["first"], t["off"], targets, k, nthreads=8)
            want = expected(t["ids"], targets, rows, cnt, SELF, 1)
            np.testing.assert_array_equal(T.rt_responsible(tg, SELF, k, 1).cpu().numpy(), want)
            if k == 8:
                assert (want != before).sum() >= 32, "the patch changed too few verdicts to show anything"


def test_two_streams(gpu):
    """Const queries without table-held scratch: two calls in flight on two streams give the same bytes."""
    name = "S10000"
    t = _tables()[name]
    tg = torch.from_numpy(_batch(name).copy()).to(gpu)
    want = want_of(name, 8, SELF, 1)
    with _make(t, gpu) as T:
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        a = torch.empty(tg.shape[0], dtype=torch.uint8, device=gpu)
        b = torch.empty(tg.shape[0], dtype=torch.uint8, device=gpu)
        for _ in range(4):
            T.rt_responsible(tg, SELF, 8, 1, out=a, stream=s1)
            T.rt_responsible(tg, SELF, 8, 1, out=b, stream=s2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(a.cpu().numpy(), want)
        np.testing.assert_array_equal(b.cpu().numpy(), want)
