"""kad_table_touch_buckets (Dht::onReportedAddr per ID) and kad_table_patch_bucket_times on the GPU, against the
yardstick of tests/maint_ref.py: findBucket as the reference's linear walk, one ID at a time."""
import numpy as np
import pytest
import torch

import maint_ref as R
import tables as TB
from opendht_amd import DeviceTable, KadError
from opendht_amd import _lib

NOW = 10**15
_CACHE = {}


def kinds():
    """name -> (table, DeviceTable keywords, the kad_table_info flag it must show or 0)."""
    if not _CACHE:
        u = TB.uniform_config(2000, 8)
        s = TB.split_config(2000)
        _CACHE["direct"] = (u, {}, _lib.KAD_INFO_WINDOW_LINES)
        _CACHE["slot_lines"] = (s, {}, _lib.KAD_INFO_SLOT_LINES)
        _CACHE["split"] = (s, {"slot_lines": False}, 0)
    return _CACHE


def pool(t):
    """5000 IDs: the all-zero and the all-ones ID, 300 IDs inside one bucket, every bucket's first and the ID just
    below it, random ones; shuffled with a fixed seed, so a short prefix holds some of each kind."""
    key = "pool_" + t["name"]
    if key not in _CACHE:
        first = t["first"]
        B = first.shape[0]
        assert 2 + 300 + 2 * B < 5000
        rng = np.random.default_rng(0x70C)
        b = B // 2
        one = np.repeat(first[b][None, :], 300, axis=0).copy()
        one[:, 12:] = rng.integers(0, 256, size=(300, 8), dtype=np.uint8)  # the low bytes: still bucket b
        parts = [np.zeros((1, 20), np.uint8), np.full((1, 20), 255, np.uint8), one, first, TB._minus_one(first)]
        m = sum(p.shape[0] for p in parts)
        parts.append(rng.integers(0, 256, size=(5000 - m, 20), dtype=np.uint8))
        ids = np.concatenate(parts)
        perm = rng.permutation(5000)
        perm = np.concatenate([[0, 1], perm[perm >= 2]])  # the two extreme IDs stay in front
        _CACHE[key] = np.ascontiguousarray(ids[perm])
        _, bk = R.touch(first, np.zeros(B, np.int64), _CACHE[key], 1)
        assert (bk == b).sum() >= 300 and np.unique(bk).shape[0] == B
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("q", [0, 1, 63, 64, 65, 5000])
@pytest.mark.parametrize("kind", ["direct", "slot_lines", "split"])
def test_touch(gpu, kind, q):
    t, kw, flag = kinds()[kind]
    B = t["first"].shape[0]
    ids = pool(t)[:q]
    tm = R.draw_times(B, NOW - 10**12, 0x33)
    want_tm, want_b = R.touch(t["first"], tm, ids, NOW)
    assert (want_tm != tm).sum() == np.unique(want_b).shape[0]
    tg = torch.from_numpy(ids).to(gpu)
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, **kw) as T:
        assert (T.info()["flags"] & flag) == flag
        T.set_bucket_times(tm)
        out = T.touch_buckets(tg, NOW)
        fb = T.find_bucket(tg)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want_b)
        assert torch.equal(out, fb)
        np.testing.assert_array_equal(T.bucket_times(), want_tm)
        # without out_bucket, a later time: the same buckets move again
        assert T.touch_buckets(tg, NOW + 7, want_bucket=False) is None
        np.testing.assert_array_equal(T.bucket_times(), R.touch(t["first"], want_tm, ids, NOW + 7)[0])
        # the host form on the same start
        T.set_bucket_times(tm)
        hb = T.touch_buckets(ids, NOW)
        np.testing.assert_array_equal(hb, want_b)
        np.testing.assert_array_equal(T.bucket_times(), want_tm)


@pytest.mark.gpu
def test_touch_allocates_on_first_use(gpu):
    t, kw, _ = kinds()["slot_lines"]
    ids = pool(t)[:65]
    B = t["first"].shape[0]
    want_tm, want_b = R.touch(t["first"], np.full(B, R.INT64_MIN, np.int64), ids, NOW)
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0) as T:
        np.testing.assert_array_equal(T.touch_buckets(ids, NOW), want_b)
        np.testing.assert_array_equal(T.bucket_times(), want_tm)
        # two touches on two streams in a row are ordered by the table: the later `now` stays
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        tg = torch.from_numpy(ids).to(gpu)
        torch.cuda.synchronize()
        T.touch_buckets(tg, NOW + 1, stream=s1)
        T.touch_buckets(tg, NOW + 2, stream=s2)
        np.testing.assert_array_equal(T.bucket_times(), R.touch(t["first"], want_tm, ids, NOW + 2)[0])


@pytest.mark.gpu
def test_patch(gpu):
    t, kw, _ = kinds()["direct"]
    B = t["first"].shape[0]
    tm = R.draw_times(B, NOW, 0x44)
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0) as T:
        # on a table without times: the others stay at INT64_MIN
        T.patch_bucket_times([3], [33])
        want = np.full(B, R.INT64_MIN, np.int64)
        want[3] = 33
        np.testing.assert_array_equal(T.bucket_times(), want)
        T.set_bucket_times(tm)
        # the later entry of a bucket listed twice wins, wherever the two stand
        b = np.array([5, 0, 5, B - 1, 7, 0, 5], np.uint32)
        v = np.array([10, 20, 30, 40, R.INT64_MIN, 60, 70], np.int64)
        T.patch_bucket_times(b, v)
        want = tm.copy()
        for x, y in zip(b, v):
            want[x] = y
        assert want[5] == 70 and want[0] == 60
        np.testing.assert_array_equal(T.bucket_times(), want)
        # 600 entries over 9 buckets (more than one workgroup of entries before the duplicates are dropped)
        rng = np.random.default_rng(9)
        b = rng.integers(0, 9, size=600).astype(np.uint32)
        v = rng.integers(0, 10**15, size=600).astype(np.int64)
        T.patch_bucket_times(b, v)
        for x, y in zip(b, v):
            want[x] = y
        np.testing.assert_array_equal(T.bucket_times(), want)
        # an index out of range: refused, nothing written (the entries before it neither)
        with pytest.raises(KadError) as e:
            T.patch_bucket_times([1, B, 2], [1, 2, 3])
        assert "INVALID" in str(e.value) and f"bucket {B} (entry 1)" in str(e.value)
        np.testing.assert_array_equal(T.bucket_times(), want)
        T.patch_bucket_times([], [])
        np.testing.assert_array_equal(T.bucket_times(), want)


@pytest.mark.gpu
def test_no_buckets_is_refused(gpu):
    t = TB.uniform_config(500, 4)
    tg = torch.from_numpy(t["ids"][:8].copy()).to(gpu)
    with DeviceTable(t["ids"], t["status"], None, None, device=gpu.index or 0, sorted=True) as T:
        for ids in (tg, t["ids"][:8], tg[:0]):
            with pytest.raises(KadError) as e:
                T.touch_buckets(ids, NOW)
            assert "INVALID" in str(e.value) and "RoutingTable" in str(e.value)
        assert T.bucket_times().shape == (0,)
        T.set_bucket_times(None)
        got = T.maintenance(NOW)
        assert got["totals"] == dict(candidates=0, stale=0, empty=0, sure=0, maybe=0, never=0, first_sure=0xFFFFFFFF,
                                     reserved=0)
        assert got["records"].shape[0] == 0
        assert T.maintenance_host(NOW)["totals"] == got["totals"]
