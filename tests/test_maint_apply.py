"""The bucket times across kad_table_apply and kad_table_expire on the GPU: REMOVE, REPLACE and INSERT leave them, a
SPLIT gives the new bucket the split bucket's time (routing_table.cpp:149). After every batch the device's times must
equal the yardstick's (tests/maint_ref.py: the split rule applied op by op), and, as a second derivation, every new
bucket's time must be that of the old bucket its first lies in (the reference's linear findBucket on the old firsts)."""
import numpy as np
import pytest

import maint_ref as R
import mutation_model as M
import tables as TB
from opendht_amd import DeviceTable, maint_scan_host
from opendht_amd._lib import KAD_OP_INSERT, KAD_OP_REMOVE, KAD_OP_REPLACE, KAD_OP_SPLIT

NOW = 10**15


def _state(T):
    ids, st, first, off = T.export()
    return TB.table(ids, st, first, off)


def _distinct_times(B, seed):
    """Every bucket its own time (a swapped pair would show), a few at INT64_MIN."""
    rng = np.random.default_rng(seed)
    tm = (NOW - rng.permutation(B).astype(np.int64) * 10**9).astype(np.int64)
    tm[rng.integers(0, B, size=max(1, B // 16))] = R.INT64_MIN
    return tm


def _apply_and_check(T, tm, ops, new_ids=None, new_st=None):
    before = _state(T)
    T.apply(ops, new_ids, new_st)
    want = R.apply_times(tm, ops)
    got = T.bucket_times()
    np.testing.assert_array_equal(got, want)
    after = _state(T)
    assert after["first"].shape[0] == want.shape[0] == before["first"].shape[0] + int((ops[:, 0] == KAD_OP_SPLIT).sum())
    src = [R.find_bucket(before["first"], f) for f in after["first"]]
    np.testing.assert_array_equal(got, np.asarray(tm)[src])
    # and the scan reads them
    twin = maint_scan_host(after["off"], after["first"], want, NOW)
    dev = T.maintenance_host(NOW)
    assert dev["totals"] == twin["totals"] and dev["records"].tobytes() == twin["records"].tobytes()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["split", "uniform"])
def test_times_follow_apply(gpu, shape):
    t = TB.split_config(2000) if shape == "split" else TB.uniform_config(2000, 6)
    rng = np.random.default_rng(0xA9 + len(shape))
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0) as T:
        tm = _distinct_times(T.B, 1)
        T.set_bucket_times(tm)
        # a batch without a split: the same array
        ops, nid, nst = M.random_ops(_state(T), rng, 60, allow_split=False)
        assert {KAD_OP_REMOVE, KAD_OP_REPLACE, KAD_OP_INSERT} <= set(int(k) for k in ops[:, 0])
        tm = _apply_and_check(T, tm, ops, nid, nst)
        # mixed batches with splits anywhere
        for _ in range(2):
            ops, nid, nst = M.random_ops(_state(T), rng, 120)
            assert (ops[:, 0] == KAD_OP_SPLIT).sum() >= 3 and (ops[:, 0] != KAD_OP_SPLIT).sum() >= 60
            tm = _apply_and_check(T, tm, ops, nid, nst)
        # the first bucket, the last bucket, and a freshly split bucket (both halves of it again)
        B = T.B
        a = B // 2
        ops = np.array([[KAD_OP_SPLIT, 0, 0], [KAD_OP_SPLIT, B, 0], [KAD_OP_SPLIT, a, 0], [KAD_OP_SPLIT, a + 1, 0],
                        [KAD_OP_SPLIT, a, 0]], np.uint32)
        tm = _apply_and_check(T, tm, ops)
        assert T.B == B + 5
        assert tm[0] == tm[1] and tm[-1] == tm[-2] and len(set(tm[a:a + 4].tolist())) == 1
        # the same three inside a batch that also inserts, replaces and removes
        ops2, nid, nst = M.random_ops(_state(T), rng, 40, allow_split=False)
        B = T.B
        ops = np.concatenate([np.array([[KAD_OP_SPLIT, B - 1, 0]], np.uint32), ops2[:20],
                              np.array([[KAD_OP_SPLIT, 0, 0], [KAD_OP_SPLIT, 1, 0]], np.uint32), ops2[20:]])
        tm = _apply_and_check(T, tm, ops, nid, nst)
        # kad_table_expire changes no bucket
        st = T.export_status()
        assert (st & 2).any()
        removed, _ = T.expire()
        assert removed.shape[0] == int(((st & 2) != 0).sum()) > 0
        np.testing.assert_array_equal(T.bucket_times(), tm)
        # and a touch after all of that lands in the new bucket list
        after = _state(T)
        ids = after["first"][[0, 1, T.B // 2, T.B - 1]]
        want, wb = R.touch(after["first"], tm, ids, NOW + 5)
        np.testing.assert_array_equal(T.touch_buckets(ids, NOW + 5), wb)
        np.testing.assert_array_equal(T.bucket_times(), want)


@pytest.mark.gpu
def test_apply_without_times_leaves_none(gpu):
    t = TB.split_config(2000)
    rng = np.random.default_rng(0x1E)
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0) as T:
        ops, nid, nst = M.random_ops(_state(T), rng, 120)
        assert (ops[:, 0] == KAD_OP_SPLIT).sum() >= 3
        T.apply(ops, nid, nst)
        T.expire()
        assert (T.bucket_times() == R.INT64_MIN).all() and T.bucket_times().shape == (T.B,)
        after = _state(T)
        want = R.scan(after["off"], after["first"], None, NOW)
        got = T.maintenance_host(NOW)
        assert got["totals"] == want["totals"] and got["records"].tobytes() == want["records"].tobytes()
        # no array was made on the way: reading the times and scanning did not add one either, setting them does
        bytes1 = T.info()["device_bytes"]
        T.set_bucket_times(None)
        assert T.info()["device_bytes"] == bytes1
        T.set_bucket_times(np.zeros(T.B, np.int64))
        assert T.info()["device_bytes"] >= bytes1 + 8 * T.B
