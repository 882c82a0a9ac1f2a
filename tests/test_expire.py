"""kad_table_expire on the GPU: Dht::expireBuckets (dht.cpp:942-956) on the device copy. The table that results equals
the oracle's std::list table after one REMOVE per expired node, and a twin table given the same ops through
kad_table_apply; unlike apply, the node times and wire records stay attached to the survivors."""
import numpy as np
import pytest
import torch

import oracle as O
import sweep_ref as R
import tables as TB
from opendht_amd import DeviceTable, KadError
from opendht_amd._lib import KAD_TABLE_SORTED

TABLES = {t["name"]: t for t in R.small_tables()}
NAMES = ["S50", "S10000", "U10_10000", "sparse_good", "U4_2000exp", "offset_first", "S257good", "one_empty_bucket"]
LINESETS = range(13)


def _open(t, gpu, **kw):
    return DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, sorted=t["sorted"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_expire_parity(gpu, name):
    t = TABLES[name]
    want = R.sweep_ref(t)
    w_ids, w_st, w_first, w_off, w_remap, ops = R.expire_ref(t)
    n0 = t["status"].shape[0]
    if name == "U4_2000exp":
        assert w_ids.shape[0] == 0 and (np.diff(w_off.astype(np.int64)) == 0).sum() == 16
    with _open(t, gpu) as T, _open(t, gpu) as twin:
        remap = torch.full((max(n0, 1),), 0x55555555, dtype=torch.int32, device=gpu)
        removed, buckets = T.expire(remap=remap)
        np.testing.assert_array_equal(removed, want["expired_nodes"])
        np.testing.assert_array_equal(buckets, want["changed_buckets"])
        np.testing.assert_array_equal(remap.cpu().numpy().view(np.uint32)[:n0], w_remap)
        ids, st, first, off = T.export()
        np.testing.assert_array_equal(first, w_first)
        np.testing.assert_array_equal(off, w_off)
        np.testing.assert_array_equal(ids, w_ids)
        np.testing.assert_array_equal(st, w_st)
        assert T.n == w_ids.shape[0] and T.info()["n_good"] == int((w_st & 1).sum())
        # queries on the shrunk table
        cur = dict(t, ids=w_ids, status=w_st, first=w_first, off=w_off)
        targets = TB.adversarial_targets(cur)
        idx, cnt = T.rt_closest(torch.from_numpy(targets).to(gpu), 8)
        torch.cuda.synchronize()
        w_idx, w_cnt = O.flat_rt_closest(w_ids, w_st, w_first, w_off, targets, 8)
        np.testing.assert_array_equal(cnt.cpu().numpy(), w_cnt)
        np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint32), w_idx)
        # the twin through kad_table_apply: the same arrays and the same derived sets
        if ops.shape[0]:
            twin.apply(ops)
        for a, b in zip(T.export(), twin.export()):
            np.testing.assert_array_equal(a, b)
        ia, ib = T.info(), twin.info()
        assert (ia["flags"], ia["n_good"], ia["n_nodes"], ia["n_buckets"]) == (ib["flags"], ib["n_good"], ib["n_nodes"],
                                                                                ib["n_buckets"])
        for which in LINESETS:
            a, b = T.export_lines(which), twin.export_lines(which)
            if a is not None and b is not None:
                np.testing.assert_array_equal(a, b, err_msg=f"line set {which}")
        # a second expire in a row changes nothing
        before = (T.info(), T.export(), [T.export_lines(w) for w in LINESETS])
        removed2, buckets2 = T.expire()
        assert removed2.shape[0] == 0 and buckets2.shape[0] == 0
        after = (T.info(), T.export(), [T.export_lines(w) for w in LINESETS])
        assert before[0] == after[0]
        for a, b in zip(before[1] + tuple(x for x in before[2] if x is not None),
                        after[1] + tuple(x for x in after[2] if x is not None)):
            np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_apply_large_removals_only_batch(gpu):
    """Plain kad_table_apply with ascending REMOVE rows alone takes the removals-only form of the host plan: a batch of
    ~12 000 removals over 8192 buckets (empty ones, untouched runs, emptied buckets) against the oracle's list table,
    and the same rows in another order (the general form of the plan) on a twin."""
    t = TB.uniform_config(40_000, 13, seed=0xA991, good=60, expired=30)
    w_ids, w_st, w_first, w_off, w_remap, ops = R.expire_ref(t)
    per = R.sweep_ref(t)
    assert ops.shape[0] >= 10_000 and ((per["per_bucket"] == per["width"]) & (per["width"] > 0)).sum() >= 100
    assert (per["per_bucket"] == 0).sum() >= 1000 and per["totals"]["empty_buckets"] >= 10
    n0 = t["status"].shape[0]
    with _open(t, gpu) as T, _open(t, gpu) as twin:
        remap = torch.empty(n0, dtype=torch.int32, device=gpu)
        T.apply(ops, remap=remap)
        twin.apply(ops[::-1].copy())
        got = T.export()
        for a, b in zip(got, (w_ids, w_st, w_first, w_off)):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(remap.cpu().numpy().view(np.uint32), w_remap)
        for a, b in zip(got, twin.export()):
            np.testing.assert_array_equal(a, b)
        for which in LINESETS:
            a, b = T.export_lines(which), twin.export_lines(which)
            if a is not None and b is not None:
                np.testing.assert_array_equal(a, b, err_msg=f"line set {which}")
        cur = dict(t, ids=w_ids, status=w_st, first=w_first, off=w_off)
        targets = TB.adversarial_targets(cur, extra=2048)
        idx, cnt = T.rt_closest(torch.from_numpy(targets).to(gpu), 8)
        torch.cuda.synchronize()
        w_idx, w_cnt = O.flat_rt_closest(w_ids, w_st, w_first, w_off, targets, 8)
        np.testing.assert_array_equal(cnt.cpu().numpy(), w_cnt)
        np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint32), w_idx)


@pytest.mark.gpu
def test_nothing_expired_keeps_the_table(gpu):
    """S257good holds no expired node: info, every exported array and KAD_TABLE_SORTED stay; the remap is the
    identity."""
    for t in (TABLES["S257good"], dict(TB.uniform_config(3000, 6, good=90, expired=0), name="U6good")):
        assert R.sweep_ref(t)["totals"]["expired"] == 0
        n0 = t["status"].shape[0]
        with _open(t, gpu) as T:
            before = (T.info(), T.export(), [T.export_lines(w) for w in LINESETS])
            remap = np.full(n0, 0x55555555, np.uint32)
            removed, buckets = T.expire(remap=remap)
            assert removed.shape[0] == 0 and buckets.shape[0] == 0
            np.testing.assert_array_equal(remap, np.arange(n0, dtype=np.uint32))
            after = (T.info(), T.export(), [T.export_lines(w) for w in LINESETS])
            assert before[0] == after[0]
            assert bool(after[0]["flags"] & KAD_TABLE_SORTED) == t["sorted"]
            for a, b in zip(before[1], after[1]):
                np.testing.assert_array_equal(a, b)
            for a, b in zip(before[2], after[2]):
                assert (a is None) == (b is None)
                if a is not None:
                    np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_times_are_carried(gpu):
    """set_times, refresh, expire, refresh at a later now without a new set_times: the survivors' statuses are
    isGood / isExpired restated from their own times. Through kad_table_apply the same sequence fails with
    "kad_table_set_times was not called": the node times do not survive it."""
    t = TABLES["S10000"]
    n = t["status"].shape[0]
    now = 10**13
    time_ns, reply_ns, expired = R.draw_times(n, 0xE791, now)
    st = R.status_at(time_ns, reply_ns, expired, now)
    keep = (st & 2) == 0
    assert 1000 <= (~keep).sum() <= n - 1000
    now2 = now + 3 * R.NODE_EXPIRE_NS // 4  # some good nodes have gone dubious by then
    st2 = R.status_at(time_ns[keep], reply_ns[keep], expired[keep], now2)
    assert ((st2 & 1) != (st[keep] & 1)).sum() >= 100
    with _open(t, gpu) as T, _open(t, gpu) as twin:
        for X in (T, twin):
            X.set_times(time_ns, reply_ns, expired)
            X.refresh_status(now)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(T.export_status(), st)
        removed, _ = T.expire()
        np.testing.assert_array_equal(removed, np.flatnonzero(~keep).astype(np.uint32))
        np.testing.assert_array_equal(T.export_status(), st[keep])
        T.refresh_status(now2)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(T.export_status(), st2)
        # and the sweep's incoming on the carried times
        got = T.sweep(incoming=True)
        assert got["totals"]["incoming"] == int((((st2 & 1) != 0) & (time_ns[keep] > reply_ns[keep])).sum())
        # patch_times still works on the new indices
        T.patch_times(np.array([0], np.uint32), np.array([now2], np.int64), np.array([now2], np.int64),
                      np.array([0], np.uint8))
        T.refresh_status(now2 + 1)
        torch.cuda.synchronize()
        assert T.export_status()[0] == 1
        # today's route drops the times
        ops = np.zeros((removed.shape[0], 3), np.uint32)
        ops[:, 0], ops[:, 1] = 1, removed
        twin.apply(ops)
        with pytest.raises(KadError) as e:
            twin.refresh_status(now2)
        assert "kad_table_set_times was not called" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("six", [False, True], ids=["v4", "v6"])
def test_wire_records_are_carried(gpu, six):
    t = TABLES["U10_10000"]
    n = t["status"].shape[0]
    rng = np.random.default_rng(0xADD5 + six)
    addrs = rng.integers(0, 256, size=(n, 18 if six else 6), dtype=np.uint8)
    keep = (t["status"] & 2) == 0
    w_ids, w_st, w_first, w_off, _, _ = R.expire_ref(t)
    with _open(t, gpu) as T:
        T.set_addrs(addrs)
        T.expire()
        targets = TB.adversarial_targets(dict(t, ids=w_ids, first=w_first), extra=512)
        tg = torch.from_numpy(targets).to(gpu)
        idx, cnt = T.rt_closest(tg, 14)
        out, m = T.buffer_nodes(tg, idx, cnt)
        torch.cuda.synchronize()
        want, wn = O.buffer_nodes(targets, w_ids, addrs[keep], idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy())
        np.testing.assert_array_equal(m.cpu().numpy(), wn)
        np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.gpu
def test_expire_needs_buckets(gpu):
    t = TABLES["empty"]
    with _open(t, gpu) as T:
        with pytest.raises(KadError) as e:
            T.expire()
        assert "INVALID" in str(e.value)
        assert T.sweep()["totals"]["expired"] == 0 and T.info()["n_nodes"] == 0
    t = TB.uniform_config(2000, 5, seed=0xE0)
    with DeviceTable(t["ids"], t["status"], None, None, device=gpu.index or 0, sorted=True) as T:
        with pytest.raises(KadError):
            T.expire()
        idx, cnt = T.nc_closest(torch.from_numpy(t["ids"][:64].copy()).to(gpu), 8)
        torch.cuda.synchronize()
        w_idx, w_cnt = O.flat_nc_closest(t["ids"], t["status"], t["ids"][:64], 8)
        np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint32), w_idx)
