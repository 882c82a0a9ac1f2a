"""Round-based ingest (opendht_amd.ingest): a candidate stream turned into kad_table_apply batches by
rounds of one triage launch each must leave the table that Dht::onNewNode(node, 0) leaves when it takes the same
candidates one at a time. The one-at-a-time side is restated here: the verdict of triage_ref.py for a single
candidate, its mirror op through oracle.FaithfulTable.apply, and after a split the same candidate again
(dht.cpp:925).

Three split-policy tables (50 and 257 nodes with mixed statuses, 257 all good), 520 candidates each: IDs already in
the table, new IDs with statuses drawn from good / dubious / expired, in-batch duplicates, and a fifth of them
sharing their first 3 bytes with self_id (they pile into self_id's bucket: MYBUCKET splits). Both values of
bootstrap. NONE cannot occur on a table with a bucket, so a table without one gets a case of its own."""
import functools

import numpy as np
import pytest
import torch

import oracle as O
import tables as TB
import triage_ref as R
from opendht_amd import DeviceTable, ingest

pytestmark = pytest.mark.gpu

SELF = np.random.default_rng(0x1E57).integers(0, 256, size=20, dtype=np.uint8)
CASES = [(name, boot) for name in ("S50", "S257", "S257good") for boot in (False, True)]
SEEN = {}  # per case: the per-kind counts ingest returned


@functools.lru_cache(maxsize=None)
def _table(name):
    if name == "S257good":
        t = TB.split_config(257, good=100, expired=0)
    else:
        n = int(name[1:])
        t = TB.split_config(n, seed=0x5EED + n)
    t["name"] = name
    return t


@functools.lru_cache(maxsize=None)
def _candidates(name):
    t = _table(name)
    rng = np.random.default_rng(0x1461 + t["ids"].shape[0])
    fresh = rng.integers(0, 256, size=(400, 20), dtype=np.uint8)
    fresh[::5, :3] = SELF[:3]  # a fifth near self_id
    known = t["ids"][rng.integers(0, t["ids"].shape[0], size=60)]
    dup = fresh[rng.integers(0, 400, size=60)]
    ids = np.concatenate([fresh, known, dup])
    ids = np.ascontiguousarray(ids[rng.permutation(ids.shape[0])])
    st = rng.choice(np.array([1, 1, 0, 2], np.uint8), size=ids.shape[0])
    assert 400 <= ids.shape[0] <= 600
    return ids, st


def one_at_a_time(t, ids, status, self_id, bootstrap):
    """Dht::onNewNode(node, 0) per candidate, in order, on host arrays; returns the final table and kind counts."""
    cur = dict(ids=t["ids"], status=t["status"], first=t["first"], off=t["off"])
    counts = {k: 0 for k in (R.NONE, R.KNOWN, R.REPLACE, R.INSERT, R.SPLIT, R.FULL)}
    for i in range(ids.shape[0]):
        for _ in range(200):  # splits of one candidate's bucket (bounded by the ID length)
            v, nd, bk = R.triage(cur, ids[i:i + 1], self_id, bootstrap)
            k = int(v[0]) & R.KIND_MASK
            counts[k] += 1
            if k == R.REPLACE:
                op = (2, int(nd[0]), 0)
            elif k == R.INSERT:
                op = (3, 0, 0)
            elif k == R.SPLIT:
                op = (4, int(bk[0]), 0)
            else:
                break
            ft = O.FaithfulTable(cur["ids"], cur["status"], cur["first"], cur["off"])
            new = k != R.SPLIT
            a, s, f, o, _, _ = ft.apply(np.array([op], np.uint32), ids[i:i + 1] if new else np.zeros((0, 20), np.uint8),
                                        status[i:i + 1] if new else np.zeros(0, np.uint8))
            ft.close()
            cur = dict(ids=a, status=s, first=f, off=o)
            if k != R.SPLIT:
                break
        else:
            raise AssertionError("a candidate split its bucket 200 times")
    return cur, counts


@functools.lru_cache(maxsize=None)
def _want(name, boot):
    ids, st = _candidates(name)
    return one_at_a_time(_table(name), ids, st, SELF, boot)


@pytest.mark.parametrize("name,boot", CASES)
def test_ingest_equals_one_at_a_time(gpu, name, boot):
    t = _table(name)
    ids, st = _candidates(name)
    want, wcounts = _want(name, boot)
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0) as T:
        got = ingest(T, ids, st, SELF, bootstrap=boot, max_rounds=200)
        e_ids, e_st, e_first, e_off = T.export()
        np.testing.assert_array_equal(e_off, want["off"])
        np.testing.assert_array_equal(e_first, want["first"])
        np.testing.assert_array_equal(e_ids, want["ids"])
        np.testing.assert_array_equal(e_st, want["status"])
        # the result answers queries as a table built from the exported arrays does
        targets = TB.adversarial_targets(dict(ids=e_ids, first=e_first), extra=1024)[:1024]
        assert targets.shape[0] == 1024
        idx, cnt = T.rt_closest(torch.from_numpy(targets).to(gpu), 8)
        torch.cuda.synchronize()
        widx, wcnt = O.flat_rt_closest(e_ids, e_st, e_first, e_off, targets, 8)
        np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint32), widx)
        np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt)
    assert got["rounds"] >= 2
    # acted-on verdicts change the table the same number of times either way
    for k, nm in ((R.REPLACE, "replace"), (R.INSERT, "insert"), (R.SPLIT, "split")):
        assert got[nm] == wcounts[k], (nm, got, wcounts)
    SEEN[(name, boot)] = got


def test_ingest_without_buckets(gpu):
    """A table without buckets: every candidate is NONE, one round, nothing applied."""
    ids, st = _candidates("S50")
    with DeviceTable(np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8), np.zeros((0, 20), np.uint8),
                     np.zeros(1, np.uint32), device=gpu.index or 0) as T:
        got = ingest(T, ids, st, SELF)
        assert T.info()["n_nodes"] == 0 and T.info()["n_buckets"] == 0
    assert got["none"] == ids.shape[0] and got["rounds"] == 1
    assert sum(got[k] for k in ("known", "replace", "insert", "split", "full")) == 0
    SEEN["empty"] = got


def test_max_rounds(gpu):
    t = _table("S257")
    ids, st = _candidates("S257")
    with DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0) as T:
        with pytest.raises(RuntimeError, match="pending"):
            ingest(T, ids, st, SELF, max_rounds=1)


def test_every_kind_counted():
    """Over the cases every kind was acted on at least once and at least one split happened. The expectation side
    is checked on its own, so this holds whichever order the tests ran in."""
    tot = {k: 0 for k in (R.KNOWN, R.REPLACE, R.INSERT, R.SPLIT, R.FULL)}
    for name, boot in CASES:
        _, c = _want(name, boot)
        for k in tot:
            tot[k] += c[k]
    assert min(tot.values()) >= 1 and tot[R.SPLIT] >= 1, tot
    if len(SEEN) == len(CASES) + 1:  # the whole module ran: the device side's own counts
        names = ("none", "known", "replace", "insert", "split", "full")
        dev = {nm: sum(c[nm] for c in SEEN.values()) for nm in names}
        assert min(dev.values()) >= 1, dev
