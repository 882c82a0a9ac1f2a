"""onNewNode triage verdicts (kad_rt_triage_batch) against the restatement of triage_ref.py.

Candidates per table: adversarial targets, up to 2048 sampled node IDs (KNOWN), the same with bytes 8..19 redrawn
(same 64-bit key, other tail: not KNOWN) and with the last bit flipped, and for each self_id 8 IDs sharing exactly
c leading bits with it for every c in 0..159 (they walk down into self_id's bucket: MYBUCKET).

Before anything is compared the expected bytes must show the kinds the table can produce (`_minimums`):
  * KNOWN at least min(n, 32) times: every sampled node ID is known.
  * REPLACE, INSERT, SPLIT, FULL at least 32 times wherever the buckets that give that kind to a new ID cover at
    least 1/8 of the ID space: of the 1024 random candidates about 128 land there (sd 11), the redrawn and flipped
    IDs only add to that. Below 1/8 nothing is required.
  * NONE everywhere on `empty`, and nowhere else.
Kinds that cannot occur: everything but NONE on `empty` (no bucket); everything but INSERT on `one_empty_bucket`;
KNOWN beyond a handful on S1 and S3 (1 and 3 nodes); REPLACE on the all-good tables S257good, S5000good and on
one12 (no expired node); INSERT on one12 (its only bucket is full) and on U4_2000 (every bucket holds > 100 nodes);
SPLIT and FULL on U4_2000 and all_bad (every bucket holds an expired node); SPLIT without bootstrap wherever
self_id's bucket is dubious or has an expired node; FULL on one12 with a self_id (a single bucket that is mine always
splits). U4_2000good (beyond the issue's list: U4_2000 with every node good) puts SPLIT and FULL without a ping node
on the WIDE path; ties48 / dups48 give it FULL with one. test_coverage holds the whole set to: every kind,
MYBUCKET, SPLIT with MYBUCKET, FULL with and without a ping node.
"""
import functools

import numpy as np
import pytest
import torch

import tables as TB
import triage_ref as R
from opendht_amd import DeviceTable

pytestmark = pytest.mark.gpu

SELF = np.random.default_rng(0x7214).integers(0, 256, size=20, dtype=np.uint8)  # drawn once
BASE = 0x7FFF0000


def _one12():
    """One bucket, 12 nodes, some not good, none expired: the n_buckets == 1 clause (a split despite dubious nodes)."""
    rng = np.random.default_rng(0x12)
    ids = rng.integers(0, 256, size=(12, 20), dtype=np.uint8)
    st = np.array([1, 1, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1], np.uint8)
    return TB.table(ids, st, np.zeros((1, 20), np.uint8), np.array([0, 12], np.uint32), name="one12")


@functools.lru_cache(maxsize=None)
def _tables():
    ts = {t["name"]: t for t in TB.all_small_tables()}
    extra = [TB.uniform_config(2000, 4), TB.split_config(257, good=100, expired=0),
             TB.split_config(5000, good=100, expired=0), _one12(), TB.uniform_config(2000, 4, good=100, expired=0)]
    for t, name in zip(extra, ("U4_2000", "S257good", "S5000good", "one12", "U4_2000good")):
        t["name"] = name
        ts[name] = t
    return ts


NAMES = ("empty", "one_empty_bucket", "S1", "S3", "S50", "S257", "S10000", "U10_10000", "all_bad", "sparse_good",
         "ties", "dups", "ties48", "dups48", "offset_first", "U4_2000", "S257good", "S5000good", "one12", "U4_2000good")


def self_ids(t):
    """A fixed random ID, a node of the table, and None (no bucket is mine). The node is the middle one, or where
    the table has full buckets (>= 8 nodes) the first node of the first full bucket at or after the middle one's
    (else before it), so that "my" bucket can be full."""
    out = [SELF]
    n = t["ids"].shape[0]
    if n:
        off = t["off"].astype(np.int64)
        mid = int(np.searchsorted(off, n // 2, side="right")) - 1
        full = np.flatnonzero(np.diff(off) >= 8)
        j = n // 2
        if full.size:
            after = full[full >= mid]
            j = int(off[after[0] if after.size else full[-1]])
        out.append(t["ids"][j].copy())
    out.append(None)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """(candidates, facts, bucket, base kind, base node) of a table, computed once and left unchanged."""
    t = _tables()[name]
    rng = np.random.default_rng(0x7A1A)
    parts = [TB.adversarial_targets(t, extra=1024)]
    n = t["ids"].shape[0]
    if n:
        pick = t["ids"][rng.choice(n, size=min(n, 2048), replace=False)]
        other_tail = pick.copy()
        other_tail[:, 8:] = rng.integers(0, 256, size=(pick.shape[0], 12), dtype=np.uint8)
        flipped = pick.copy()
        flipped[:, 19] ^= 1
        parts += [pick, other_tail, flipped]
    parts += [R.near_targets(s, rng) for s in self_ids(t) if s is not None]
    cand = np.ascontiguousarray(np.concatenate(parts), np.uint8)
    cand.setflags(write=False)
    facts = R.BucketFacts(t)
    bucket = R.find_bucket(t, cand)
    kind, node = R.base_verdicts(t, facts, cand, bucket)
    return cand, facts, bucket, kind, node


def _minimums(name, facts, self_id, bootstrap):
    """The least count of each kind the expected bytes must show (module docstring)."""
    t = _tables()[name]
    if facts.B == 0:
        return {R.NONE: _case(name)[0].shape[0]}
    need = {R.KNOWN: min(t["ids"].shape[0], 32)}
    cls = facts.bucket_class()
    sb = None if self_id is None else int(R.find_bucket(t, self_id)[0])
    ok = facts.split_ok(sb, bootstrap)
    final = np.where(cls == R._FULLISH, np.where(ok, R.SPLIT, R.FULL), cls)
    for k in (R.REPLACE, R.INSERT, R.SPLIT, R.FULL):
        if facts.share[final == k].sum() >= 0.125:
            need[k] = 32
    return need


def want_of(name, self_id, bootstrap, index_base=0, check=True):
    cand, facts, bucket, kind, node = _case(name)
    v, nd, bk = R.finish(_tables()[name], facts, kind, node, bucket, self_id, bootstrap, index_base)
    if check:
        kinds = v & R.KIND_MASK
        for k, least in _minimums(name, facts, self_id, bootstrap).items():
            got = int((kinds == k).sum())
            assert got >= least, f"{name} self={None if self_id is None else 'id'} boot={bootstrap}: kind {k} {got} < {least}"
        if name != "empty":
            assert not (kinds == R.NONE).any()
    return v, nd, bk


def _make(t, gpu, **kw):
    return DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, sorted=t["sorted"], **kw)


def _got(res):
    v, nd, bk = res
    f = lambda a: None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else a)  # noqa: E731
    v, nd, bk = f(v), f(nd), f(bk)
    return v, nd.view(np.uint32), None if bk is None else bk.view(np.uint32)


@pytest.mark.parametrize("name", NAMES)
def test_verdicts(gpu, name):
    """verdict, node and bucket equal the restatement for every self_id and both values of bootstrap; bucket equals
    find_bucket; without want_bucket the other two are the same; the host-pointer call gives the same."""
    t = _tables()[name]
    cand = _case(name)[0]
    tg = torch.from_numpy(cand.copy()).to(gpu)
    with _make(t, gpu) as T:
        fb = T.find_bucket(tg).cpu().numpy().view(np.uint32)
        for sid in self_ids(t):
            for boot in (False, True):
                wv, wn, wb = want_of(name, sid, boot)
                msg = f"{name} self={'none' if sid is None else sid[:4].tobytes().hex()} boot={boot}"
                v, nd, bk = _got(T.rt_triage(tg, sid, boot, want_bucket=True))
                np.testing.assert_array_equal(v, wv, err_msg=msg)
                np.testing.assert_array_equal(nd, wn, err_msg=msg)
                np.testing.assert_array_equal(bk, wb, err_msg=msg)
                np.testing.assert_array_equal(bk, fb, err_msg=msg)
                v2, nd2, bk2 = _got(T.rt_triage(tg, sid, boot))
                assert bk2 is None
                np.testing.assert_array_equal(v2, wv, err_msg=msg)
                np.testing.assert_array_equal(nd2, wn, err_msg=msg)
                hv, hn, hb = _got(T.rt_triage_host(cand, sid, boot, want_bucket=True))
                np.testing.assert_array_equal(hv, wv, err_msg=msg + " host")
                np.testing.assert_array_equal(hn, wn, err_msg=msg + " host")
                np.testing.assert_array_equal(hb, wb, err_msg=msg + " host")


def test_coverage():
    """The expected bytes over all tables hold every kind, the MYBUCKET bit, SPLIT with MYBUCKET, and FULL both with
    and without a ping node, each at least 32 times: no comparison above passes on empty ground."""
    tot = {k: 0 for k in (R.NONE, R.KNOWN, R.REPLACE, R.INSERT, R.SPLIT, R.FULL)}
    mine = split_mine = full_ping = full_noping = 0
    for name in NAMES:
        for sid in self_ids(_tables()[name]):
            for boot in (False, True):
                v, nd, _ = want_of(name, sid, boot, check=False)
                k = v & R.KIND_MASK
                for kk in tot:
                    tot[kk] += int((k == kk).sum())
                mine += int(((v & R.MYBUCKET) != 0).sum())
                split_mine += int(((k == R.SPLIT) & ((v & R.MYBUCKET) != 0)).sum())
                full_ping += int(((k == R.FULL) & (nd != R.NO_NODE)).sum())
                full_noping += int(((k == R.FULL) & (nd == R.NO_NODE)).sum())
    assert min(tot.values()) >= 32, tot
    assert min(mine, split_mine, full_ping, full_noping) >= 32, (mine, split_mine, full_ping, full_noping)
    # the cases the issue names: SPLIT on the 257-node all-good table under bootstrap, SPLIT with MYBUCKET on the
    # all-good 5000-node table when self_id is one of its nodes
    v, _, _ = want_of("S257good", SELF, True)
    assert int(((v & R.KIND_MASK) == R.SPLIT).sum()) >= 32
    t = _tables()["S5000good"]
    v, _, _ = want_of("S5000good", self_ids(t)[1], False)
    assert int((v == (R.SPLIT | R.MYBUCKET)).sum()) >= 32
    v, _, _ = want_of("one12", SELF, False)
    assert int(((v & R.KIND_MASK) == R.SPLIT).sum()) >= 32 and not ((v & R.KIND_MASK) == R.FULL).any()


@pytest.mark.parametrize("name", ["S10000", "U4_2000"])
def test_index_base(gpu, name):
    """index_base shifts node and nothing else (lane path and WIDE path)."""
    t = _tables()[name]
    cand = _case(name)[0]
    tg = torch.from_numpy(cand.copy()).to(gpu)
    wv, wn, wb = want_of(name, SELF, True, index_base=BASE)
    w0 = want_of(name, SELF, True)
    assert np.array_equal(wv, w0[0]) and np.array_equal(wb, w0[2]) and (wn != w0[1]).sum() >= 32
    with _make(t, gpu, index_base=BASE) as T:
        v, nd, bk = _got(T.rt_triage(tg, SELF, True, want_bucket=True))
    np.testing.assert_array_equal(v, wv)
    np.testing.assert_array_equal(nd, wn)
    np.testing.assert_array_equal(bk, wb)


@pytest.mark.parametrize("name", ["U10_10000", "S10000", "U4_2000"])
def test_after_status_patch(gpu, name):
    """After patch_status on half the nodes the verdicts follow the new snapshot (status bytes and the directory's
    good mask alike), and at least 32 of them changed."""
    t = _tables()[name]
    cand = _case(name)[0]
    tg = torch.from_numpy(cand.copy()).to(gpu)
    rng = np.random.default_rng(5)
    st = t["status"].copy()
    with _make(t, gpu) as T:
        before = _got(T.rt_triage(tg, SELF, True, want_bucket=True))
        nodes = rng.choice(st.shape[0], size=st.shape[0] // 2, replace=False).astype(np.uint32)
        st[nodes] = rng.choice(np.array([0, 1, 1, 2], np.uint8), size=nodes.shape[0])
        T.patch_status(nodes, st[nodes])
        t2 = dict(t, status=st)
        wv, wn, wb = R.triage(t2, cand, SELF, True)
        v, nd, bk = _got(T.rt_triage(tg, SELF, True, want_bucket=True))
        np.testing.assert_array_equal(v, wv)
        np.testing.assert_array_equal(nd, wn)
        np.testing.assert_array_equal(bk, wb)
        assert ((wv != before[0]) | (wn != before[1])).sum() >= 32, "the patch changed too few verdicts"


def test_two_streams(gpu):
    """A const query without table-held scratch: two calls in flight on two streams give the same bytes."""
    name = "S10000"
    t = _tables()[name]
    tg = torch.from_numpy(_case(name)[0].copy()).to(gpu)
    wv, wn, wb = want_of(name, SELF, True)
    with _make(t, gpu) as T:
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        q = tg.shape[0]
        outs = [(torch.empty(q, dtype=torch.uint8, device=gpu), torch.empty(q, dtype=torch.int32, device=gpu),
                 torch.empty(q, dtype=torch.int32, device=gpu)) for _ in range(2)]
        for _ in range(4):
            T.rt_triage(tg, SELF, True, out=outs[0], stream=s1)
            T.rt_triage(tg, SELF, True, out=outs[1], stream=s2)
        torch.cuda.synchronize()
        for o in outs:
            v, nd, bk = _got(o)
            np.testing.assert_array_equal(v, wv)
            np.testing.assert_array_equal(nd, wn)
            np.testing.assert_array_equal(bk, wb)
