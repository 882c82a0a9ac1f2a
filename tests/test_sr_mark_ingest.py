"""opendht_amd.mark_search_nodes over the steady input of test_search_ingest.py: 200 live searches of
14 good nodes each. 5 % of the member nodes expire (some of them long ago, so they are removable at once) and two
searches lose every node; one mark. Then half of the expired nodes reply and a few entries become candidates; a second
mark. After each, the device set equals the host's lists flag for flag, and the split of the changed searches (would
expire at its next step / short of good nodes / neither) equals Dht::searchStep's own tests on the host double. A
try_search_insert_device tick on the marked set then ends in the state of sequential trySearchInsert on the mutated host
double, with nothing uploaded in between. The CPU tests run over a device set made of the flag-level model, the GPU
tests over the device."""
import functools

import numpy as np
import pytest

import insert_ref as I
import mark_ref as M
import refill_ref as F
import searches_ref as R
import test_search_ingest as T
from opendht_amd.searches import mark_search_nodes, try_search_insert_device

CAP, NOW = T.CAP, T.NOW


def steady_shared():
    """test_search_ingest.steady with one Node object per ID."""
    searches, cands = T.steady()
    known = {}
    for s in searches:
        for sn in s.nodes:
            sn.node = known.setdefault(sn.node.id, sn.node)
    return searches, cands, list(known.values())


def first_changes(searches, members):
    """5 % of the member nodes expire, a third of them long ago; searches 3 and 100 lose every node."""
    rng = np.random.default_rng(51)
    nodes = [members[int(i)] for i in rng.choice(len(members), size=len(members) // 20, replace=False)]
    for k, n in enumerate(nodes):
        n.expired = True
        if k % 3 == 0:
            n.time = NOW - 2 * R.NODE_EXPIRE_TIME
    for s in (3, 100):
        for sn in searches[s].nodes:
            if not sn.node.expired:
                sn.node.expired = True
                nodes.append(sn.node)
    return nodes


def second_changes(searches, expired):
    """Half of the expired nodes reply; every 97th entry becomes a candidate."""
    nodes = expired[::2]
    for n in nodes:
        n.expired, n.time = False, NOW
    pairs, k = [], 0
    for i, s in enumerate(searches):
        for sn in s.nodes:
            k += 1
            if k % 97 == 0:
                sn.candidate = True
                pairs.append((i, sn.node))
    return nodes, pairs


@functools.lru_cache(maxsize=None)
def sequential():
    """The state after both changes and trySearchInsert of every candidate in order, on the host double alone."""
    searches, cands, members = steady_shared()
    second_changes(searches, first_changes(searches, members))
    sids = [s.id for s in searches]
    for c in cands:
        R.try_search_insert(searches, sids, c, NOW)
    return T.state_of(searches, cands)


def run(DS_of, check):
    searches, cands, members = steady_shared()
    DS = DS_of(searches)
    host = M.HostMark(searches)
    nodes = first_changes(searches, members)
    out = mark_search_nodes(DS, host, nodes, [], NOW)
    check(DS, searches)
    changed = sorted(out["expire"] + out["short"] + out["neither"])
    assert host.step_split(changed) == {k: out[k] for k in ("expire", "short", "neither")}
    assert out["expire"] == [3, 100] and len(out["short"]) > 50 and (out["hits"] >= 1).all()
    holders = set(i for i, s in enumerate(searches) for sn in s.nodes if sn.node.expired)
    assert set(changed) == holders
    nodes2, pairs = second_changes(searches, nodes)
    out2 = mark_search_nodes(DS, host, nodes2, pairs, NOW)
    check(DS, searches)
    changed2 = sorted(out2["expire"] + out2["short"] + out2["neither"])
    assert host.step_split(changed2) == {k: out2[k] for k in ("expire", "short", "neither")}
    assert len(out2["neither"]) > 10 and len(out2["short"]) > 10 and out2["pair_found"].all() and len(pairs) > 20
    assert 3 not in out2["expire"] and 100 not in out2["expire"]  # half of their nodes replied
    # the tick on the marked set: no list is uploaded before it
    counts = try_search_insert_device(DS, I.HostInsert(searches, cands, NOW), R.id_bytes([c.id for c in cands]), NOW, 8)
    assert T.state_of(searches, cands) == sequential()
    assert counts["skipped"] + counts["device"] + counts["host"] == len(cands) and counts["device"] > 100, counts
    check(DS, searches)
    return DS


def test_mark_then_tick_on_the_model():
    def check(DS, searches):
        assert [s.key() for s in DS.s] == [I.from_search(s, NOW).key() for s in searches]

    class Model(I.ModelSearches, M.ModelMark):
        def mark_nodes(self, *a, **kw):
            before = [s.key() for s in self.s]
            r = M.ModelMark.mark_nodes(self, *a, **kw)
            for i, s in enumerate(self.s):
                if s.key() != before[i]:
                    self._changed(i)
            return r

    run(lambda searches: Model(searches, CAP, NOW), check)


@pytest.mark.gpu
def test_mark_then_tick_on_the_device(gpu):
    from opendht_amd import DeviceSearches

    def check(DS, searches):
        got, want = DS.export(), F.expected_export(searches, DS.cap, NOW)
        for k in want:
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, (k, bad[:4])

    with run(lambda searches: DeviceSearches(*F.snapshot(searches, NOW), cap=CAP, device=0), check):
        pass
