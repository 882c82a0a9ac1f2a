"""The flag-level model of kad_sr_mark_nodes (mark_ref.py) against the reference's own way of keeping
node status: searches_ref searches that share Node objects, whose expired, time and candidate fields are flipped in
place. What SearchNode::isBad() and removeExpiredNode's test then read is what the model's bytes must say, with the ops
derived as opendht_amd.mark_search_nodes derives them; the counts equal dht.cpp:583-597 transcribed. Also a check that
the cases of test_sr_mark.py contain every mechanism. CPU only."""
import numpy as np
import pytest

import insert_ref as I
import mark_ref as M
import refill_ref as F
import searches_ref as R
from opendht_amd.searches import mark_search_nodes

T0 = 0.0  # searches_ref.make_search stamps its nodes relative to 0


def shared_set(rng, S, cap):
    """searches_ref.make_set with Node objects shared between searches: one member's Node takes the place of an entry's
    node in up to three other searches."""
    searches = R.make_set(rng, S, tuple(st for st in R.STATES if st != "trim" or cap >= 16), cap)
    holders = [s for s in searches if s.nodes]
    for _ in range(S // 4):
        node = holders[int(rng.integers(0, len(holders)))].nodes[0].node
        for i in rng.permutation(len(holders))[:3]:
            s = holders[int(i)]
            if any(sn.node.id == node.id for sn in s.nodes):
                continue
            s.nodes[int(rng.integers(0, len(s.nodes)))].node = node
            s.nodes.sort(key=lambda sn: sn.node.id ^ s.id)
    return searches


def mutate(rng, searches, now0, now1):
    """Timeouts, replies, old expiries and candidate flips on the shared objects. Returns the changed nodes and the
    pairs a host would report: every node whose expired or time moved, or whose removability differs between now0 and
    now1; every entry whose candidate flipped, or that is a candidate and whose node is among the changed."""
    nodes = {}
    for s in searches:
        for sn in s.nodes:
            nodes[id(sn.node)] = sn.node
    was = {k: F.removable(n, now0) for k, n in nodes.items()}
    changed = {}
    for k, n in nodes.items():
        r = rng.random()
        if r < 0.10:  # a request timed out
            n.expired = True
        elif r < 0.20:  # a reply
            n.expired, n.time = False, now1
        elif r < 0.25:  # expired long ago
            n.expired, n.time = True, now1 - 2 * R.NODE_EXPIRE_TIME
        elif r < 0.30:  # reported although nothing moved
            pass
        else:
            if F.removable(n, now1) != was[k]:
                changed[k] = n
            continue
        changed[k] = n
    pairs = []
    for i, s in enumerate(searches):
        for sn in s.nodes:
            flipped = rng.random() < 0.08
            if flipped:
                sn.candidate = not sn.candidate
            if flipped or (sn.candidate and id(sn.node) in changed):
                pairs.append((i, sn.node))
    return list(changed.values()), pairs


@pytest.mark.parametrize("cap,later", [(14, 0.0), (32, 0.0), (32, 660.0), (64, 1300.0)])
def test_model_follows_the_shared_nodes(cap, later):
    rng = np.random.default_rng(300 + cap + int(later))
    for rep in range(6):
        searches = shared_set(rng, 40, cap)
        DS = M.ModelMark(searches, cap, T0)
        assert [s.key() for s in DS.s] == [I.from_search(s, T0).key() for s in searches]
        host = M.HostMark(searches)
        nodes, pairs = mutate(rng, searches, T0, T0 + later)
        now = T0 + later
        out = mark_search_nodes(DS, host, nodes, pairs, now)
        # the model's lists and records are the mutated searches' snapshot
        assert [s.key() for s in DS.s] == [I.from_search(s, now).key() for s in searches]
        got, want = I.expected_export(DS.s, cap), F.expected_export(searches, cap, now)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        for m, s in zip(DS.s, searches):  # searches_ref.snapshot knows KAD_SN_BAD alone
            fl, ids, nfl = R.search_state(s)
            assert [e[1] & M.SN_BAD for e in m.ents] == list(nfl) and [e[0] for e in m.ents] == [sn.node.id for sn in s.nodes]
        assert out["pair_found"].all() and (out["hits"] >= 1).all()
        changed = sorted(out["expire"] + out["short"] + out["neither"])
        assert host.step_split(changed) == {k: out[k] for k in ("expire", "short", "neither")}
        assert len(changed) >= 5


def test_counts_equal_the_reference_loops():
    rng = np.random.default_rng(77)
    for s in shared_set(rng, 60, 32):
        bad = sum(1 for sn in s.nodes if sn.is_bad())
        lead = 0
        for sn in s.nodes:
            if not sn.is_bad():
                break
            lead += 1
        full, _ = R.trim([F.node_flag(sn, T0) for sn in s.nodes], R.SR_EXPIRED if s.expired else 0)
        assert M.counts_of(I.from_search(s, T0)) == (len(s.nodes), bad, lead, (1 if full else 0) | (2 if s.expired else 0))


def test_model_by_hand():
    """Node ops first, pairs after them; a search is changed only if a byte differs from before."""
    sid = 1 << 100
    a = I.FlagSearch(sid, False, [(sid ^ (i + 1), 0) for i in range(16)])
    b = I.FlagSearch(sid + 1, True, [(sid ^ 1, M.SN_BAD), (sid ^ 99, M.BOTH)])
    c = I.FlagSearch(sid + 2, False, [(sid ^ 1, M.SN_BAD)])
    x, y = sid ^ 1, sid ^ 99
    after, hits, found, changed, counts = M.mark([a, b, c], [x, y, 5], [0, M.SN_REMOVABLE, 3], [M.SN_BAD, 0, 0],
                                                 [(0, x, 0), (1, sid ^ 7, 1), (2, x, M.BOTH)])
    assert list(hits) == [3, 1, 0] and list(found) == [1, 0, 1]
    assert after[0] is a  # the op set BAD, the pair put the byte back: not changed
    assert list(changed) == [1, 2] and after[1].ents == [(x, M.SN_BAD), (y, M.SN_BAD)] and after[2].ents == [(x, M.BOTH)]
    assert [tuple(r) for r in counts] == [(2, 2, 2, 2), (1, 1, 1, 0)]
    # 16 good entries: t = 14; two bad ones among the first 14 move it up to 16
    after, _, _, changed, counts = M.mark([a], [sid ^ 3, sid ^ 4], [0, 0], [1, 1], [])
    assert list(changed) == [0] and tuple(counts[0]) == (16, 2, 0, 1)
    assert R.trim([e[1] for e in after[0].ents], 0) == (True, 16)


def test_cases_cover_the_mechanisms():
    """Passes on the model alone: every mechanism of the call occurs in the GPU cases."""
    tot = M.new_stats()
    for name in M.CASES:
        c = M.case(name)
        for k, v in c["stats"].items():
            tot[k] += v
        assert len(set(c["nodes"])) == len(c["nodes"]) == M.CASES[name][2]
        assert len(c["pairs"]) == M.CASES[name][3]
        # the call that undoes it restores every search and reports the same searches
        assert [s.key() for s in c["undone"][0]] == [s.key() for s in c["searches"]]
        assert np.array_equal(c["undone"][3], c["changed"])
    for k, v in tot.items():
        assert v >= 2, (k, tot)
    assert {M.CASES[n][0] for n in M.CASES} >= {0, 1, 3, 65, 300}
    assert {M.CASES[n][1] for n in M.CASES} == {14, 32, 64}
    assert {M.CASES[n][2] for n in M.CASES} >= {0, 1, 63, 64, 65, M.LDS_KEYS, M.LDS_KEYS + 1}
    assert {M.CASES[n][3] for n in M.CASES} >= {0, 1, 70}
    for name in M.CASES:  # every state of the cap in every set of 65 or 300 searches, and changed there by the call
        S, cap = M.CASES[name][:2]
        c = M.case(name)
        assert len(c["states"]) == S
        if S >= 65:
            assert set(c["states"]) == set(I.states_for(cap)), (name, set(I.states_for(cap)) - set(c["states"]))
    for cap in (14, 32, 64):
        hit = set()
        for name in M.CASES:
            if M.CASES[name][1] == cap:
                hit |= set(M.case(name)["states"][int(s)] for s in M.case(name)["changed"])
        assert hit >= set(I.states_for(cap)) - {"empty"}, (cap, hit)
    # the set a case is made of is the one insert_ref.make_set draws from the same seed
    rng_a, rng_b = np.random.default_rng(9), np.random.default_rng(9)
    assert [s.key() for s in M.make_set(rng_a, 65, 32)[0]] == [s.key() for s in I.make_set(rng_b, 65, 32)]
    # the large batches are mostly IDs that nobody holds
    for name in M.CASES:
        c = M.case(name)
        if len(c["nodes"]) >= M.LDS_KEYS:
            assert (c["hits"] == 0).sum() > len(c["nodes"]) // 2
