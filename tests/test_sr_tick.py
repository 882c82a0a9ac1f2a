"""kad_sr_try_insert_tick and opendht_amd.try_search_insert_tick on the GPU. The seven cases of
test_sr_insert_ingest.py: the host's searches end as after the sequential reference, the device set equals the host's
lists, its verdicts afterwards are the reference's, and the counts are those of try_search_insert_device on a twin set.
The raw call's first round against kad_sr_try_insert_batch_host and kad_searches_export on a twin. Edges: a set of 5000
searches (the prefix-directory form of the verdict kernel), a 64-entry list at cap 64, a refusal that trims, an old
member elsewhere, a slab overflow in the middle of a tick, no candidates, no searches, slabs above 64 entries."""
import numpy as np
import pytest

import insert_ref as I
import refill_ref as F
import searches_ref as R
import test_search_ingest as T
import test_sr_insert_ingest as G
import tick_ref as K
from test_sr_tick_model import run_both

pytestmark = pytest.mark.gpu
CAP, NOW = G.CAP, G.NOW


def device_set(searches, cap=CAP):
    from opendht_amd import DeviceSearches

    return DeviceSearches(*F.snapshot(searches, NOW), cap=cap, device=0)


def assert_verdicts_equal_reference(DS, searches, ids):
    for g, w in zip(DS.try_insert_host(R.id_bytes(ids)), R.verdicts(searches, ids, NOW)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("name,max_rounds", G.CASES)
def test_tick_equals_sequential_and_the_round_driver(gpu, name, max_rounds):
    DS, searches, twin = run_both(name, max_rounds, device_set)
    with DS, twin:
        G.assert_device_equals_host(DS, searches)
        assert_verdicts_equal_reference(DS, searches, [c.id for c in G.INPUTS[name]()[1][:300]])


def test_first_round_equals_the_existing_calls(gpu):
    """max_rounds = 1 on the adversarial input: what the call reports for the candidates it decided is what
    try_insert_host and export(nodes=False) give on a twin set that nothing was applied to."""
    searches, cands = T.adversarial()
    ids = R.id_bytes([c.id for c in cands])
    flags = np.array([I.SN_BAD if c.expired else 0 for c in cands], np.uint8)
    with device_set(searches) as DS, device_set(searches) as twin:
        r = DS.try_insert_tick(ids, flags, max_rounds=1)
        lb, fwd, back, stop = twin.try_insert_host(ids)
        trim = K.trim_bits(lb, fwd, back, stop, K.trims_of_export(twin.export(nodes=False)))
    done = r["kind"] != K.LEFT
    st = r["stats"]
    assert st["rounds"] == 1 and st["skipped"] + st["applied"] + st["left"] == len(cands)
    assert st["overflowed"] == len(r["overflow"]) and list(r["overflow"]) == sorted(set(r["overflow"]))  # `cap` searches
    assert st["skipped"] == (r["kind"] == K.TICK_SKIPPED).sum() and st["applied"] == (r["kind"] == K.APPLIED).sum()
    assert st["skipped"] and st["applied"] and st["left"] and trim[done].any()
    for got, want in ((r["lb"], lb), (r["fwd"], fwd), (r["back"], back), (r["stop"], stop), (r["trim"], trim)):
        assert np.array_equal(got[done], want[done])
    assert (r["round"][done] == 1).all()
    kind, pw, _, _ = K.plan_round(len(searches), lb, fwd, back, stop, trim)
    assert np.array_equal(r["kind"] == K.LEFT, kind == K.DEFERRED) and st["pairs"] == len(pw)
    assert st["verdict_ms"] > 0 and st["insert_ms"] > 0


def tick_against_sequential(make, cap=CAP, max_rounds=8):
    from opendht_amd import try_search_insert_tick

    searches, cands = make()
    ref, rc = make()
    sids = [s.id for s in ref]
    for n in rc:
        R.try_search_insert(ref, sids, n, NOW)
    DS = device_set(searches, cap)
    counts = try_search_insert_tick(DS, I.HostInsert(searches, cands, NOW), R.id_bytes([c.id for c in cands]), NOW,
                                    max_rounds)
    assert T.state_of(searches, cands) == T.state_of(ref, rc)
    G.assert_device_equals_host(DS, searches)
    return DS, searches, cands, counts


def five_thousand():
    """5000 searches, most of them full with their 14 closest nodes, every 40th one short (0 to 3 nodes, so it accepts);
    600 candidates: strangers, members, nodes next to the short searches, repeats."""
    rng = np.random.default_rng(77)
    ids = R.make_ids(rng, 5000)
    searches = []
    for i, sid in enumerate(ids):
        n = int(rng.integers(0, 4)) if i % 40 == 7 else R.SEARCH_NODES
        searches.append(R.Search(sid, False, [R.SearchNode(R.Node(v, time=NOW)) for v in R.make_list(rng, sid, n)]))
    known = {sn.node.id: sn.node for s in searches for sn in s.nodes}
    cands = []
    for k in range(600):
        kind = k % 4
        if kind == 0:
            x = int.from_bytes(rng.bytes(20), "big")
        elif kind == 1:
            x = ids[40 * int(rng.integers(0, 125)) + 7] ^ int(rng.integers(1, 1 << 30))
        elif kind == 2:
            s = searches[int(rng.integers(0, 5000))]
            x = s.nodes[int(rng.integers(0, len(s.nodes)))].node.id if s.nodes else s.id ^ 5
        else:
            x = cands[int(rng.integers(0, len(cands)))].id
        if x not in known:
            known[x] = R.Node(x, expired=bool(rng.random() < 0.2), time=NOW)
        cands.append(known[x])
    return searches, cands


def test_five_thousand_searches_take_the_prefix_directory(gpu):
    DS, searches, cands, counts = tick_against_sequential(five_thousand, max_rounds=None)
    with DS:
        assert DS.S == 5000 and counts["host"] == 0 and counts["device"] >= 100 and counts["skipped"] >= 100, counts
        assert_verdicts_equal_reference(DS, searches, [c.id for c in cands[:300]])


def sixty_four():
    """cap 64, one live search of 64 entries: 14 good (the most distant entry among them), 50 bad. A good candidate
    closer than all of them makes a 65th entry; the pops cut the list back to 64."""
    sid = 1 << 140
    bad = set(range(13, 63))
    nodes = [R.SearchNode(R.Node(sid ^ (2 * (i + 1)), expired=i in bad, time=NOW)) for i in range(64)]
    return [R.Search(sid, False, nodes)], [R.Node(sid ^ 3, time=NOW)]


def test_a_full_slab_of_sixty_four_takes_one_insert(gpu):
    DS, searches, _, counts = tick_against_sequential(sixty_four, cap=64)
    with DS:
        assert DS.cap == 64 and len(searches[0].nodes) == 64 and searches[0].nodes[1].node.id == (1 << 140) ^ 3
        assert counts == {"skipped": 0, "device": 1, "host": 0, "rounds": 1, "pairs": 1, "overflowed": 0}


def test_trimming_refusal_and_old_member_elsewhere(gpu):
    DS, searches, _, counts = tick_against_sequential(G.trimming_refusal)
    with DS:
        assert len(searches[0].nodes) == 14
        assert counts["host"] == 0 and counts["device"] == 1 and counts["pairs"] == 1 and counts["skipped"] == 0
    DS, searches, _, counts = tick_against_sequential(G.old_member_elsewhere)
    with DS:
        assert counts["host"] == 1 and counts["device"] == 1
        assert any(sn.node.id == (1 << 150) - 7 for sn in searches[2].nodes) and len(searches[2].nodes) == 5


def walls_and(good, bad):
    """Six searches at cap 16: walls (full, 14 close good nodes) W0 < O < W1 < W2 < A < W3. O is live with `good` good and
    `bad` bad entries, A holds 3 nodes. Candidates: x, good and closer to O than all its entries; y, which A takes; y
    again; z, which A takes as well. In the first round x and y are ready, the second y and z meet y's searches."""
    def wall(sid):
        return R.Search(sid, False, [R.SearchNode(R.Node(sid ^ (i + 1), time=NOW)) for i in range(14)])
    o, a = 2 << 150, 5 << 150
    O = R.Search(o, False, [R.SearchNode(R.Node(o ^ (2 * (i + 1)), expired=i >= good, time=NOW)) for i in range(good + bad)])
    A = R.Search(a, False, [R.SearchNode(R.Node(a ^ (i + 1), time=NOW)) for i in range(3)])
    y = R.Node(a ^ 100, time=NOW)
    return ([wall(1 << 150), O, wall(3 << 150), wall(4 << 150), A, wall(6 << 150)],
            [R.Node(o ^ 1, time=NOW), y, y, R.Node(a ^ 101, time=NOW)])


def test_overflow_stops_the_call_and_the_driver_finishes(gpu):
    """13 good and 3 bad entries fill a slab of 16 without making the search full: the closer good candidate is a 17th
    entry and nothing is popped. The device leaves the search as it was and lists it; the call ends with that round."""
    searches, cands = walls_and(13, 3)
    ids = R.id_bytes([c.id for c in cands])
    with device_set(searches, 16) as DS:
        before = DS.export()
        r = DS.try_insert_tick(ids, None, 0)
        after = DS.export()
    assert list(r["overflow"]) == [1] and list(r["kind"]) == [K.APPLIED, K.APPLIED, K.LEFT, K.LEFT]
    assert (r["lb"][0], r["fwd"][0], r["back"][0], r["stop"][0]) == (2, 0, 1, R.FAR | R.FAR << 4)
    st = r["stats"]
    assert (st["rounds"], st["applied"], st["left"], st["overflowed"], st["pairs"]) == (1, 2, 2, 1, 2)
    for k in before:
        assert np.array_equal(before[k][1], after[k][1]), k  # byte for byte as it was
    assert after["n"][4] == 4 and before["n"][4] == 3  # the other pair of the round was applied
    # the driver replays, patches and grows, then asks again for what was left
    DS, searches, _, counts = tick_against_sequential(lambda: walls_and(13, 3), cap=16)
    with DS:
        assert DS.cap == 32 and len(searches[1].nodes) == 17 and len(searches[4].nodes) == 5
        assert counts == {"skipped": 0, "device": 4, "host": 0, "rounds": 3, "pairs": 3, "overflowed": 1}  # the second y is known


def test_fourteen_good_and_two_bad_do_not_overflow(gpu):
    """14 good and 2 bad entries at cap 16: the search is full, so the closer good candidate is a 15th good entry and the
    pops take the most distant good one (and what follows it) in the same insertNode: the list never outgrows its slab."""
    DS, searches, _, counts = tick_against_sequential(lambda: walls_and(14, 2), cap=16)
    with DS:
        assert DS.cap == 16 and len(searches[1].nodes) == 14 and counts["overflowed"] == 0 and counts["host"] == 0


def test_no_candidates_no_searches_and_large_slabs(gpu):
    from opendht_amd import DeviceSearches, KadError, _lib

    searches, cands = walls_and(13, 3)
    ids = R.id_bytes([c.id for c in cands])
    with device_set(searches, 16) as DS:
        before = DS.export()
        r = DS.try_insert_tick(np.zeros((0, 20), np.uint8))
        assert len(r["kind"]) == 0 and len(r["overflow"]) == 0 and not any(r["stats"].values())
        assert all(np.array_equal(before[k], v) for k, v in DS.export().items())
    with DeviceSearches(np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint32),
                        np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8), cap=16, device=0) as DS:
        r = DS.try_insert_tick(ids)
        assert (r["kind"] == K.TICK_SKIPPED).all() and r["stats"]["skipped"] == 4 and r["stats"]["rounds"] == 0
        assert not any(r[k].any() for k in ("round", "lb", "fwd", "back", "stop", "trim"))
    with device_set(searches, 65) as DS:
        before = DS.export()
        with pytest.raises(KadError) as e:
            DS.try_insert_tick(ids)
        assert e.value.code == _lib.KAD_ERR_UNSUPPORTED
        with pytest.raises(KadError) as e:  # the flags are checked first
            DS.try_insert_tick(ids, np.array([0, 2, 0, 0], np.uint8))
        assert e.value.code == _lib.KAD_ERR_INVALID
        assert len(DS.try_insert_tick(np.zeros((0, 20), np.uint8))["kind"]) == 0
        assert all(np.array_equal(before[k], v) for k, v in DS.export().items())
