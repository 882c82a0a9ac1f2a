"""opendht_amd.try_search_insert against Dht::trySearchInsert applied to the candidates one at a
time (searches_ref.py): the searches end in the same state, node for node and flag for flag. An adversarial input
(every state, candidates on and beside members and thresholds, expired candidates, old expired members that
removeExpiredNode drops) where almost every candidate falls back, and a steady input (every search live and holding
the 14 closest of a large population, candidates new random IDs) where at most 10 % may fall back. The CPU tests run
the host half of the scheme with the restatement's own verdicts; the GPU tests the whole, kernel and patch included."""
import functools

import numpy as np
import pytest

import searches_ref as R
from opendht_amd.searches import apply_search_verdicts

CAP = 32
NOW = 0.0


def adversarial():
    """(searches, candidate nodes): built anew on every call, equal every time."""
    rng = np.random.default_rng(21)
    searches = R.make_set(rng, 300, R.STATES, CAP, 4)
    known = {sn.node.id: sn.node for s in searches for sn in s.nodes}  # one Node per ID
    cands = []
    for x in R.make_cands(rng, searches, 3000):
        if x not in known:
            known[x] = R.Node(x, expired=bool(rng.random() < 0.3), time=NOW)
        cands.append(known[x])
    return searches, cands


def steady():
    """200 live searches, each holding the 14 closest of a population of 60 000 good nodes (300 per search); 5000 new
    random candidates."""
    rng = np.random.default_rng(22)
    pop = np.frombuffer(rng.bytes(20 * 60000), np.uint8).reshape(-1, 20)
    key = pop[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    sids = sorted(int.from_bytes(rng.bytes(20), "big") for _ in range(200))
    searches = []
    for sid in sids:
        near = np.argpartition(key ^ np.uint64(sid >> 96), 20)[:20]  # the top 64 bits order 60 000 random IDs
        ids = sorted((int.from_bytes(pop[i].tobytes(), "big") for i in near), key=lambda v: v ^ sid)[:R.SEARCH_NODES]
        searches.append(R.Search(sid, False, [R.SearchNode(R.Node(v, time=NOW)) for v in ids]))
    cands = [R.Node(int.from_bytes(rng.bytes(20), "big"), time=NOW) for _ in range(5000)]
    return searches, cands


def state_of(searches, cands):
    return ([(s.id, s.expired, [(sn.node.id, sn.is_bad(), sn.node.time) for sn in s.nodes]) for s in searches],
            [c.time for c in cands])


@functools.lru_cache(maxsize=None)
def sequential(make):
    """The state after trySearchInsert of every candidate in order."""
    searches, cands = make()
    sids = [s.id for s in searches]
    for c in cands:
        R.try_search_insert(searches, sids, c, NOW)
    return state_of(searches, cands)


def trims_of(searches):
    out = np.zeros(len(searches), bool)
    for i, s in enumerate(searches):
        fl, _, nfl = R.search_state(s)
        full, t = R.trim(list(nfl), fl)
        out[i] = full and t < len(nfl)
    return out


@pytest.mark.parametrize("make", [adversarial, steady])
def test_scheme_with_reference_verdicts(make):
    searches, cands = make()
    v = R.verdicts(searches, [c.id for c in cands], NOW)
    counts, dirty = apply_search_verdicts(R.HostSearches(searches, cands, NOW), len(searches), *v, trims_of(searches))
    assert state_of(searches, cands) == sequential(make)
    assert sum(counts[k] for k in ("skipped", "direct", "fallback")) == len(cands)
    if make is steady:
        assert counts["fallback"] <= len(cands) // 10, counts
        assert counts["skipped"] > len(cands) // 2 and counts["inserts"] > 0
    else:
        assert counts["fallback"] > counts["direct"] and counts["skipped"] > 0 and dirty.any(), counts


def test_refusal_that_trims_is_not_skipped():
    """A live search with 16 good entries refuses a far candidate and drops its last two entries while doing so
    (dht.cpp:1010-1011): the scheme must let the host see that candidate."""
    def one():
        return [R.Search(1 << 100, False, [R.SearchNode(R.Node((1 << 100) ^ (i + 1))) for i in range(16)])], \
               [R.Node(R.MAX_ID)]
    searches, cands = one()
    v = R.verdicts(searches, [c.id for c in cands], NOW)
    assert int(v[1][0]) == 0 and int(v[3][0]) == (R.END | R.FAR << 4)
    counts, dirty = apply_search_verdicts(R.HostSearches(searches, cands, NOW), 1, *v, trims_of(searches))
    ref, rc = one()
    R.try_search_insert(ref, [s.id for s in ref], rc[0], NOW)
    assert len(ref[0].nodes) == 14 and state_of(searches, cands) == state_of(ref, rc)
    assert counts["skipped"] == 0 and counts["fallback"] == 1 and dirty[0]


@pytest.mark.gpu
@pytest.mark.parametrize("make", [adversarial, steady])
def test_try_search_insert_equals_sequential(gpu, make):
    from opendht_amd import DeviceSearches, try_search_insert
    from test_searches import assert_export

    searches, cands = make()
    ids = R.id_bytes([c.id for c in cands])
    with DeviceSearches(*R.snapshot(searches), cap=CAP, device=0) as DS:
        counts = try_search_insert(DS, R.HostSearches(searches, cands, NOW), ids)
        assert state_of(searches, cands) == sequential(make)
        assert_export(DS, searches)  # the set was patched to the state the inserts left
        probe = ids[:500]
        got = DS.try_insert_host(probe)
    for g, w in zip(got, R.verdicts(searches, [c.id for c in cands[:500]], NOW)):
        assert np.array_equal(g, w)
    print(make.__name__, counts)
    assert sum(counts[k] for k in ("skipped", "direct", "fallback")) == len(cands)
    if make is steady:
        assert counts["fallback"] <= len(cands) // 10, counts
