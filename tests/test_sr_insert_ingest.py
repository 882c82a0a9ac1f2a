"""plan_insert_round and opendht_amd.try_search_insert_device against Dht::trySearchInsert applied to
the candidates one at a time (searches_ref.py): the searches end in the same state, node for node and flag for flag,
node times included, and the device set equals the host's lists with KAD_SN_REMOVABLE at `now`. Inputs: the adversarial
and the steady one of test_search_ingest.py, and inputs of 120 searches and 1400 candidates where half of the expired
candidates are old (barriers) and 200 candidates repeat. The CPU tests run the tick over a device set made of the
flag-level model with the restatement's verdicts (insert_ref.ModelSearches); the GPU tests run the whole."""
import functools

import numpy as np
import pytest

import insert_ref as I
import refill_ref as F
import searches_ref as R
import test_search_ingest as T
from opendht_amd.searches import plan_insert_round, try_search_insert_device

CAP, NOW = T.CAP, T.NOW
OLD = NOW - 2 * R.NODE_EXPIRE_TIME - 100.0


def with_old(seed):
    """(searches, candidate nodes): 120 searches in every state, 1200 candidates on and beside members and thresholds,
    30 % of the strangers expired and half of those old, then 200 repeats of earlier candidates mixed in."""
    rng = np.random.default_rng(seed)
    searches = R.make_set(rng, 120, R.STATES, CAP, 4)
    known = {sn.node.id: sn.node for s in searches for sn in s.nodes}
    cands = []
    for x in R.make_cands(rng, searches, 1200):
        if x not in known:
            expired = bool(rng.random() < 0.3)
            known[x] = R.Node(x, expired=expired, time=OLD if expired and rng.random() < 0.5 else NOW)
        cands.append(known[x])
    for _ in range(200):
        cands.insert(int(rng.integers(0, len(cands) + 1)), cands[int(rng.integers(0, len(cands)))])
    return searches, cands


old_a, old_b, old_c = (functools.partial(with_old, s) for s in (41, 42, 43))
INPUTS = {"adversarial": T.adversarial, "steady": T.steady, "old_a": old_a, "old_b": old_b, "old_c": old_c}


@functools.lru_cache(maxsize=None)
def sequential(name):
    """(the state after trySearchInsert of every candidate in order, how many candidates were old at their turn)."""
    searches, cands = INPUTS[name]()
    sids = [s.id for s in searches]
    n_old = 0
    for c in cands:
        n_old += F.removable(c, NOW)
        R.try_search_insert(searches, sids, c, NOW)
    return T.state_of(searches, cands), n_old


def model_set(searches):
    return I.ModelSearches(searches, CAP, NOW)


def check_tick(name, DS, searches, cands, max_rounds):
    counts = try_search_insert_device(DS, I.HostInsert(searches, cands, NOW), R.id_bytes([c.id for c in cands]), NOW,
                                      max_rounds)
    want, n_old = sequential(name)
    assert T.state_of(searches, cands) == want
    assert counts["skipped"] + counts["device"] + counts["host"] == len(cands), counts
    print(name, max_rounds, counts, "old:", n_old)
    if name == "steady" and max_rounds == 8:
        assert counts["host"] <= len(cands) // 100, counts  # the reference scheme alone gives 5 of 5000
    if max_rounds is None:
        assert counts["host"] == n_old, (counts, n_old)  # only the old candidates take the host path
    return counts


CASES = [("adversarial", None), ("adversarial", 8), ("steady", 8), ("steady", None), ("old_a", None), ("old_b", 8),
         ("old_c", None)]


@pytest.mark.parametrize("name,max_rounds", CASES)
def test_tick_with_reference_verdicts_and_the_model(name, max_rounds):
    searches, cands = INPUTS[name]()
    DS = model_set(searches)
    check_tick(name, DS, searches, cands, max_rounds)
    assert [s.key() for s in DS.s] == [I.from_search(s, NOW).key() for s in searches]


def test_old_inputs_hold_barriers_and_repeats():
    for name in ("old_a", "old_b", "old_c"):
        searches, cands = INPUTS[name]()
        assert len(searches) == 120 and len(cands) == 1400
        assert sequential(name)[1] >= 20 and len(cands) - len(set(c.id for c in cands)) >= 200
    assert sequential("adversarial")[1] >= 1 and sequential("steady")[1] == 0


def test_plan_insert_round_rules():
    """One round over the adversarial input's first verdicts: the three lists partition the candidates, ready
    candidates never share a search, and every pair is an accepting search or a stopper that trims."""
    searches, cands = T.adversarial()
    lb, fwd, back, stop = R.verdicts(searches, [c.id for c in cands], NOW)
    trims = T.trims_of(searches)
    skipped, ready, deferred = plan_insert_round(len(searches), lb, fwd, back, stop, trims)
    assert sorted(skipped + [j for j, _ in ready] + deferred) == list(range(len(cands)))
    assert skipped and ready and deferred
    seen = set()
    for j, pairs in ready:
        l, f, b = int(lb[j]), int(fwd[j]), int(back[j])
        for s, want in pairs:
            assert s not in seen
            seen.add(s)
            assert (want == 1 and l - b <= s < l + f) or (want == 0 and s in (l + f, l - b - 1) and trims[s])
        assert sum(w for _, w in pairs) == f + b
    for j in skipped:
        assert fwd[j] + back[j] == 0 and all(v in (R.END, R.FAR) for v in (int(stop[j]) & 15, int(stop[j]) >> 4))
    assert plan_insert_round(0, *R.verdicts([], [1, 2], NOW), np.zeros(0, bool)) == ([0, 1], [], [])


def trimming_refusal():
    """A live search with 16 good entries refuses a far candidate and drops its last two entries while doing so."""
    return [R.Search(1 << 100, False, [R.SearchNode(R.Node((1 << 100) ^ (i + 1))) for i in range(16)])], \
           [R.Node(R.MAX_ID)]


def old_member_elsewhere():
    """Searches A < B < C. X (below A, so its walk starts there) is expired long ago and a removable member of C; as a
    candidate A accepts it, which sets its time to `now`, and the full search B refuses it, so the walk never reaches C.
    Y then enters C: removeExpiredNode must not take X there."""
    a, b, c = 1 << 150, 1 << 155, 1 << 158
    x, y = R.Node(a - 7, expired=True, time=OLD), R.Node(c ^ 6)
    A = R.Search(a, False, [R.SearchNode(R.Node(a ^ (i + 1))) for i in range(3)])
    B = R.Search(b, False, [R.SearchNode(R.Node(b ^ (i + 1))) for i in range(14)])
    C = R.Search(c, False, [R.SearchNode(R.Node(c ^ (i + 1))) for i in range(3)] + [R.SearchNode(x)])
    return [A, B, C], [x, y]


def check_single(make, DS_of):
    searches, cands = make()
    ref, rc = make()
    for n in rc:
        R.try_search_insert(ref, [s.id for s in ref], n, NOW)
    DS = DS_of(searches)
    counts = try_search_insert_device(DS, I.HostInsert(searches, cands, NOW), R.id_bytes([c.id for c in cands]), NOW)
    assert T.state_of(searches, cands) == T.state_of(ref, rc)
    return DS, searches, counts


def test_trimming_refusal_runs_on_the_device_model():
    DS, searches, counts = check_single(trimming_refusal, model_set)
    assert len(searches[0].nodes) == 14 and len(DS.s[0].ents) == 14
    assert counts["host"] == 0 and counts["device"] == 1 and counts["pairs"] == 1 and counts["skipped"] == 0


def test_old_member_survives_elsewhere_model():
    DS, searches, counts = check_single(old_member_elsewhere, model_set)
    assert counts["host"] == 1 and counts["device"] == 1
    assert [s.key() for s in DS.s] == [I.from_search(s, NOW).key() for s in searches]
    assert any(sn.node.id == (1 << 150) - 7 for sn in searches[2].nodes) and len(searches[2].nodes) == 5


# ---- on the GPU ------------------------------------------------------------------------------------------------------
def assert_device_equals_host(DS, searches):
    got, want = DS.export(), F.expected_export(searches, DS.cap, NOW)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, bad[:4])


def device_set(searches):
    from opendht_amd import DeviceSearches

    return DeviceSearches(*F.snapshot(searches, NOW), cap=CAP, device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,max_rounds", CASES)
def test_try_search_insert_device_equals_sequential(gpu, name, max_rounds):
    searches, cands = INPUTS[name]()
    with device_set(searches) as DS:
        check_tick(name, DS, searches, cands, max_rounds)
        assert_device_equals_host(DS, searches)
        probe = R.id_bytes([c.id for c in cands[:300]])
        got = DS.try_insert_host(probe)
    for g, w in zip(got, R.verdicts(searches, [c.id for c in cands[:300]], NOW)):
        assert np.array_equal(g, w)


@pytest.mark.gpu
def test_trimming_refusal_runs_on_the_device(gpu):
    DS, searches, counts = check_single(trimming_refusal, device_set)
    with DS:
        assert len(searches[0].nodes) == 14
        assert counts["host"] == 0 and counts["device"] == 1 and counts["pairs"] == 1 and counts["skipped"] == 0
        assert_device_equals_host(DS, searches)


@pytest.mark.gpu
def test_old_member_survives_elsewhere(gpu):
    DS, searches, counts = check_single(old_member_elsewhere, device_set)
    with DS:
        assert counts["host"] == 1 and counts["device"] == 1
        assert_device_equals_host(DS, searches)
        assert any(sn.node.id == (1 << 150) - 7 for sn in searches[2].nodes) and len(searches[2].nodes) == 5
