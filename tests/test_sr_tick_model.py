"""opendht_amd.try_search_insert_tick over a device set made of the flag-level model
(tick_ref.TickModel: the model's verdicts, the engine's planner, the model's insert): the seven cases of
test_sr_insert_ingest.py end in the state of the sequential reference, with the counts try_search_insert_device returns on
a twin model set. CPU only."""
import pytest

import insert_ref as I
import searches_ref as R
import test_search_ingest as T
import test_sr_insert_ingest as G
import tick_ref as K
from opendht_amd.searches import try_search_insert_device, try_search_insert_tick

CAP, NOW = G.CAP, G.NOW


def run_both(name, max_rounds, make_set):
    """(counts of the tick, counts of try_search_insert_device on a twin, the tick's set and searches)"""
    searches, cands = G.INPUTS[name]()
    ids = R.id_bytes([c.id for c in cands])
    DS = make_set(searches)
    counts = try_search_insert_tick(DS, I.HostInsert(searches, cands, NOW), ids, NOW, max_rounds)
    want, n_old = G.sequential(name)
    assert T.state_of(searches, cands) == want
    assert counts["skipped"] + counts["device"] + counts["host"] == len(cands), counts
    if max_rounds is None:
        assert counts["host"] == n_old, (counts, n_old)
    twin_searches, twin_cands = G.INPUTS[name]()
    twin = make_set(twin_searches)
    twin_counts = try_search_insert_device(twin, I.HostInsert(twin_searches, twin_cands, NOW), ids, NOW, max_rounds)
    assert counts == twin_counts
    return DS, searches, twin


@pytest.mark.parametrize("name,max_rounds", G.CASES)
def test_tick_over_the_model_equals_sequential(name, max_rounds):
    DS, searches, twin = run_both(name, max_rounds, lambda s: K.TickModel(s, CAP, NOW))
    assert [s.key() for s in DS.s] == [I.from_search(s, NOW).key() for s in searches]
    assert [s.key() for s in DS.s] == [s.key() for s in twin.s]


def test_single_cases_over_the_model():
    for make, device, pairs in ((G.trimming_refusal, 1, 1), (G.old_member_elsewhere, 1, None)):
        searches, cands = make()
        ref, rc = make()
        for n in rc:
            R.try_search_insert(ref, [s.id for s in ref], n, NOW)
        DS = K.TickModel(searches, CAP, NOW)
        counts = try_search_insert_tick(DS, I.HostInsert(searches, cands, NOW), R.id_bytes([c.id for c in cands]), NOW)
        assert T.state_of(searches, cands) == T.state_of(ref, rc)
        assert [s.key() for s in DS.s] == [I.from_search(s, NOW).key() for s in searches]
        assert counts["device"] == device and (pairs is None or counts["pairs"] == pairs), counts
