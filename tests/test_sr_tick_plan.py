"""kad_sr_plan_round (kadplan::sr_round_plan) against opendht_amd.plan_insert_round: the same kinds and
the same pairs for the verdicts of the first three rounds of the adversarial, the steady and the three with_old inputs of
test_sr_insert_ingest.py (the ready candidates of a round applied on the reference searches before the next), and for
hand-made rounds: no searches, no candidates, a long accepting run, equal IDs back to back, a deferred candidate with an
open stop that blocks a later disjoint one. CPU only."""
import numpy as np
import pytest

import searches_ref as R
import test_search_ingest as T
import test_sr_insert_ingest as G
import tick_ref as K
from opendht_amd.searches import plan_round

NOW = T.NOW
END, KNOWN, FAR, FAR_EXPIRED = R.END, R.KNOWN, R.FAR, R.FAR_EXPIRED


def both_plans(S, lb, fwd, back, stop, trims):
    want_kind, want_pairs = K.python_plan(S, lb, fwd, back, stop, trims)
    kind, pairs = K.native_plan(S, lb, fwd, back, stop, K.trim_bits(lb, fwd, back, stop, trims))
    assert np.array_equal(kind, want_kind), np.flatnonzero(kind != want_kind)[:8]
    assert pairs == want_pairs
    return kind


@pytest.mark.parametrize("name", list(G.INPUTS))
def test_three_rounds_equal_plan_insert_round(name):
    searches, cands = G.INPUTS[name]()
    sids = [s.id for s in searches]
    rem = list(range(len(cands)))
    seen = set()
    for _ in range(3):
        v = R.verdicts(searches, [cands[j].id for j in rem], NOW)
        kind = both_plans(len(searches), *v, T.trims_of(searches))
        seen |= set(int(k) for k in kind)
        for k in np.flatnonzero(kind == K.READY):  # the ready candidates never meet: any order is the sequential one
            R.try_search_insert(searches, sids, cands[rem[k]], NOW)
        rem = [rem[k] for k in np.flatnonzero(kind == K.DEFERRED)]
        if not rem:
            break
    assert {K.SKIPPED, K.READY} <= seen and (name == "steady" or K.DEFERRED in seen)


def arrays(rows):
    """rows of (lb, fwd, back, fstop, bstop)"""
    a = np.array(rows, np.int64).reshape(-1, 5)
    return (a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32),
            (a[:, 3] | a[:, 4] << 4).astype(np.uint8))


def test_no_searches_and_no_candidates():
    kind, pw, pc, want = plan_round(0, *arrays([(0, 0, 0, END, END)] * 3), np.zeros(3, np.uint8))
    assert list(kind) == [K.SKIPPED] * 3 and len(pw) == len(pc) == len(want) == 0
    kind, pw, _, _ = plan_round(7, *arrays([]), np.zeros(0, np.uint8))
    assert len(kind) == 0 and len(pw) == 0
    both_plans(0, *arrays([(0, 0, 0, END, END)] * 2), np.zeros(0, bool))


def test_a_run_of_forty_empty_searches_takes_one_candidate():
    """lb = 17 of 40 searches, all accepting: 23 forwards and 17 backwards, both walks run off the ends; a second
    candidate anywhere waits."""
    v = arrays([(17, 23, 17, END, END), (3, 0, 0, FAR, FAR), (3, 1, 0, FAR, FAR)])
    kind = both_plans(40, *v, np.zeros(40, bool))
    assert list(kind) == [K.READY, K.SKIPPED, K.DEFERRED]
    _, pw, pc, want = plan_round(40, *v, np.zeros(3, np.uint8))
    assert list(pw) == list(range(40)) and not pc.any() and want.all()
    # 300 searches: an interval that covers whole bitmap words, one that ends inside a word
    v = arrays([(100, 150, 90, FAR, KNOWN), (260, 0, 0, FAR, FAR), (255, 3, 4, FAR, FAR), (5, 2, 0, FAR, FAR)])
    trims = np.zeros(300, bool)
    trims[[250, 259, 258]] = True
    kind = both_plans(300, *v, trims)
    assert list(kind) == [K.READY, K.READY, K.DEFERRED, K.READY]


def test_equal_ids_back_to_back():
    """The same verdict twice: the first is ready, the second waits for it (the next round finds it KNOWN)."""
    kind = both_plans(20, *arrays([(5, 2, 1, FAR, FAR)] * 2 + [(12, 0, 0, FAR, FAR)] * 2), np.zeros(20, bool))
    assert list(kind) == [K.READY, K.DEFERRED, K.SKIPPED, K.SKIPPED]
    trims = np.zeros(20, bool)
    trims[12] = True
    kind = both_plans(20, *arrays([(12, 0, 0, FAR, FAR)] * 2), trims)
    assert list(kind) == [K.READY, K.DEFERRED]


@pytest.mark.parametrize("fstop,bstop,blocked_above,blocked_below", [(KNOWN, FAR, True, False), (FAR, FAR_EXPIRED, False, True),
                                                                     (FAR_EXPIRED, KNOWN, True, True), (FAR, FAR, False, False)])
def test_an_open_stop_blocks_disjoint_candidates(fstop, bstop, blocked_above, blocked_below):
    """Candidate 1 meets candidate 0 and waits; its open stops may let it walk on next round, so candidates far above or
    below it wait too, although their searches are disjoint from everything seen."""
    rows = [(10, 1, 0, FAR, FAR), (11, 1, 1, fstop, bstop), (30, 1, 0, FAR, FAR), (3, 1, 0, FAR, FAR)]
    kind = both_plans(40, *arrays(rows), np.zeros(40, bool))
    assert list(kind) == [K.READY, K.DEFERRED, K.DEFERRED if blocked_above else K.READY,
                          K.DEFERRED if blocked_below else K.READY]


def test_verdicts_outside_the_searches_are_refused():
    for row in ((9, 0, 0, END, END), (5, 4, 0, END, END), (2, 0, 3, END, END), (7, 1, 0, FAR, FAR), (0, 1, 0, FAR, FAR),
                (3, 0, 0, 4, END)):
        with pytest.raises(ValueError):
            plan_round(8, *arrays([row]), np.zeros(1, np.uint8))
