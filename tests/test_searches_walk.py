"""The device set of live searches through kad_sr_refill and kad_searches_patch in turn: refill of the even searches,
a patch of a third of the set (grown, shrunk and flag-flipped lists, half of them refilled just before), a refill of the
odd searches and of the patched even ones, a patch of the searches that refill overflowed, and two refills of the whole
set. After every step the export equals the one of a set created from the restated searches (refill_ref), and
trySearchInsert verdicts equal both a freshly created set's and the restatement's (searches_ref.verdicts); every
refill's rows, counts, insert masks and statuses equal refill_ref.device_refill on the model. 300 searches over a cache
of 3000 nodes, slabs of 32 and of 64 entries; the model is built once per slab size and shared."""
import functools

import numpy as np
import pytest

import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable

NOW = F.NOW
CAPS = (32, 64)
# the refill_ref.make_search state a patched search gets: a longer list, a shorter one, or the other `expired` flag
GROW, SHRINK, EXPIRE, REVIVE = "cap", "notfull", "expired", "full"


def _patched(rng, s, cap, cache, k):
    """Search s in a new, valid state: grown to the slab's size, shrunk, flipped to expired, or (an expired one) live."""
    state = REVIVE if s.expired else (GROW, SHRINK, EXPIRE, "empty")[k % 4]
    return F.make_search(rng, s.id, state, cap, cache)


@functools.lru_cache(maxsize=None)
def walk(cap):
    """The whole sequence on the restatement: {"cache", "base", "start", "steps"}; a step is ("refill", which, after,
    rows, cnt, ins, status) or ("patch", which, after). Built once, never changed."""
    rng = np.random.default_rng(0x5EA0 + cap)
    cache = F.make_cache(rng, 3000)
    start = F.make_set(rng, 300, F.states_for(cap), cap, cache)
    base = 1000 if cap == 32 else 0
    S = len(start)
    steps = []

    def refill(cur, which):
        after, rows, cnt, ins, status = F.device_refill(cur, cache, [int(s) for s in which], NOW, cap, base)
        steps.append(("refill", np.asarray(which, np.uint32), after, rows, cnt, ins, status))
        return after, status

    def patch(cur, which, new):
        after = list(cur)
        for s, x in zip(which, new):
            after[int(s)] = x
        steps.append(("patch", np.asarray(which, np.uint32), after))
        return after

    a = np.arange(0, S, 2)
    cur, _ = refill(start, a)                                                       # 1
    third = np.arange(0, S, 3)  # every second one is even: refilled in step 1, patched now
    cur = patch(cur, third, [_patched(rng, cur[int(s)], cap, cache, k) for k, s in enumerate(third)])  # 2
    w3 = np.union1d(np.arange(1, S, 2), third[third % 2 == 0])
    cur, status = refill(cur, w3)                                                   # 3
    over = w3[status == F.REFILL_OVERFLOW]
    new = []
    for s in over:  # as refill_searches: the host's own refill, uploaded when it fits the slab; a shorter list otherwise
        c = cur[int(s)].copy()
        F.refill(c, cache, NOW)
        new.append(c if len(c.nodes) <= cap else F.make_search(rng, c.id, SHRINK, cap, cache))
    cur = patch(cur, over, new)                                                     # 4
    cur, _ = refill(cur, np.arange(S))                                              # 5
    refill(cur, np.arange(S))                                                       # 6
    return {"cache": cache, "base": base, "start": start, "steps": steps}


@pytest.mark.parametrize("cap", CAPS)
def test_every_refill_meets_patched_searches(cap):
    """Passes on the restatement alone: every refill after the first lists at least 5 searches the patch before it
    changed, step 3 overflows at least one search and step 4 patches it, the patches hold grown, shrunk and
    flag-flipped lists, and the last refill inserts nothing into a search it reports as refilled."""
    w = walk(cap)
    steps = w["steps"]
    assert [s[0] for s in steps] == ["refill", "patch", "refill", "patch", "refill", "refill"]
    for j in (2, 4, 5):  # each refill after the first against the last patch before it
        p = steps[1] if j == 2 else steps[3]
        before = steps[0][2] if j == 2 else steps[2][2]
        changed = {int(s) for s in p[1] if p[2][int(s)] is not before[int(s)]}
        assert len(changed & {int(s) for s in steps[j][1]}) >= 5, (j, len(changed))
    over = steps[2][1][steps[2][6] == F.REFILL_OVERFLOW]
    assert len(over) >= 1 and np.array_equal(steps[3][1], over)
    was, now = steps[0][2], steps[1][2]
    grown = sum(len(now[int(s)].nodes) > len(was[int(s)].nodes) for s in steps[1][1])
    shrunk = sum(len(now[int(s)].nodes) < len(was[int(s)].nodes) for s in steps[1][1])
    flipped = sum(now[int(s)].expired != was[int(s)].expired for s in steps[1][1])
    refilled = sum(was[int(s)] is not w["start"][int(s)] for s in steps[1][1])
    assert min(grown, shrunk, flipped, refilled) >= 5, (grown, shrunk, flipped, refilled)
    last = steps[5]
    assert (last[5][last[6] == F.REFILL_OK] == 0).all()


def assert_export(DS, searches, tag):
    got, want = DS.export(), F.expected_export(searches, DS.cap, NOW)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


def csr(searches, which):
    st = [F.search_state(searches[int(s)], NOW) for s in which]
    off = np.zeros(len(st) + 1, np.uint32)
    off[1:] = np.cumsum([x[1].shape[0] for x in st])
    return (np.array([x[0] for x in st], np.uint8), off,
            np.concatenate([x[1] for x in st] + [np.zeros((0, 20), np.uint8)]),
            np.concatenate([x[2] for x in st] + [np.zeros(0, np.uint8)]))


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
def test_refill_patch_refill(gpu, cap):
    w = walk(cap)
    ids, status = w["cache"].table_arrays()
    with DeviceTable(ids, status, device=0, index_base=w["base"], sorted=True) as NC, \
            DeviceSearches(*F.snapshot(w["start"], NOW), cap=cap, device=0) as DS:
        assert_export(DS, w["start"], "start")
        for j, step in enumerate(w["steps"]):
            tag = f"step {j + 1} {step[0]}"
            which, after = step[1], step[2]
            if step[0] == "refill":
                rows, cnt, ins, status = DS.refill(NC, which)
                assert np.array_equal(rows, step[3]) and np.array_equal(cnt, step[4]), tag
                bad = np.flatnonzero((ins != step[5]) | (status != step[6]))
                assert bad.size == 0, (tag, bad[:5], ins[bad[:5]], step[5][bad[:5]], status[bad[:5]], step[6][bad[:5]])
            else:
                DS.patch(which, *csr(after, which))
            assert_export(DS, after, tag)
            cands = R.make_cands(np.random.default_rng(5), after, 257)
            with DeviceSearches(*F.snapshot(after, NOW), cap=cap, device=0) as fresh:
                got, want = DS.try_insert_host(R.id_bytes(cands)), fresh.try_insert_host(R.id_bytes(cands))
            for g, x, r in zip(got, want, R.verdicts(after, cands, NOW)):
                assert np.array_equal(g, x) and np.array_equal(g, r), tag
        assert (ins[status == F.REFILL_OK] == 0).all()
