"""The flag-level model of kad_sr_insert (insert_ref.py) against Search::insertNode as restated in
searches_ref.py, on every state of searches_ref.STATES with good and expired candidates, old expired ones included;
and a check that the cases of test_sr_insert.py contain every mechanism of the insert. CPU only."""
import numpy as np
import pytest

import insert_ref as I
import refill_ref as F
import searches_ref as R

NOW = I.NOW


@pytest.mark.parametrize("state,cap", [(s, c) for c in (14, 32, 64) for s in R.STATES if s != "trim" or c >= 16])
def test_model_equals_insert_node(state, cap):
    rng = np.random.default_rng(100 + cap)
    for rep in range(12):
        sid = int.from_bytes(rng.bytes(20), "big")
        ref = R.make_search(rng, sid, state, cap, now=NOW)
        if rep % 3 == 2 and ref.nodes:  # an expired search of the same list
            ref.expired = True
        model = I.from_search(ref, NOW)
        known = {sn.node.id: sn.node for sn in ref.nodes}
        for x, xfl in I.make_cand_list(rng, model, 40):
            node = known.get(x)
            if node is None:  # a stranger: good, expired, or expired long ago (its time becomes `now` on insert)
                node = known[x] = R.Node(x, expired=bool(xfl), time=F.TIMES[int(rng.integers(0, 4))])
            got = I.insert_one(model, x, I.SN_BAD if node.expired else 0)
            want = ref.insert_node(node, NOW)
            assert got == want, (state, cap, rep)
            assert model.key() == I.from_search(ref, NOW).key(), (state, cap, rep)


def test_model_refuses_as_the_reference_says():
    """The two single searches of the issue: a live search of 16 good entries trims while refusing; an expired search
    takes a BAD candidate without flipping and is cut to 14."""
    sid = 1 << 100
    s = I.FlagSearch(sid, False, [(sid ^ (i + 1), 0) for i in range(16)])
    assert not I.insert_one(s, R.MAX_ID, 0) and len(s.ents) == 14
    e = I.FlagSearch(sid, True, [(sid ^ (i + 1), I.SN_BAD) for i in range(13)])
    assert I.insert_one(e, sid ^ 14, I.SN_BAD) and e.expired and len(e.ents) == 14
    assert I.insert_one(e, sid, I.SN_BAD) and e.expired and len(e.ents) == 14 and e.ents[0][0] == sid
    assert not I.insert_one(e, sid ^ 100, 0) and e.expired  # full and beyond t: FAR_EXPIRED
    f = I.FlagSearch(sid, True, [(sid ^ (i + 2), I.SN_BAD) for i in range(13)])
    assert I.insert_one(f, sid ^ 1, 0) and not f.expired and len(f.ents) == 14  # a good one flips it, no pops


def test_cases_cover_the_mechanisms():
    """Passes on the model alone: every mechanism of the insert occurs in the GPU cases."""
    tot = I.new_stats()
    over = dup = 0
    counts, listed = set(), set()
    for name in I.CASES:
        c = I.case(name)
        for k, v in c["stats"].items():
            tot[k] += v
        over += int((c["status"] == I.INSERT_OVERFLOW).sum())
        counts |= set(len(x) for x in c["lists"])
        listed.add(len(c["which"]))
        for lst in c["lists"]:
            dup += len(lst) - len(set(x[0] for x in lst))
    for k, v in tot.items():
        assert v >= 5, (k, tot)
    assert over >= 5 and dup >= 5
    assert counts >= set(I.COUNTS) and {63, 64, 65} <= listed
    assert {I.CASES[n][1] for n in I.CASES} == {14, 32, 64}
    assert {I.CASES[n][0] for n in I.CASES} >= {0, 1, 3, 65, 300}
    # an overflowing search with a succeeding one on either side, in one call
    ok = False
    for name in I.CASES:
        st = I.case(name)["status"]
        ins = I.case(name)["ins"]
        off = I.csr(I.case(name)["lists"])[0]
        for k in range(1, len(st) - 1):
            took = [bool(ins[off[i]:off[i + 1]].any()) for i in (k - 1, k + 1)]
            ok |= st[k] == I.INSERT_OVERFLOW and st[k - 1] == st[k + 1] == I.INSERT_OK and all(took)
    assert ok
