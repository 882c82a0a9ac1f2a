"""kad_sr_mark_entries against step_ref.mark_entries: found and not found pairs, an ID that only a
padding slot could match (the zero ID, in a search with room left), an ID another search holds, a member's 64-bit key with
another tail, ops that change nothing, the pairs in any order; the export afterwards equals the model's (records
untouched: no step bit moves t, full or the threshold), and the step that follows sees the new bits. Sets of 3 and 300
searches with slabs of 14, 32 and 64 entries; 0, 1, 257 pairs."""
import numpy as np
import pytest

import insert_ref as I
import searches_ref as R
import step_ref as T
from opendht_amd import DeviceSearches, KadError, _lib


def make_pairs(rng, searches, p):
    """p distinct (search, ID, clear, set): members, the zero ID, another search's member, a member's key with another
    tail, strangers; a fifth of the ops change nothing."""
    S, out, seen = len(searches), [], set()
    while len(out) < p:
        kind, s = int(rng.integers(0, 6)), int(rng.integers(0, S))
        ents = searches[s].ents
        if kind <= 1 and ents:
            x = ents[int(rng.integers(0, len(ents)))][0]
        elif kind == 2:
            x = 0
        elif kind == 3:
            o = searches[int(rng.integers(0, S))].ents
            x = o[0][0] if o else 1
        elif kind == 4 and ents:
            x = (ents[0][0] >> 96 << 96) | int.from_bytes(rng.bytes(12), "big")
        else:
            x = int.from_bytes(rng.bytes(20), "big")
        if (s, x) in seen:
            continue
        seen.add((s, x))
        bits = [int(b) for b in rng.permutation([T.CAND, T.PEND, T.SYNC, T.NOGET])]
        k = int(rng.integers(0, 4))
        clear, setb = sum(bits[:k]), sum(bits[k:int(rng.integers(k, 5))])
        if len(out) % 5 == 4:
            clear, setb = 0, 0
        out.append((s, x, clear, setb))
    return out


def call(DS, pairs):
    return DS.mark_entries(np.array([p[0] for p in pairs], np.uint32),
                           R.id_bytes([p[1] for p in pairs]) if pairs else np.zeros((0, 20), np.uint8),
                           np.array([p[2] for p in pairs], np.uint8), np.array([p[3] for p in pairs], np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("S,cap,p", [(3, 14, 1), (3, 64, 0), (300, 14, 257), (300, 32, 257), (300, 64, 257)])
def test_mark_entries_equals_the_model(gpu, S, cap, p):
    searches = T.step_set(S, cap, 50 + cap)
    rng = np.random.default_rng(cap + p)
    pairs = make_pairs(rng, searches, p)
    after, found = T.mark_entries(searches, pairs)
    if p > 1:
        assert 0 < found.sum() < p
        assert any(x == 0 for _, x, _, _ in pairs) and not any(x == 0 and f for (_, x, _, _), f in zip(pairs, found))
    want_export = I.expected_export(after, cap)
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        got = call(DS, pairs)
        assert np.array_equal(got, found)
        ex = DS.export()
        for k in want_export:
            assert np.array_equal(ex[k], want_export[k]), k
        T.assert_step(DS.step(), T.device_step(after, None, 0)[1:], "step after")
        # the same ops again change nothing; the clears and sets swapped bring the cleared bits back only where they were set
        assert np.array_equal(call(DS, pairs), found)
        ex = DS.export()
        for k in want_export:
            assert np.array_equal(ex[k], want_export[k]), k


@pytest.mark.gpu
def test_mark_entries_checks_that_need_a_set(gpu):
    searches = T.step_set(5, 32, 2)
    x = next(s for s in range(5) if searches[s].ents)
    node = searches[x].ents[0][0]
    L = _lib.lib()
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        for pairs, what in (([(5, node, 0, T.SYNC)], b"not below S"),
                            ([(x, node, 0, T.SYNC), (x, node, T.PEND, 0)], b"are equal"),
                            ([(x, node, T.SYNC, T.SYNC)], b"both cleared and set"),
                            ([(x, node, 0, I.SN_BAD)], b"outside the step bits")):
            with pytest.raises(KadError) as e:
                call(DS, pairs)
            assert e.value.code == _lib.KAD_ERR_INVALID and what in L.kad_last_error()
        ex, want = DS.export(), I.expected_export(searches, 32)
        for k in want:
            assert np.array_equal(ex[k], want[k]), k
        # NULL bit arrays are all zero, NULL out_found is allowed
        ids = R.id_bytes([node])
        pw = np.array([x], np.uint32)
        assert L.kad_sr_mark_entries(DS._h, 1, _lib.ptr(pw), _lib.ptr(ids), None, None, None) == 0
        assert DS.mark_entries(pw, ids)[0] == 1
        ex = DS.export()
        for k in want:
            assert np.array_equal(ex[k], want[k]), k
