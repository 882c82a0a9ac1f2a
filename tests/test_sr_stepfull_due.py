"""kad_sr_mark_due against step_ref.mark_entries (the model does not care which bits it is given):
found and not found pairs, the zero ID against padding slots, an ID another search holds, a member's 64-bit key with
another tail, ops that change nothing; the export afterwards equals the model's, so the step bits of the same byte are
untouched, and kad_sr_mark_entries in turn leaves the due bits; the step that follows sees the new bits. Sets of 3 and 300
searches with slabs of 14, 32 and 64 entries; 0, 1, 257 pairs."""
import numpy as np
import pytest

import insert_ref as I
import searches_ref as R
import step_ref as T
import stepfull_ref as F
from opendht_amd import DeviceSearches, KadError, _lib


def make_pairs(rng, searches, p, bits):
    """p distinct (search, ID, clear, set) over `bits`: members, the zero ID, another search's member, a member's key
    with another tail, strangers; a fifth of the ops change nothing."""
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
        order = [int(b) for b in rng.permutation(bits)]
        k = int(rng.integers(0, len(bits) + 1))
        clear, setb = sum(order[:k]), sum(order[k:int(rng.integers(k, len(bits) + 1))])
        if len(out) % 5 == 4:
            clear, setb = 0, 0
        out.append((s, x, clear, setb))
    return out


def call(fn, pairs):
    return fn(np.array([p[0] for p in pairs], np.uint32),
              R.id_bytes([p[1] for p in pairs]) if pairs else np.zeros((0, 20), np.uint8),
              np.array([p[2] for p in pairs], np.uint8), np.array([p[3] for p in pairs], np.uint8))


def assert_export(DS, searches, tag):
    ex, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        assert np.array_equal(ex[k], want[k]), (tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize("S,cap,p", [(3, 14, 1), (3, 64, 0), (300, 14, 257), (300, 32, 257), (300, 64, 257)])
def test_mark_due_equals_the_model(gpu, S, cap, p):
    searches = F.full_set(S, cap, 70 + cap)
    rng = np.random.default_rng(cap + p)
    pairs = make_pairs(rng, searches, p, [F.LDUE, F.ADUE])
    after, found = T.mark_entries(searches, pairs)
    if p > 1:
        assert 0 < found.sum() < p
        assert any(x == 0 for _, x, _, _ in pairs) and not any(x == 0 and f for (_, x, _, _), f in zip(pairs, found))
        assert any(a is not b for a, b in zip(after, searches))
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        assert np.array_equal(call(DS.mark_due, pairs), found)
        assert_export(DS, after, "due")  # every other bit of every byte, the step bits among them, as it was
        md = F.draw_modes(rng, S, 0.0)
        F.assert_step_full(DS.step_full(None, md), F.device_step_full(after, None, md)[1:], "step after")
        assert np.array_equal(call(DS.mark_due, pairs), found)  # the same ops again change nothing
        assert_export(DS, after, "due again")
        # the reverse: kad_sr_mark_entries on the same entries leaves the due bits
        steps = [(s, x, c >> 4, st >> 4) for s, x, c, st in pairs]  # 0x40 -> 0x04 (CANDIDATE), 0x80 -> 0x08 (PENDING)
        both, found2 = T.mark_entries(after, steps)
        assert np.array_equal(call(DS.mark_entries, steps), found2) and np.array_equal(found2, found)
        assert_export(DS, both, "entries")


@pytest.mark.gpu
def test_mark_due_checks_that_need_a_set(gpu):
    searches = F.full_set(5, 32, 2)
    x = next(s for s in range(5) if searches[s].ents)
    node = searches[x].ents[0][0]
    L = _lib.lib()
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        for pairs, what in (([(5, node, 0, F.LDUE)], b"not below S"),
                            ([(x, node, 0, F.LDUE), (x, node, F.ADUE, 0)], b"are equal"),
                            ([(x, node, F.ADUE, F.ADUE)], b"both cleared and set"),
                            ([(x, node, 0, T.SYNC)], b"outside the due bits"),
                            ([(x, node, I.SN_BAD, 0)], b"outside the due bits")):
            with pytest.raises(KadError) as e:
                call(DS.mark_due, pairs)
            assert e.value.code == _lib.KAD_ERR_INVALID and what in L.kad_last_error()
        with pytest.raises(KadError):  # and the due bits stay refused where the step bits are set
            call(DS.mark_entries, [(x, node, 0, F.LDUE)])
        assert b"outside the step bits" in L.kad_last_error()
        assert_export(DS, searches, "refused")
        # NULL bit arrays are all zero, NULL out_found is allowed
        ids = R.id_bytes([node])
        pw = np.array([x], np.uint32)
        assert L.kad_sr_mark_due(DS._h, 1, _lib.ptr(pw), _lib.ptr(ids), None, None, None) == 0
        assert DS.mark_due(pw, ids)[0] == 1
        assert_export(DS, searches, "no ops")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [14, 32])
def test_create_patch_and_export_carry_the_due_bits(gpu, cap):
    """kad_searches_create and _export pass all eight bits of a member's byte, and kad_searches_patch writes the lists it
    is given with theirs: a third of the searches patched to the same lists with the due bits flipped."""
    searches = F.full_set(90, cap, 90 + cap)
    which = np.arange(1, 90, 3, dtype=np.uint32)
    after = list(searches)
    for s in which:
        x = searches[s]
        after[s] = I.FlagSearch(x.id, x.expired, [(y, f ^ F.DUE_BITS) for y, f in x.ents])
    assert any(f & F.DUE_BITS for s in which for f in [e[1] for e in searches[s].ents])
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        assert_export(DS, searches, "create")
        _, flags, off, node_ids, node_flags = I.snapshot([after[s] for s in which])
        DS.patch(which, flags, off, node_ids, node_flags)
        assert_export(DS, after, "patch")
