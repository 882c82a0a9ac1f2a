"""kad_sr_step against step_ref's entry-by-entry searchStep over flag-level sets (pinned to the closed
form's host twin by test_sr_step_model.py). Per case: every search's output equals the model in verdict mode, with
which = NULL and with which = range(S), and the export stays byte-identical; a scattered which with mixed modes (APPLY,
NO_SEND, DONE_IF_SYNCED, NO_EXPIRE in one call) equals the model and leaves the model's export; a second APPLY call over
the whole set picks only what the first left room for; an expired search's record and slab are those of a freshly created
empty expired search, and trySearchInsert verdicts over the stepped set equal those of a twin created from the model. The
shapes are the smallest at which each path can break: sets of 0, 1, 63, 64, 65 and 257 searches (one lane per search,
blocks of 256) and 5000, slabs of 14 and 20 entries (the byte path, slabs starting at any byte), 16, 32, 48 and 64 (one
to four 16-byte units); 65 is refused. The first half of every set is the named cases of step_ref."""
import numpy as np
import pytest

import insert_ref as I
import searches_ref as R
import step_ref as T
from opendht_amd import DeviceSearches, KadError, _lib

CASES = [(S, 32) for S in (0, 1, 63, 64, 65, 257, 5000)] + [(257, cap) for cap in (14, 16, 20, 48, 64)] + \
        [(5000, 14), (5000, 64), (65, 20)]


def assert_export(DS, searches, tag):
    got, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


def mixed_modes(rng, m, apply_part):
    md = rng.choice([0, T.NO_SEND, T.DONE_IF_SYNCED, T.NO_EXPIRE, T.DONE_IF_SYNCED | T.NO_EXPIRE], size=m).astype(np.uint8)
    md[rng.random(m) < apply_part] |= T.APPLY
    return md


def candidates(rng, searches, q):
    out = []
    for k in range(q):
        s = searches[int(rng.integers(0, len(searches)))]
        v = int.from_bytes(rng.bytes(20), "big")
        out.append((v, s.id, s.id ^ 1, s.id ^ (v >> 150), s.ents[0][0] if s.ents else v,
                    s.id ^ (v >> int(rng.integers(8, 150))))[k % 6])
    return R.id_bytes(out)


@pytest.mark.gpu
@pytest.mark.parametrize("S,cap", CASES)
def test_step_equals_the_model(gpu, S, cap):
    searches = T.step_set(S, cap, 7 * S + cap)
    rng = np.random.default_rng(S + cap)
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        first = DS.export()
        # verdict mode over the whole set: only read
        md = mixed_modes(rng, S, 0.0)
        want = T.device_step(searches, None, md)
        got = DS.step(None, md)
        T.assert_step(got, want[1:], "all")
        st = got["stats"]
        assert st["picks"] == sum(bin(int(v)).count("1") for v in want[1])
        assert st["synced"] == int(((want[6] & T.SYNCED) != 0).sum()) and st["kernel_ms"] >= 0.0
        assert st["expired"] == int(((want[6] & T.EXPIRE) != 0).sum())
        assert st["skipped"] == int(((want[6] & T.SKIPPED) != 0).sum())
        listed = DS.step(np.arange(S, dtype=np.uint32), md)
        for k in ("picks", "n", "bad", "lead_bad", "solicited", "bits"):
            assert np.array_equal(listed[k], got[k]), k
        T.assert_step(DS.step(), T.device_step(searches, None, 0)[1:], "mode NULL")
        back = DS.export()
        for k in first:
            assert np.array_equal(back[k], first[k]), k
        if S == 0:
            return
        # a scattered which with every mode in one call
        which = np.sort(rng.choice(S, size=max(1, S // 3), replace=False)).astype(np.uint32)
        md = mixed_modes(rng, which.shape[0], 0.6)
        after = T.device_step(searches, which, md)
        T.assert_step(DS.step(which, md), after[1:], "scattered")
        assert_export(DS, after[0], "scattered")
        # APPLY over the whole set, twice: the second call sends only where the first left room
        once = T.device_step(after[0], None, T.APPLY)
        T.assert_step(DS.step(None, T.APPLY), once[1:], "apply")
        assert_export(DS, once[0], "apply")
        twice = T.device_step(once[0], None, T.APPLY)
        got = DS.step(None, T.APPLY)
        T.assert_step(got, twice[1:], "apply again")
        assert_export(DS, twice[0], "apply again")
        live = (twice[6] & T.SKIPPED) == 0
        assert (got["solicited"][live] <= np.maximum(4, once[5][live])).all()
        assert not (got["picks"] & once[1]).any()  # nothing is sent twice
        # the expired searches are fresh empty expired searches, and the verdict kernel cannot tell the set from a twin
        gone = [s for s in range(S) if twice[0][s].expired and not searches[s].expired]
        if S >= 63:
            assert gone
        ex = DS.export()
        for s in gone:
            assert ex["flags"][s] == 1 and ex["n"][s] == 0 and ex["t"][s] == 0 and ex["full"][s] == 0
            assert not ex["node_ids"][s].any() and not ex["node_flags"][s].any()
        cands = candidates(rng, twice[0], 257)
        with DeviceSearches(*I.snapshot(twice[0]), cap=cap, device=0) as twin:
            for a, b in zip(DS.try_insert_host(cands), twin.try_insert_host(cands)):
                assert np.array_equal(a, b)


@pytest.mark.gpu
def test_named_cases_on_the_device(gpu):
    """Every named case as one search of a set with slabs of 64 entries, under its own mode plus APPLY."""
    names = list(T.NAMED)
    rng = np.random.default_rng(3)
    searches = T.make_step_set(rng, len(names), 64, [(T.NAMED[k][0], T.NAMED[k][1]) for k in names])
    md = np.array([T.NAMED[k][2] | T.APPLY for k in names], np.uint8)
    want = T.device_step(searches, None, md)
    with DeviceSearches(*I.snapshot(searches), cap=64, device=0) as DS:
        got = DS.step(None, md)
        T.assert_step(got, want[1:], "named")
        assert_export(DS, want[0], "named")
    for k, name in enumerate(names):
        by_hand = T.step(*T.NAMED[name])
        assert [e for e in range(64) if (int(got["picks"][k]) >> e) & 1] == by_hand[0], name
        assert int(got["bits"][k]) == by_hand[5], name
    no_expire = names.index("no_expire")
    assert want[6][no_expire] & T.EXPIRE and not want[0][no_expire].expired and want[0][no_expire].ents


@pytest.mark.gpu
def test_step_checks_that_need_a_set(gpu):
    searches = T.step_set(5, 32, 1)
    L = _lib.lib()
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        before = DS.export()
        for which, modes, what in ((None, np.array([0, 0, 0x10, 0, 0], np.uint8), b"mode bit"),
                                   ([0, 2, 2], None, b"ascending"), ([1, 5], None, b"ascending"),
                                   ([3, 1], [T.APPLY, T.APPLY], b"ascending")):
            with pytest.raises(KadError):
                DS.step(which, modes)
            assert what in L.kad_last_error()
        out = np.zeros(3, _lib.STEP_OUT_DTYPE)
        assert L.kad_sr_step(DS._h, 3, None, None, _lib.ptr(out), None) == _lib.KAD_ERR_INVALID  # m != S
        after = DS.export()
        for k in before:
            assert np.array_equal(after[k], before[k]), k
        assert DS.step([], None)["picks"].shape == (0,)
    with DeviceSearches(*I.snapshot(searches), cap=65, device=0) as DS:
        with pytest.raises(KadError) as e:
            DS.step(None, T.APPLY)
        assert e.value.code == _lib.KAD_ERR_UNSUPPORTED
        with pytest.raises(KadError) as e:
            DS.mark_entries([0], R.id_bytes([1]), None, [T.SYNC])
        assert e.value.code == _lib.KAD_ERR_UNSUPPORTED
        assert_export(DS, searches, "cap 65")
