"""kad_sr_step_full against stepfull_ref's entry-by-entry loops over flag-level sets and against
kad_search_step_full_batch on the exported bytes. Per case: verdict mode with which = NULL and which = range(S) equals
both and leaves the export byte-identical; a scattered which carrying every valid mode in one call; after APPLY the
export is the issue's byte rule applied to the yardstick's picks (stepfull_ref.device_step_full checks the rule against
what its loops left); a second APPLY call sends nothing twice; expired searches are freshly created empty expired ones;
without LISTEN and ANNOUNCE the results and the set after APPLY are kad_sr_step's on a twin. The shapes are the smallest
at which each path can break: sets of 0, 1, 63, 64, 65 and 257 searches (one lane per search, blocks of 256) and 5000,
slabs of 14 and 20 entries (the byte path), 16, 32, 48 and 64 (one to four 16-byte units), and sets whose lists fill
slabs of 48 and 64, so that picks fall in every unit; 65 is refused. The first half of a set is the named cases."""
import numpy as np
import pytest

import insert_ref as I
import step_ref as T
import stepfull_ref as F
from opendht_amd import DeviceSearches, KadError, _lib, search_step_full_batch

CASES = [(S, 32, False) for S in (0, 1, 63, 64, 65, 257, 5000)] + [(257, cap, False) for cap in (14, 16, 20, 48, 64)] + \
        [(257, 48, True), (257, 64, True)]
OLD = ("picks", "n", "bad", "lead_bad", "solicited", "bits")


def assert_export(DS, searches, tag):
    got, want = DS.export(), I.expected_export(searches, DS.cap)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


def host_twin(DS, which, md):
    """kad_search_step_full_batch on the exported bytes of the searches `which` (None: all)."""
    ex = DS.export()
    idx = np.arange(DS.S) if which is None else np.asarray(which, np.int64)
    n = ex["n"][idx].astype(np.int64)
    off = np.zeros(idx.shape[0] + 1, np.uint32)
    off[1:] = np.cumsum(n)
    flat = np.concatenate([ex["node_flags"][s, :n[k]] for k, s in enumerate(idx)] + [np.zeros(0, np.uint8)])
    return search_step_full_batch(off, flat, ex["flags"][idx].astype(np.uint8), md)


def assert_same(got, twin, tag):
    for k in F.FIELDS:
        assert np.array_equal(np.asarray(got[k]).astype(np.uint64), np.asarray(twin[k]).astype(np.uint64)), (tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize("S,cap,full", CASES)
def test_step_full_equals_the_model(gpu, S, cap, full):
    searches = F.full_set(S, cap, 11 * S + cap, full)
    rng = np.random.default_rng(S + cap)
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as DS:
        first = DS.export()
        md = F.draw_modes(rng, S, 0.0)
        want = F.device_step_full(searches, None, md)
        twin = host_twin(DS, None, md)
        got = DS.step_full(None, md)
        F.assert_step_full(got, want[1:], "all")
        assert_same(got, twin, "all")
        st = got["stats"]
        for name, field in (("picks", 1), ("listens", 2), ("announces", 3)):
            assert st[name] == sum(bin(int(v)).count("1") for v in want[field]), name
        assert st["synced"] == int(((want[8] & T.SYNCED) != 0).sum()) and st["kernel_ms"] >= 0.0
        assert st["expired"] == int(((want[8] & T.EXPIRE) != 0).sum())
        assert st["skipped"] == int(((want[8] & T.SKIPPED) != 0).sum())
        if S >= 63:
            assert st["listens"] and st["announces"] and st["picks"]
        assert_same(DS.step_full(np.arange(S, dtype=np.uint32), md), got, "which = range(S)")
        F.assert_step_full(DS.step_full(), F.device_step_full(searches, None, 0)[1:], "mode NULL")
        back = DS.export()
        for k in first:
            assert np.array_equal(back[k], first[k]), k
        if S == 0:
            return
        # a scattered which with every valid mode in one call
        m = max(1, S // 3)
        which = np.sort(rng.choice(S, size=m, replace=False)).astype(np.uint32)
        md = F.draw_modes(rng, m, 0.6)
        if m >= len(F.MODES):
            md[rng.choice(m, size=len(F.MODES), replace=False)] = F.MODES
        after = F.device_step_full(searches, which, md)
        twin = host_twin(DS, which, md)
        got = DS.step_full(which, md)
        F.assert_step_full(got, after[1:], "scattered")
        assert_same(got, twin, "scattered")
        assert_export(DS, after[0], "scattered")
        # APPLY over the whole set, twice: nothing is sent twice
        md = F.draw_modes(rng, S, 1.0)
        once = F.device_step_full(after[0], None, md)
        twin = host_twin(DS, None, md)
        got = DS.step_full(None, md)
        F.assert_step_full(got, once[1:], "apply")
        assert_same(got, twin, "apply")
        assert_export(DS, once[0], "apply")
        twice = F.device_step_full(once[0], None, md)
        got = DS.step_full(None, md)
        F.assert_step_full(got, twice[1:], "apply again")
        assert_export(DS, twice[0], "apply again")
        for k, name in ((1, "picks"), (2, "listen"), (3, "announce")):
            assert not (got[name] & once[k]).any(), name
        # the expired searches are fresh empty expired searches, as a twin set created from the model has them
        gone = [s for s in range(S) if twice[0][s].expired and not searches[s].expired]
        if S >= 63:
            assert gone
        ex = DS.export()
        for s in gone:
            assert ex["flags"][s] == 1 and ex["n"][s] == 0 and ex["t"][s] == 0 and ex["full"][s] == 0
            assert not ex["node_ids"][s].any() and not ex["node_flags"][s].any()
        with DeviceSearches(*I.snapshot(twice[0]), cap=cap, device=0) as fresh:
            fx = fresh.export()
            for k in fx:
                assert np.array_equal(ex[k], fx[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("S,cap", [(257, 14), (257, 32), (65, 64)])
def test_old_modes_equal_kad_sr_step_on_a_twin(gpu, S, cap):
    searches = F.full_set(S, cap, 11 * S + cap)
    rng = np.random.default_rng(5 * S + cap)
    md = rng.choice(F.OLD_MODES, size=S).astype(np.uint8)
    md[rng.random(S) < 0.6] |= F.APPLY
    with DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as A, \
            DeviceSearches(*I.snapshot(searches), cap=cap, device=0) as B:
        for _ in range(2):
            a, b = A.step_full(None, md), B.step(None, md)
            for k in OLD:
                assert np.array_equal(a[k], b[k]), k
            assert not a["listen"].any() and not a["announce"].any()
            ea, eb = A.export(), B.export()
            for k in ea:
                assert np.array_equal(ea[k], eb[k]), k
        assert (ea["node_flags"] & F.DUE_BITS).any()  # the due bits were there and stayed


@pytest.mark.gpu
def test_named_cases_on_the_device(gpu):
    """Every named case as one search of a set with slabs of 64 entries, under its own mode plus APPLY."""
    names = list(F.NAMED)
    rng = np.random.default_rng(3)
    searches = F.make_full_set(rng, len(names), 64, [(F.NAMED[k][0], F.NAMED[k][1]) for k in names])
    md = np.array([F.NAMED[k][2] | F.APPLY for k in names], np.uint8)
    want = F.device_step_full(searches, None, md)
    with DeviceSearches(*I.snapshot(searches), cap=64, device=0) as DS:
        got = DS.step_full(None, md)
        F.assert_step_full(got, want[1:], "named")
        assert_export(DS, want[0], "named")
    for k, name in enumerate(names):
        by_hand = F.step_full(*F.NAMED[name])
        assert [F.positions(got[f][k]) for f in ("picks", "listen", "announce")] == list(by_hand[:3]), name
        assert int(got["bits"][k]) == by_hand[7] and int(got["solicited"][k]) == by_hand[6], name
    k = names.index("announce_in_every_unit_of_64")
    assert all((int(got["announce"][k]) >> (16 * u)) & 0xFFFF for u in range(4))
    k = names.index("listen_in_every_unit_of_64")
    assert all((int(got["listen"][k]) >> (16 * u)) & 0xFFFF for u in range(4))


@pytest.mark.gpu
def test_step_full_checks_that_need_a_set(gpu):
    searches = F.full_set(5, 32, 1)
    L = _lib.lib()
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        before = DS.export()
        for which, modes, what in ((None, np.array([0, 0, 0x80, 0, 0], np.uint8), b"invalid mode"),
                                   (None, np.array([0, F.DONE_IF_SYNCED | F.LISTEN, 0, 0, 0], np.uint8), b"invalid mode"),
                                   (None, np.array([0, 0, 0, 0, F.PROBE_BLOCKS | F.APPLY], np.uint8), b"invalid mode"),
                                   ([0, 2, 2], None, b"ascending"), ([1, 5], None, b"ascending"),
                                   ([3, 1], [F.APPLY | F.LISTEN, F.APPLY], b"ascending")):
            with pytest.raises(KadError):
                DS.step_full(which, modes)
            assert what in L.kad_last_error()
        # the old call still refuses the new modes
        with pytest.raises(KadError):
            DS.step(None, F.LISTEN)
        out = np.zeros(3, _lib.STEP_FULL_OUT_DTYPE)
        assert L.kad_sr_step_full(DS._h, 3, None, None, _lib.ptr(out), None) == _lib.KAD_ERR_INVALID  # m != S
        after = DS.export()
        for k in before:
            assert np.array_equal(after[k], before[k]), k
        assert DS.step_full([], None)["picks"].shape == (0,)
    with DeviceSearches(*I.snapshot(searches), cap=65, device=0) as DS:
        with pytest.raises(KadError) as e:
            DS.step_full(None, F.APPLY | F.LISTEN)
        assert e.value.code == _lib.KAD_ERR_UNSUPPORTED
        ids = np.zeros((1, 20), np.uint8)
        ids[0, 19] = 1
        with pytest.raises(KadError) as e:
            DS.mark_due([0], ids, None, [F.LDUE])
        assert e.value.code == _lib.KAD_ERR_UNSUPPORTED
        assert_export(DS, searches, "cap 65")
