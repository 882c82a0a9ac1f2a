"""opendht_amd.step_searches_full: one device step with all three send loops for the listed searches,
checked search by search against the host's own entry-by-entry searchStep and replayed on the host (listen, announce_probe,
send, expire()). On the CPU the device set is the model (stepfull_ref.ModelStepFull); on the GPU it is the real one, and
its export afterwards equals the host's lists without anything having been uploaded. A host whose lists differ from the
device's raises before anything is replayed."""
import numpy as np
import pytest

import insert_ref as I
import step_ref as T
import stepfull_ref as F
from opendht_amd import step_searches_full


def drive(DS, searches):
    host = F.HostStepFull(searches)
    S = len(searches)
    rng = np.random.default_rng(9)
    which = np.sort(rng.choice(S, size=S // 2, replace=False)).astype(np.uint32)
    md = F.draw_modes(rng, which.shape[0], 0.7)
    want = F.device_step_full(searches, which, md)
    r = step_searches_full(DS, host, which, md, T.NOW)
    for bit, name in ((T.SYNCED, "synced"), (T.SHORT, "short"), (T.DONE, "done"), (T.EXHAUSTED, "exhausted"),
                      (T.EXPIRE, "expire"), (T.SKIPPED, "skipped")):
        assert r[name] == [int(s) for s, b in zip(which, want[8]) if b & bit], name
        assert r[name], name  # the set holds every kind
    for k, name in ((1, "picks"), (2, "listen"), (3, "announce")):
        assert r[name] == {int(s): F.positions(p) for s, p in zip(which, want[k]) if p}, name
        assert r[name], name
    assert [s.key() for s in host.searches] == [s.key() for s in want[0]]
    md = F.draw_modes(rng, S, 1.0)  # every search
    r = step_searches_full(DS, host, None, md, T.NOW)
    again = F.device_step_full(want[0], None, md)
    assert [s.key() for s in host.searches] == [s.key() for s in again[0]]
    for name, stat in (("picks", "picks"), ("listen", "listens"), ("announce", "announces")):
        assert sum(len(v) for v in r[name].values()) == r["stats"][stat], name
    return host


def test_step_searches_full_over_the_model():
    searches = F.full_set(160, 32, 78)
    DS = F.ModelStepFull(searches, 32)
    host = drive(DS, searches)
    assert [s.key() for s in DS.s] == [s.key() for s in host.searches]
    # a host list that differs from the device's in a due bit only: the comparison raises and nothing is replayed
    k = next(i for i, s in enumerate(host.searches) if F.step_full([e[1] for e in s.ents], s.expired, F.LISTEN)[7] & T.SYNCED
             and not s.ents[0][1] & (T.BAD | F.LDUE) and s.ents[0][1] & T.SYNC)
    s = host.searches[k]
    host.searches[k] = I.FlagSearch(s.id, False, [(s.ents[0][0], s.ents[0][1] | F.LDUE)] + s.ents[1:])
    before = [x.key() for x in host.searches]
    with pytest.raises(RuntimeError, match=f"search {k} "):
        step_searches_full(F.ModelStepFull(DS.s, 32), host, None, F.APPLY | F.LISTEN, T.NOW)
    assert [x.key() for x in host.searches] == before


@pytest.mark.gpu
def test_step_searches_full_on_the_device(gpu):
    from opendht_amd import DeviceSearches

    searches = F.full_set(160, 32, 78)
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        host = drive(DS, searches)
        got, want = DS.export(), I.expected_export(host.searches, 32)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
