"""opendht_amd.step_searches: one device step for the listed searches, checked search by search against
the host's own entry-by-entry searchStep and replayed on the host (sends, expire()). On the CPU the device set is the
model (step_ref.ModelStep); on the GPU it is the real one, and its export afterwards equals the host's lists without
anything having been uploaded. A host whose lists differ from the device's raises before anything is replayed."""
import numpy as np
import pytest

import insert_ref as I
import step_ref as T
from opendht_amd import step_searches


def drive(DS, searches):
    host = T.HostStep(searches)
    S = len(searches)
    rng = np.random.default_rng(9)
    which = np.sort(rng.choice(S, size=S // 2, replace=False)).astype(np.uint32)
    md = rng.choice([T.APPLY, T.APPLY | T.DONE_IF_SYNCED, T.APPLY | T.NO_EXPIRE, 0, T.NO_SEND], size=which.shape[0]).astype(np.uint8)
    want = T.device_step(searches, which, md)
    r = step_searches(DS, host, which, md, T.NOW)
    for bit, name in ((T.SYNCED, "synced"), (T.SHORT, "short"), (T.DONE, "done"), (T.EXHAUSTED, "exhausted"),
                      (T.EXPIRE, "expire"), (T.SKIPPED, "skipped")):
        assert r[name] == [int(s) for s, b in zip(which, want[6]) if b & bit], name
        assert r[name], name  # the set holds every kind
    assert r["picks"] == {int(s): [e for e in range(64) if (int(p) >> e) & 1] for s, p in zip(which, want[1]) if p}
    assert [s.key() for s in host.searches] == [s.key() for s in want[0]]
    r = step_searches(DS, host, None, T.APPLY, T.NOW)  # every search, one mode for all
    again = T.device_step(want[0], None, T.APPLY)
    assert [s.key() for s in host.searches] == [s.key() for s in again[0]]
    assert sum(len(v) for v in r["picks"].values()) == r["stats"]["picks"]
    return host


def test_step_searches_over_the_model():
    searches = T.step_set(120, 32, 77)
    DS = T.ModelStep(searches, 32)
    host = drive(DS, searches)
    assert [s.key() for s in DS.s] == [s.key() for s in host.searches]
    # a host list that differs from the device's: the comparison raises and nothing is replayed
    k = next(i for i, s in enumerate(host.searches) if not s.expired and s.ents)
    s = host.searches[k]
    host.searches[k] = I.FlagSearch(s.id, False, [(s.ents[0][0], s.ents[0][1] ^ T.BAD)] + s.ents[1:])  # another bad count
    before = [x.key() for x in host.searches]
    with pytest.raises(RuntimeError, match=f"search {k} "):
        step_searches(T.ModelStep(DS.s, 32), host, None, T.APPLY, T.NOW)
    assert [x.key() for x in host.searches] == before


@pytest.mark.gpu
def test_step_searches_on_the_device(gpu):
    from opendht_amd import DeviceSearches

    searches = T.step_set(120, 32, 77)
    with DeviceSearches(*I.snapshot(searches), cap=32, device=0) as DS:
        host = drive(DS, searches)
        got, want = DS.export(), I.expected_export(host.searches, 32)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
