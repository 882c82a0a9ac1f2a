"""kad_sr_refill against Dht::refill restated in refill_ref.py: getCachedNodes over the cache, then
Search::insertNode on every result in walk order. Per case the rows, counts, insert masks and statuses equal the
restatement elementwise, the export afterwards is the one of a set created from the restated searches (overflowed and
unlisted searches byte-identical to before), later trySearchInsert verdicts equal those of a fresh set, and a second
refill inserts nothing. The shapes are the smallest at which each mechanism can break: caches of 0, 1, 13, 40 and 3000
nodes (rows shorter than 14, one radix slot, many), sets of 0 to 300 searches, slabs of 14, 32 and 64 entries (64: a
list of 64 entries holds its 65th outside the lanes), 63, 64 and 65 listed searches (the last wave of a block).
The expected outputs are computed once per case and shared."""
import numpy as np
import pytest

import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable

NOW = F.NOW


def test_get_cached_nodes_equals_the_oracle():
    """The restated walk of node_cache.cpp:36-66 against the oracle's flat_nc_closest on the same IDs."""
    import oracle as O

    for name in ("n1_s3", "n13_s65_cap14", "n40_s65_cap14", "n3000_s300_cap32"):
        c = F.case(name)
        cache = c["cache"]
        ids, status = cache.table_arrays()
        rng = np.random.default_rng(3)
        targets = [s.id for s in c["searches"]] + cache.ids[:40] + [0, R.MAX_ID]
        targets += [cache.ids[int(rng.integers(0, len(cache.ids)))] ^ (1 << int(rng.integers(0, 160))) for _ in range(64)]
        want, wcnt = O.flat_nc_closest(ids, status, R.id_bytes(targets), F.SEARCH_NODES)
        for i, t in enumerate(targets):
            row = cache.get_cached_nodes(t)
            assert len(row) == wcnt[i] and row == [int(v) for v in want[i, :wcnt[i]]], (name, i)


def test_expected_outputs_cover_the_mechanisms():
    """Passes on the restatement alone: every mechanism of the refill occurs in the cases."""
    tot = F.new_stats()
    over = short = m0 = mfull = mpart = 0
    for name in F.CASES:
        c = F.case(name)
        for k, v in c["stats"].items():
            tot[k] += v
        over += int(c["status"].sum())
        ok = c["status"] == F.REFILL_OK
        full = (1 << c["cnt"].astype(np.uint32)) - 1
        short += int(((c["cnt"] > 0) & (c["cnt"] < F.SEARCH_NODES)).sum())
        m0 += int((ok & (c["cnt"] > 0) & (c["ins"] == 0)).sum())
        mfull += int((ok & (c["cnt"] > 0) & (c["ins"] == full)).sum())
        mpart += int((ok & (c["ins"] != 0) & (c["ins"] != full)).sum())
    for k, v in tot.items():
        assert v >= 5, (k, v)
    assert min(over, short, m0, mfull, mpart) >= 5, (over, short, m0, mfull, mpart)
    assert sorted(len(F.case(n)["which"]) for n in ("m63", "m64", "n3000_s65_cap64")) == [63, 64, 65]
    c = F.case("n3000_s65_cap64")  # lists of 64 entries that take an insert: the 65th entry outside the lanes
    assert sum(1 for s, a in zip(c["searches"], c["after"]) if len(s.nodes) == 64 and a is not s) >= 2
    assert int(c["status"].sum()) >= 1


def cache_table(c):
    ids, status = c["cache"].table_arrays()
    return DeviceTable(ids, status, device=0, index_base=c["base"], sorted=True)


def assert_export(DS, searches, tag):
    got, want = DS.export(), F.expected_export(searches, DS.cap, NOW)
    for k in want:
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(F.CASES))
def test_refill_equals_the_restatement(gpu, name):
    c = F.case(name)
    searches, after, which, cap = c["searches"], c["after"], c["which"], c["cap"]
    with cache_table(c) as NC, DeviceSearches(*F.snapshot(searches, NOW), cap=cap, device=0) as DS:
        assert_export(DS, searches, "before")
        rows, cnt, ins, status = DS.refill(NC, which)
        # the rows are the ones of the NodeCache query, and of the restatement
        sids = R.id_bytes([searches[int(s)].id for s in which]) if len(which) else np.zeros((0, 20), np.uint8)
        qrows, qcnt = NC.nc_closest_host(sids, F.SEARCH_NODES)
        assert np.array_equal(rows, qrows) and np.array_equal(cnt, qcnt)
        assert np.array_equal(rows, c["rows"]) and np.array_equal(cnt, c["cnt"])
        bad = np.flatnonzero((ins != c["ins"]) | (status != c["status"]))
        assert bad.size == 0, (bad[:5], ins[bad[:5]], c["ins"][bad[:5]], status[bad[:5]], c["status"][bad[:5]])
        assert_export(DS, after, "after")
        for k in np.flatnonzero(status == F.REFILL_OVERFLOW):
            assert after[int(which[k])] is searches[int(which[k])] and ins[k] == 0
        if len(searches):
            cands = R.make_cands(np.random.default_rng(5), after, 257)
            with DeviceSearches(*F.snapshot(after, NOW), cap=cap, device=0) as fresh:
                got, want = DS.try_insert_host(R.id_bytes(cands)), fresh.try_insert_host(R.id_bytes(cands))
            for g, w, r in zip(got, want, R.verdicts(after, cands, NOW)):
                assert np.array_equal(g, w) and np.array_equal(g, r)
        # the same searches again: the rows are unchanged, every node of an applied row is now a member or was
        # refused on its merits, so nothing is inserted
        rows2, cnt2, ins2, status2 = DS.refill(NC, which)
        assert np.array_equal(rows2, rows) and np.array_equal(cnt2, cnt) and np.array_equal(status2, status)
        again = F.device_refill(after, c["cache"], [int(s) for s in which], NOW, cap, c["base"])
        assert np.array_equal(ins2, again[3])
        assert_export(DS, again[0], "second")
        assert (ins2[status == F.REFILL_OK] == 0).all()


@pytest.mark.gpu
def test_refill_after_patch_and_unlisted_searches(gpu):
    """Refill of one part of a set, then of the rest: the unlisted searches stay as they were in between, and the two
    calls together equal one call over all searches."""
    c = F.case("n3000_s300_cap32")
    searches, cap = c["searches"], c["cap"]
    S = len(searches)
    a, b = np.arange(0, S, 2, dtype=np.uint32), np.arange(1, S, 2, dtype=np.uint32)
    with cache_table(c) as NC, DeviceSearches(*F.snapshot(searches, NOW), cap=cap, device=0) as DS:
        DS.refill(NC, a)
        mid = F.device_refill(searches, c["cache"], [int(s) for s in a], NOW, cap, c["base"])[0]
        assert_export(DS, mid, "half")
        DS.refill(NC, b)
        assert_export(DS, c["after"], "both")
