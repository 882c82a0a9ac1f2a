"""opendht_amd.refill_searches against the restatement run sequentially: after one device refill and
the host's replay of the rows, the host's searches are the ones Dht::refill leaves search by search, and the device
set exports exactly them, the searches the device handed back as overflowed included (patched when their final list
fits the slab, a new set with larger slabs when it does not)."""
import numpy as np
import pytest

import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable, refill_searches

NOW = F.NOW


def sequential(c):
    """Dht::refill on copies of the listed searches, one after the other: (searches afterwards, masks)."""
    out, masks = list(c["searches"]), []
    for s in c["which"]:
        out[int(s)] = c["searches"][int(s)].copy()
        masks.append(F.refill(out[int(s)], c["cache"], NOW)[1])
    return out, masks


def same_searches(a, b):
    return all(x.expired == y.expired and [n.node.id for n in x.nodes] == [n.node.id for n in y.nodes]
               and [n.is_bad() for n in x.nodes] == [n.is_bad() for n in y.nodes] for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n0_s3", "n13_s65_cap14", "n3000_s300_cap32", "n3000_s300_cap64", "n40_s0"])
def test_refill_searches_equals_sequential_refill(gpu, name):
    c = F.case(name)
    want, masks = sequential(c)
    mine = [s.copy() for s in c["searches"]]
    host = F.HostRefill(mine, c["cache"], NOW, c["base"])
    ids, status = c["cache"].table_arrays()
    with DeviceTable(ids, status, device=0, index_base=c["base"], sorted=True) as NC, \
            DeviceSearches(*F.snapshot(c["searches"], NOW), cap=c["cap"], device=0) as DS:
        counts = refill_searches(DS, NC, host, c["which"], NOW)
        assert same_searches(mine, want)
        over = int(c["status"].sum())
        assert counts == {"refilled": int(((c["status"] == 0) & (c["cnt"] > 0)).sum()), "overflowed": over,
                          "inserts": sum(bin(m).count("1") for m in masks), "untouched": int((c["cnt"] == 0).sum())}
        longest = max([len(s.nodes) for s in want] + [0])
        assert DS.cap == (c["cap"] if longest <= c["cap"] else max(longest, 2 * c["cap"]))
        got, exp = DS.export(), F.expected_export(want, DS.cap, NOW)
        for k in exp:
            assert np.array_equal(got[k], exp[k]), k
        if len(want):
            cands = R.make_cands(np.random.default_rng(9), want, 129)
            for g, r in zip(DS.try_insert_host(R.id_bytes(cands)), R.verdicts(want, cands, NOW)):
                assert np.array_equal(g, r)


def test_cases_cover_both_overflow_paths():
    """Without a GPU: among the ingest cases one hands overflowed searches back whose final lists all fit (a patch)
    and one ends with a list longer than its slab (a new set)."""
    kinds = set()
    for name in ("n13_s65_cap14", "n3000_s300_cap32", "n3000_s300_cap64"):
        c = F.case(name)
        if c["status"].sum():
            want, _ = sequential(c)
            kinds.add(max(len(want[int(s)].nodes) for s in c["which"][c["status"] == 1]) > c["cap"])
    assert kinds == {True, False}
