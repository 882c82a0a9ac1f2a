"""A walk over every mutation of a device search set around kad_searches_apply: apply, refill,
patch, apply again (erasing searches that were just refilled, inserting others, growing the slabs), the
trySearchInsert tick of opendht_amd.try_search_insert, and an apply back to the first membership. After every step the
set must equal one freshly created from the model (apply_ref.compare: export, device bytes, verdicts). 300 searches in
every state over a cache of 3000 nodes, once with slabs that take the 16-byte path (32 -> 64) and once with the narrow
one (15 -> 33)."""
import numpy as np
import pytest

import apply_ref as A
import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, try_search_insert

NOW = A.NOW


class TickHost(R.HostSearches):
    """The host of try_search_insert with the flag bytes of this file's snapshots (KAD_SN_REMOVABLE at NOW)."""

    def state(self, s):
        return F.search_state(self.searches[s], NOW)


@pytest.mark.gpu
@pytest.mark.parametrize("cap,cap2", [(32, 64), (15, 33)])
def test_walk(gpu, cap, cap2):
    rng = np.random.default_rng(cap)
    c = A.cache()
    m0 = A._make(4000 + cap, 300, cap)
    ids0 = [s.id for s in m0]
    with A.cache_table() as NC, DeviceSearches(*A.snap(m0), cap=cap, device=0) as DS:
        A.compare(DS, m0, cap, tag="created")
        # 1. searches expire, others start
        erase = sorted(int(i) for i in rng.choice(300, 20, replace=False))
        ins = [c.ids[k] ^ (1 << (k % 90)) for k in range(3, 3000, 125)] + [0, R.MAX_ID]
        m = A.apply(DS, m0, erase, ins)
        A.compare(DS, m, cap, tag="apply 1")
        new = [i for i, s in enumerate(m) if s.id in set(ins)]
        # 2. the new searches and some old ones are refilled
        which = sorted(set(new) | set(int(i) for i in rng.choice(len(m), 40, replace=False)))
        m, _ = A.refill_and_compare(DS, NC, m, which, cap, tag="refill")
        # 3. the host changed some lists: half of their nodes gone, the expired flag flipped
        which = sorted(int(i) for i in rng.choice(len(m), 15, replace=False))
        m = list(m)
        for i in which:
            m[i] = R.Search(m[i].id, not m[i].expired, m[i].nodes[:len(m[i].nodes) // 2])
        DS.patch(np.array(which, np.uint32), *A.snap([m[i] for i in which])[1:])
        A.compare(DS, m, cap, tag="patch")
        # 4. half of the searches refilled in step 2 expire, others start, and the slabs grow
        ins2 = [c.ids[k] ^ (1 << (k % 70)) for k in range(50, 3000, 300)]
        m = A.apply(DS, m, new[::2], ins2, expired=[k % 2 for k in range(len(ins2))], cap=cap2)
        A.compare(DS, m, cap2, tag="apply 2")
        # 5. a tick of trySearchInsert: the host inserts where the verdicts say and patches the set
        cands = R.make_cands(np.random.default_rng(6), m, 200)
        nodes = {v: R.Node(v) for v in cands}
        host = TickHost([s.copy() for s in m], [nodes[v] for v in cands], NOW)
        counts = try_search_insert(DS, host, R.id_bytes(cands))
        assert counts["inserts"] > 0
        m = host.searches
        A.compare(DS, m, DS.cap, tag="tick")
        # 6. back to the first membership: the searches that left come back empty
        have = set(s.id for s in m)
        m = A.apply(DS, m, [i for i, s in enumerate(m) if s.id not in set(ids0)], [v for v in ids0 if v not in have])
        assert [s.id for s in m] == ids0
        A.compare(DS, m, DS.cap, tag="back")
