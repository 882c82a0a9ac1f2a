"""kad_searches_apply restated for the tests: delete from the Python list of searches_ref.Search
objects, add Search(id, expired) with no nodes, sort by ID. After every apply the device set must be
indistinguishable from a set freshly created from that model at the final cap: `compare` checks the export, the
device bytes and the trySearchInsert verdicts. Shared by test_searches_apply*.py; the models are built once and never
changed (an apply makes a new list, a refill works on copies)."""
import functools

import numpy as np

import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable

NOW = F.NOW
NO_NODE = 0xFFFFFFFF
STRAY = 0x80  # a flag bit the library does not know: carried through create, apply and export


def snap(model, stray=False):
    """The CSR arrays of kad_searches_create for the model, KAD_SN_REMOVABLE evaluated at NOW; with stray, entries
    whose node ID ends in a multiple of 5 carry STRAY as well."""
    ids, flags, off, nid, nfl = F.snapshot(model, NOW)
    if stray and nfl.size:
        nfl = nfl | np.where(nid[:, 19] % 5 == 0, STRAY, 0).astype(np.uint8)
    return ids, flags, off, nid, nfl


def model_apply(model, erase=(), ins=(), expired=None):
    """(the model afterwards, remap, new_index): ins are integer IDs, expired one bool per inserted search."""
    gone = set(int(e) for e in erase)
    new = [R.Search(int(v), bool(expired[j]) if expired is not None else False) for j, v in enumerate(ins)]
    out = sorted([s for i, s in enumerate(model) if i not in gone] + new, key=lambda s: s.id)
    at = {id(s): i for i, s in enumerate(out)}
    remap = np.array([NO_NODE if i in gone else at[id(s)] for i, s in enumerate(model)], np.uint32).reshape(-1)
    return out, remap, np.array([at[id(s)] for s in new], np.uint32).reshape(-1)


def apply(DS, model, erase=(), ins=(), expired=None, cap=None):
    """DeviceSearches.apply against the model: remap and new_index must be the model's. Returns the new model."""
    out, remap, new_index = model_apply(model, erase, ins, expired)
    got = DS.apply(np.array(erase, np.uint32), R.id_bytes(ins) if len(ins) else (),
                   None if expired is None else np.array(expired, np.uint8), cap)
    assert np.array_equal(got[0], remap) and np.array_equal(got[1], new_index)
    assert DS.S == len(out) and (cap is None or DS.cap == cap)
    assert np.array_equal(DS._ids, snap(out)[0])
    return out


def last_byte(v, by):
    return (v & ~0xFF) | ((v + by) & 0xFF)


def candidates(model, q=96, seed=5):
    """make_cands plus every search ID, every search ID +- 1 in the last byte, 00..0 and FF..F."""
    ids = [s.id for s in model]
    return (R.make_cands(np.random.default_rng(seed), model, q) + ids + [last_byte(v, 1) for v in ids] +
            [last_byte(v, -1) for v in ids] + [0, R.MAX_ID])


def compare(DS, model, cap, stray=False, tag=""):
    """DS against a set freshly created from the model at `cap`: all seven export arrays, the device bytes, and the
    verdicts of `candidates` from both sets and from searches_ref.verdicts."""
    assert DS.S == len(model) and DS.cap == cap, tag
    cands = candidates(model)
    cb = R.id_bytes(cands)
    with DeviceSearches(*snap(model, stray), cap=cap, device=0) as fresh:
        got, want = DS.export(), fresh.export()
        assert sorted(got) == sorted(want) and len(want) == 7
        for k in want:
            assert got[k].shape == want[k].shape, (tag, k)
            bad = np.argwhere(got[k] != want[k])
            assert bad.size == 0, (tag, k, bad[:4])
        assert DS.device_bytes == fresh.device_bytes, tag
        v_got, v_want = DS.try_insert_host(cb), fresh.try_insert_host(cb)
    for name, g, w, r in zip(("lb", "fwd", "back", "stop"), v_got, v_want, R.verdicts(model, cands, NOW)):
        assert np.array_equal(g, w), (tag, name, np.flatnonzero(g != w)[:4])
        assert np.array_equal(g, r), (tag, name, np.flatnonzero(g != r)[:4])


def free_between(model, i, count):
    """count consecutive IDs strictly between two neighbouring searches, the first pair at or after search i that is
    far enough apart (make_ids puts some IDs beside each other)."""
    while model[i + 1].id - model[i].id <= count:
        i += 1
    return [model[i].id + 1 + k for k in range(count)]


@functools.lru_cache(maxsize=None)
def cache():
    """A NodeCache of 3000 nodes, shared."""
    return F.make_cache(np.random.default_rng(77), 3000)


def cache_table():
    ids, status = cache().table_arrays()
    return DeviceTable(ids, status, device=0, sorted=True)


def _make(seed, S, cap):
    m = F.make_set(np.random.default_rng(seed), S + 2, F.states_for(cap), cap, cache())
    return [s for s in m if s.id not in (0, R.MAX_ID)][:S]  # make_ids always takes 0 and FF..F: they stay free


@functools.lru_cache(maxsize=None)
def pool():
    """8400 searches for slabs of 14 entries. Their lists share at least 40 bits with the search ID, as the lists of
    a node with thousands of live searches do: a neighbouring search's ID (13 bits shared) is refused by a full
    search, so the restated walks stay short. Five in six are full or expired, the others empty or not full."""
    rng = np.random.default_rng(1014)
    out = []
    for sid in R.make_ids(rng, 8402):
        if sid in (0, R.MAX_ID):
            continue
        kind = int(rng.integers(0, 12))
        n = 14 if kind < 10 else (0 if kind == 10 else int(rng.integers(1, 14)))
        ids, shift = set(), int(rng.integers(40, 121))
        while len(ids) < n:
            ids.add(sid ^ (int.from_bytes(rng.bytes(20), "big") >> shift))
        ids.discard(sid)
        expired = kind in (7, 8, 9)  # all of its nodes bad, some of them old enough to be removable
        nodes = [R.SearchNode(R.Node(v, expired=expired, time=F.TIMES[int(rng.integers(0, 4))]))
                 for v in sorted(ids, key=lambda v: v ^ sid)]
        out.append(R.Search(sid, expired, nodes))
    return tuple(out[:8400])


@functools.lru_cache(maxsize=None)
def base(S, cap):
    """S searches in ID order, 0 and FF..F not among their IDs: up to 100 searches a set of its own in every state
    the cap allows, beyond that a spread over the pool (lists of up to 14 entries, good for every cap)."""
    if S <= 100:
        return _make(2000 + 131 * S + cap, S, cap) if S else []
    p = pool()
    return [p[int(i)] for i in np.linspace(0, len(p) - 1, S).astype(np.int64)]


def refill_and_compare(DS, NC, model, which, cap, tag=""):
    """kad_sr_refill of `which` against refill_ref.device_refill on the model: rows, counts, masks, statuses and,
    through compare, the export. Returns the model afterwards and the statuses."""
    which = np.array(sorted(int(w) for w in which), np.uint32)
    after, rows, cnt, ins, status = F.device_refill(model, cache(), [int(w) for w in which], NOW, cap)
    g_rows, g_cnt, g_ins, g_status = DS.refill(NC, which)
    assert np.array_equal(g_rows, rows) and np.array_equal(g_cnt, cnt), tag
    assert np.array_equal(g_ins, ins) and np.array_equal(g_status, status), tag
    compare(DS, after, cap, tag=tag + " refilled")
    return after, status


class Host(F.HostRefill):
    """The `host` of start_searches / expire_searches over a model: the list stays in ID order."""

    def __init__(self, model):
        super().__init__([s.copy() for s in model], cache(), NOW)

    def add(self, ids):
        self.searches = model_apply(self.searches, ins=[int.from_bytes(bytes(r), "big") for r in np.asarray(ids)])[0]

    def erase(self, erase):
        self.searches = model_apply(self.searches, erase=erase)[0]
