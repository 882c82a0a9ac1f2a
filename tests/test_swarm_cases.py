"""Config 5 edge cases on the CPU: the oracle's capped lookups against its unbounded ones, its
tables and per-peer findClosestNodes on the case swarms (swarm_cases.py) against the RoutingTable restatement and the
model's shape invariants with the depth cap, and the conditions under which tests/test_swarm_edges.py covers what it is
there for — asserted, so that a change of the inputs that loses a branch fails here."""
import numpy as np
import pytest

import oracle as O
import swarm_cases as SC
import swarm_ref as R
from opendht_amd import synth as S
from test_swarm import _as_routing_table, _check_lookup_properties_vec, _offline, _swarm_ids

SHAPED = ("clustered", "oneprefix", "lopsided") + SC.TINY_NAMES
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def test_case_builders_are_deterministic_and_sorted():
    for name in SC.NAMES:
        ids, src, tg = SC.case(name)
        assert ids.shape[0] <= 5000 and src.shape[0] <= 2000 and src.shape[0] == tg.shape[0]
        as_int = [int.from_bytes(x.tobytes(), "big") for x in ids]
        assert all(a < b for a, b in zip(as_int, as_int[1:]))  # strictly ascending
        assert int(src.max()) < ids.shape[0]
        SC.case.cache_clear()
        SC.swarm.cache_clear()
        again = SC.case(name)
        for a, b in zip((ids, src, tg), again):
            np.testing.assert_array_equal(a, b)
    assert np.array_equal(SC.offline(np.arange(5000), 3000), _offline(np.arange(5000), 3000))


@pytest.mark.parametrize("off", [0, 1000, 3000])
def test_capped_search_with_no_caps_equals_search_ex(off):
    """test_swarm_search_offline_peers_oracle's and test_swarm_lazy_model_equals_eager's inputs: the new entry with both
    capacities 0 is search_ex; with the device's capacities as well there (no list reaches them), without an event."""
    for seed, n, count, filt in ((0x5A6, 30_000, 400, True), (0x5AA, 30_000, 500, False)):
        ids = _swarm_ids(n, seed)
        M = O.SwarmModel(ids)
        src = np.random.default_rng(8 + off).integers(0, n, count).astype(np.uint32)
        if filt:
            src = src[~_offline(src, off)]
        tg = S.random_targets(src.shape[0], seed=9)
        for hops in (1, 3, 64):
            want = M.search_ex(src, tg, off, max_hops=hops)
            for caps in ((0, 0), (R.LIST_CAP, R.SILENT_CAP)):
                got = M.search_cap(src, tg, off, *caps, max_hops=hops)
                for a, b, f in zip(got, want, R.FIELDS):
                    np.testing.assert_array_equal(a, b, err_msg=f"{caps} hops {hops}: {f}")
                assert got[6].max() < R.LIST_CAP and got[7].max() < R.SILENT_CAP and not got[8].any()
                assert (got[6] >= got[3]).all()
        M.close()


def _plain_lookup(M, ids, s, t, off, list_cap, silent_cap):
    """One lookup of the model with the two capacities, in plain Python from DESIGN.md §7.2's words (160-bit integer
    distances, lists of [peer, queried, bad]); only the per-peer findClosestNodes comes from the oracle.
    Returns (list, hops, done, hops in which a capacity was hit)."""
    tint = int.from_bytes(t.tobytes(), "big")

    def dist(v):
        return int.from_bytes(ids[v].tobytes(), "big") ^ tint

    def closest(p, k):
        got = M.closest(np.array([p], np.uint32), t[None], k)[0][0]
        return [int(x) for x in got if x != O.NO_NODE]

    def select():
        sel = []
        for e in L:
            if len(sel) < 4 and not e[1] and not e[2]:
                e[1] = True
                sel.append(e[0])
        return sel

    L = [[v, False, False] for v in closest(s, 14)]
    silent, hops, done, cap_hops = [], 0, 0, 0
    sel = select()
    done = 0 if sel else 2
    while not done:
        hops += 1
        hit = False
        for v in sel:
            if SC.offline(v, off):
                continue
            for r in closest(v, 8):
                if r == s or any(e[0] == r for e in L):
                    continue
                pos = sum(1 for e in L if dist(e[0]) < dist(r))
                if sum(1 for e in L if not e[2]) >= 14:  # full: cut after the last prefix with 14 non-bad nodes
                    seen, cut = 0, len(L)
                    for i, e in enumerate(L):
                        seen += not e[2]
                        if seen == 15:
                            cut = i
                            break
                    del L[cut:]
                    if pos >= cut:
                        continue
                if list_cap and len(L) == list_cap:  # the list keeps the list_cap closest of its entries and r
                    hit = True
                    if pos == len(L):
                        continue
                    L.pop()
                L.insert(pos, [r, False, r in silent])
                while sum(1 for e in L if not e[2]) > 14:
                    L.pop()
        for v in sel:
            if SC.offline(v, off):
                if not silent_cap or len(silent) < silent_cap:
                    silent.append(v)
                else:
                    hit = True
                for e in L:
                    e[2] = e[2] or e[0] == v
        cap_hops += hit
        good = [e for e in L if not e[2]][:8]
        lead = next((i for i, e in enumerate(L) if not e[2]), len(L))
        if good and all(e[1] for e in good):
            done = 1
        elif L and lead >= min(len(L), 25):
            done = 3
        else:
            sel = select()
            done = 0 if sel else 2
    return L, hops, done, cap_hops


@pytest.mark.parametrize("caps", [(32, 64), (20, 6), (15, 1), (0, 0)])
def test_capped_search_equals_the_rule_in_plain_python(caps):
    """The oracle's capped lookups against the rule restated in plain Python, on lookups that hit the capacities
    (and some that do not), at the device's capacities and at smaller ones that make both events common — the
    silent-peer rule, which no case reaches at 64, runs here at 6 and 1."""
    events = 0
    for name, off in (("clustered", 6000), ("random5k", 8000), ("tinyskew", 5000), ("lopsided", 9700)):
        ids, src, tg = SC.case(name)
        M = R.model(name)
        got = M.search_cap(src, tg, off, *caps)
        hit = np.flatnonzero(got[8] > 0)[:25]
        pick = np.unique(np.concatenate([hit, np.linspace(0, src.shape[0] - 1, 25).astype(np.int64)]))
        for i in pick:
            L, hops, done, cap_hops = _plain_lookup(M, ids, int(src[i]), tg[i], off, *caps)
            where = f"{name} at {off}, lookup {i}, caps {caps}"
            w = min(len(L), 32)  # (the oracle returns the first 32 entries of an unbounded list)
            assert [e[0] for e in L[:w]] == got[0][i, :w].tolist() and (got[0][i, w:] == O.NO_NODE).all(), where
            assert [int(e[1]) for e in L[:w]] == got[1][i, :w].tolist(), where
            assert [int(e[2]) for e in L[:w]] == got[2][i, :w].tolist(), where
            assert (len(L), hops, done, cap_hops) == (got[3][i], got[4][i], got[5][i], got[8][i]), where
            events += cap_hops
    assert (events > 0) == (caps != (0, 0))


@pytest.mark.parametrize("name", SC.NAMES)
def test_capped_search_keeps_the_model_invariants(name):
    """Every offline share of the edge tests: the capped lists stay within 32 entries, ascending, with <= 14 non-bad
    nodes, zero padding; where no capacity was hit the capped lookup is the unbounded one."""
    ids, src, tg = SC.case(name)
    for off in SC.offline_shares(name):
        lst, q, bad, n, hops, done, peak, silent, cap_hops = R.capped(name, off)
        u = R.unbounded(name, off)
        assert n.max() <= R.LIST_CAP and peak.max() <= R.LIST_CAP and silent.max() <= R.SILENT_CAP
        pad = np.arange(32)[None, :] >= n.astype(np.int64)[:, None]
        assert (lst[pad] == O.NO_NODE).all() and not q[pad].any() and not bad[pad].any()
        _check_lookup_properties_vec(ids, lst, q, bad, n, done, off, tg)
        same = cap_hops == 0
        assert (u[6][same] <= R.LIST_CAP).all() and (u[6][~same] >= R.LIST_CAP).all()
        for a, b, f in zip((lst, q, bad, n, hops, done), u, R.FIELDS):
            np.testing.assert_array_equal(a[same], b[same], err_msg=f"{name} {off}: {f}")
        assert set(np.unique(done)) <= {1, 2, 3}


@pytest.mark.parametrize("name", SHAPED)
def test_case_closest_matches_routing_table_restatement(name):
    """The swarm model's per-peer findClosestNodes equals the general restatement on the peer's table written out as
    a RoutingTable, at the depth cap, on one-sided tables and on tables of one or two buckets."""
    ids, src, tg = SC.case(name)
    M = R.model(name)
    pick = np.unique(np.linspace(0, src.shape[0] - 1, 140).astype(np.int64))
    peers, targets = np.ascontiguousarray(src[pick]), np.ascontiguousarray(tg[pick])
    tables = {}
    for count in (1, 8, 14, 16):
        got, gc = M.closest(peers, targets, count)
        for i, p in enumerate(peers):
            p = int(p)
            if p not in tables:
                depth, cnt, ent = M.table(p)
                tables[p] = _as_routing_table(ids, p, depth, cnt, ent)
            firsts, off, members = tables[p]
            sub = ids[members] if members.size else np.zeros((0, 20), np.uint8)
            st = np.ones(members.shape[0], np.uint8)
            w, wc = O.flat_rt_closest(sub, st, firsts, off, targets[i:i + 1], count)
            want = np.where(w[0] != O.NO_NODE, members[np.minimum(w[0], max(members.size - 1, 0))], O.NO_NODE)
            assert gc[i] == wc[0]
            np.testing.assert_array_equal(got[i], want)


@pytest.mark.parametrize("name", SHAPED)
def test_case_tables_shape_k_with_depth_cap(name):
    """Depth is the least D with <= 8 other peers sharing >= D leading bits, or 27; at 27 my bucket is the first 8
    other peers of the run in ID order; a level holds min(8, |S_d|) distinct peers sharing exactly d bits."""
    ids = SC.swarm(name)
    key = SC.key64(ids)
    n = ids.shape[0]
    M = R.model(name)
    peers = np.arange(n) if n <= 200 else np.unique(np.concatenate([
        np.random.default_rng(7).integers(0, n, 150), [0, 1, 7, 8, 9, n - 9, n - 1]]))
    capped_runs = 0
    for p in peers:
        p = int(p)
        depth, cnt, ent = M.table(p)
        share = np.array([64 - int(v).bit_length() for v in key ^ key[p]])  # leading bits shared with p (top 64)
        others = lambda D: int((share >= D).sum()) - 1  # noqa: E731
        want_depth = next(D for D in range(SC.LEVELS) if others(D) <= 8 or D == SC.CAP_DEPTH)
        assert depth == want_depth == SC.depth_of(key, p)
        for d in range(depth):
            members = ent[d, :cnt[d]]
            assert cnt[d] == min(8, int((share == d).sum()))
            assert (share[members] == d).all() and len(set(members.tolist())) == cnt[d]
        assert not cnt[depth + 1:].any()
        run = np.flatnonzero(share >= depth)
        assert (np.diff(run) == 1).all()  # the peers sharing a prefix are a run of the sorted IDs
        want_mine = [int(v) for v in run if v != p][:8]
        assert ent[depth, :cnt[depth]].tolist() == want_mine and cnt[depth] == min(8, others(depth))
        capped_runs += depth == SC.CAP_DEPTH and run.size > 9
    if name in ("clustered", "oneprefix", "lopsided"):
        assert capped_runs > 0


def _count(name, off):
    lst, q, bad, n, hops, done, peak, silent, cap_hops = R.capped(name, off)
    return dict(lookups=int(n.shape[0]), capped=int((cap_hops > 0).sum()), events=int(cap_hops.sum()),
                synced=int((done == 1).sum()), expired=int((done == 3).sum()), hops=int(hops.max()),
                longest_unbounded=int(R.unbounded(name, off)[6].max()), silent=int(silent.max()),
                offline_sources=int(SC.offline(SC.case(name)[1], off).sum()))


def test_coverage_conditions():
    """What the GPU edge tests rely on the cases for. The counts are printed (pytest -s) and quoted in DESIGN.md §7.2."""
    # a peer at the depth cap whose own bucket's run is longer than 9 (lvl_index's skip rule with m > 8)
    for name in ("clustered", "oneprefix", "lopsided"):
        key = SC.key64(SC.swarm(name))
        deep = [p for p in range(key.shape[0]) if SC.depth_of(key, p) == SC.CAP_DEPTH]
        longest = max(np.subtract(*SC.run_of(key, p, SC.CAP_DEPTH)[::-1]) for p in deep)
        print(f"{name}: {len(deep)} of {key.shape[0]} peers at depth 27, longest run {longest}")
        assert deep and longest > 9
    # the list capacity, synced and expired lookups
    for name, off in (("random5k", 8000), ("clustered", 6000)):
        c = _count(name, off)
        print(f"{name} at {off}: {c}")
        assert c["capped"] >= 20 and c["synced"] >= 100 and c["expired"] >= 50
        assert c["longest_unbounded"] > R.LIST_CAP and c["hops"] <= 32
        assert 0 < c["offline_sources"] < c["lookups"]
    for name in SC.NAMES:
        for off in SC.offline_shares(name):
            c = _count(name, off)
            assert c["hops"] <= 32
            if off:  # sources are not filtered: a share of them is offline
                assert c["offline_sources"] >= (c["lookups"] // 8 if off >= 3000 else 1), (name, off)
        lst, q, bad, n, hops, done = R.capped(name, 10000)[:6]
        assert (done[n > 0] == 3).all() and (n > 0).all()  # every peer offline: every lookup expires
    # an entry at top-64 distance ~0 (the kernels' padding key) in a tiny swarm's list; one that joins at a hop
    # (it is not in the seed list), with every peer online and with half of them offline
    tiny_far = 0
    for name in SC.TINY_NAMES:
        ids, src, tg = SC.case(name)
        mine = 0
        for off in SC.offline_shares(name)[:2]:
            r = R.capped(name, off)
            d, valid = R.top64_distances(ids, tg, r[0], r[3])
            far = ((d == FF) & valid).any(axis=1)
            mine += int(far.sum())
            if name == "tinyskew":
                d0, v0 = R.top64_distances(ids, tg, *[R.capped(name, off, 0)[k] for k in (0, 3)])
                joined = far & ~((d0 == FF) & v0).any(axis=1)
                print(f"tinyskew at {off}: {int(joined.sum())} lookups take a node at distance ~0 at a hop")
                assert joined.sum() >= 3
        assert mine > 0, name
        tiny_far += mine
    print(f"tiny swarms: {tiny_far} lists with an entry at top-64 distance ~0")
    assert tiny_far > 0
    # a top-64 tie among three peers in one list
    ids, src, tg = SC.case("clustered")
    triple = 0
    for off in (0, 6000):
        r = R.capped("clustered", off)
        d, valid = R.top64_distances(ids, tg, r[0], r[3])
        triple += int(((d[:, 2:] == d[:, :-2]) & valid[:, 2:]).any(axis=1).sum())
    print(f"clustered: {triple} lists with three entries at one top-64 distance")
    assert triple > 0
    assert any(hi - lo >= 3 for lo, hi in SC.tied_groups(ids))


SILENT_SHARES = (5000, 5500, 6000, 6500, 7000, 7500, 8000, 8500, 9000, 9400, 9700)
HIGHEST_SILENT = 62  # random5k at 7500; DESIGN.md §7.2 quotes it (shares in steps of 100 find no more)


def test_silent_capacity_is_not_reached():
    """Offline shares 5000 to 9700 on the large case swarms, unbounded lists: the most silent peers any lookup meets. No lookup reaches the device's 64, so no case exercises that branch (a
    lookup meets at most 4 silent peers a hop and the cases end within 20 hops)."""
    highest = 0
    for name in SC.BIG:
        _, src, tg = SC.case(name)
        for off in SILENT_SHARES:
            highest = max(highest, int(R.model(name).search_cap(src, tg, off, 0, 0)[7].max()))
    print(f"most silent peers in one lookup: {highest}")
    assert highest < R.SILENT_CAP, "a lookup reaches the silent-peer capacity: add its case to test_swarm_edges.py"
    assert highest == HIGHEST_SILENT
