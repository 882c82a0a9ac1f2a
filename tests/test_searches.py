"""kad_sr_try_insert_batch / _host and the device search set against Search::insertNode restated in
searches_ref.py and run on a copy of each probed search: lb, fwd, back and stop equal elementwise, over sets of
0..5000 searches in every state (empty, not full, full, expired, lists the trim loop shortens, lists of exactly cap
entries), search IDs with shared keys, last-bit neighbours, 0 and 2^160-1, and candidates placed on and beside
search IDs, members and thresholds. The expected outputs are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import searches_ref as R
from opendht_amd import DeviceSearches

CAP = 32
MIX = R.STATES
# name: (S, states, longest run of one state, batch size, seed)
CASES = {
    "s0": (0, MIX, 4, 65, 1),
    "s1": (1, ("trim",), 1, 63, 2),
    "s2": (2, MIX, 1, 65, 3),
    "s3": (3, MIX, 2, 1, 4),
    "s64": (64, MIX, 4, 4001, 5),
    "s65_notfull": (65, ("notfull", "empty", "cap"), 4, 65, 6),
    "s300_empty": (300, ("empty",), 4, 63, 7),
    "s300_full": (300, ("full",), 4, 3999, 8),
    "s300_expired": (300, ("expired",), 4, 65, 9),
    "s300_mix": (300, MIX, 4, 4000, 10),
    "s5000_mix": (5000, MIX, 3, 4000, 11),
    "s5000_empty": (5000, ("empty",), 4, 1, 12),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(searches, candidate IDs, expected (lb, fwd, back, stop)); built once, never changed."""
    S, states, run, q, seed = CASES[name]
    rng = np.random.default_rng(seed)
    searches = R.make_set(rng, S, states, CAP, run)
    cands = [0, R.MAX_ID][:q] + R.make_cands(rng, searches, max(q - 2, 0))
    return searches, cands, R.verdicts(searches, cands)


def device_set(searches, cap=CAP):
    return DeviceSearches(*R.snapshot(searches), cap=cap, device=0)


def test_expected_outputs_cover_the_verdict():
    """Every stop code on both sides, walks of two and more on both sides, a walk over a whole set."""
    fstops, bstops, fmax, bmax = set(), set(), 0, 0
    for name in CASES:
        searches, _, (lb, fwd, back, stop) = case(name)
        fstops |= set(int(v) & 15 for v in stop)
        bstops |= set(int(v) >> 4 for v in stop)
        if len(searches):
            fmax, bmax = max(fmax, int(fwd.max())), max(bmax, int(back.max()))
    assert fstops == bstops == {R.END, R.KNOWN, R.FAR, R.FAR_EXPIRED}
    assert fmax >= 2 and bmax >= 2
    for name in ("s65_notfull", "s300_empty", "s5000_empty"):
        searches, _, (lb, fwd, back, stop) = case(name)
        assert int(fwd[0]) == len(searches) and int(stop[0]) == 0  # candidate 0: the walk spans the set
    _, _, (lb, fwd, back, _) = case("s300_mix")
    assert ((fwd >= 2).sum() > 10) and ((back >= 2).sum() > 10)
    searches, _, _ = case("s300_mix")
    moved = [s for s in searches if R.trim(R.search_state(s)[2], 0)[1] < len(s.nodes) and not s.expired]
    assert len(moved) > 5 and any(len(s.nodes) == CAP for s in searches)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_try_insert_equals_insert_node(gpu, name):
    searches, cands, want = case(name)
    ids = R.id_bytes(cands)
    with device_set(searches) as DS:
        got = DS.try_insert(torch.from_numpy(ids).to(gpu))
        torch.cuda.synchronize()
        got = [g.cpu().numpy() for g in got]
        host = DS.try_insert_host(ids)
        nolb = DS.try_insert(torch.from_numpy(ids).to(gpu), want_lb=False)
        torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.view(np.uint32) if k < 3 else g
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (("lb", "fwd", "back", "stop")[k], bad[:5], g[bad[:5]], w[bad[:5]])
    for g, h in zip(got, host):
        assert np.array_equal(g.view(h.dtype), h)
    assert nolb[0] is None
    for g, h in zip(got[1:], nolb[1:]):
        assert np.array_equal(g, h.cpu().numpy())


@pytest.mark.gpu
def test_two_streams(gpu):
    searches, cands, want = case("s300_mix")
    ids = torch.from_numpy(R.id_bytes(cands)).to(gpu)
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with device_set(searches) as DS:
        a = DS.try_insert(ids, stream=s1)
        b = DS.try_insert(ids, stream=s2)
        torch.cuda.synchronize()
    for x, y, w in zip(a, b, want):
        assert np.array_equal(x.cpu().numpy().view(w.dtype), w) and np.array_equal(y.cpu().numpy().view(w.dtype), w)


def expected_export(searches, cap):
    S = len(searches)
    out = {"ids": R.id_bytes([s.id for s in searches]), "flags": np.zeros(S, np.uint8), "n": np.zeros(S, np.uint32),
           "full": np.zeros(S, np.uint8), "t": np.zeros(S, np.uint32), "node_ids": np.zeros((S, cap, 20), np.uint8),
           "node_flags": np.zeros((S, cap), np.uint8)}
    for i, s in enumerate(searches):
        fl, nid, nfl = R.search_state(s)
        full, t = R.trim(list(nfl), fl)
        out["flags"][i], out["n"][i], out["full"][i], out["t"][i] = fl, len(nfl), full, t
        out["node_ids"][i, :len(nfl)] = nid
        out["node_flags"][i, :len(nfl)] = nfl
    return out


def assert_export(DS, searches):
    got, want = DS.export(), expected_export(searches, DS.cap)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s0", "s3", "s300_mix"])
def test_export_reads_back_the_set(gpu, name):
    searches, _, _ = case(name)
    with device_set(searches) as DS:
        assert_export(DS, searches)
        assert DS.device_bytes == len(searches) * (64 + 8 + CAP * 21)


@pytest.mark.gpu
def test_patch(gpu):
    """A third of the searches replaced (grown, shrunk, flags flipped): the export equals the host arrays and the
    verdicts those of a freshly created set, and of the restatement."""
    searches, cands, _ = case("s300_mix")
    rng = np.random.default_rng(77)
    which = np.sort(rng.choice(len(searches), size=len(searches) // 3, replace=False))
    which[:4] = (0, 1, 2, 3)  # a run of consecutive searches, the first of the set included
    which = np.unique(which)
    after = list(searches)
    for k, s in enumerate(which):
        old = searches[s]
        if k % 3 == 0 and old.nodes:  # flags flipped, same list
            after[s] = R.Search(old.id, not old.expired,
                                [R.SearchNode(sn.node, not sn.candidate and not sn.node.expired) for sn in old.nodes])
        else:  # another state: grown or shrunk
            after[s] = R.make_search(rng, old.id, R.STATES[int(rng.integers(0, len(R.STATES)))], CAP)
    ids = R.id_bytes(cands)
    with device_set(searches) as DS, device_set(after) as fresh:
        _, flags, off, nid, nfl = R.snapshot([after[s] for s in which])
        DS.patch(which, flags, off, nid, nfl)
        assert_export(DS, after)
        got, want = DS.try_insert_host(ids), fresh.try_insert_host(ids)
    ref = R.verdicts(after, cands)
    for g, w, r in zip(got, want, ref):
        assert np.array_equal(g, w) and np.array_equal(g, r)
    assert any(not np.array_equal(r, o) for r, o in zip(ref, case("s300_mix")[2]))  # the patch changed verdicts


@pytest.mark.gpu
def test_patch_and_create_refusals_leave_the_set(gpu):
    from opendht_amd import KadError, _lib
    searches, _, _ = case("s64")
    with device_set(searches) as DS:
        _, flags, off, nid, nfl = R.snapshot(searches[:2])
        for which in ([1, 0], [3, 3], [0, 64]):
            with pytest.raises(KadError) as e:
                DS.patch(np.array(which, np.uint32), flags, off, nid, nfl)
            assert e.value.code == _lib.KAD_ERR_INVALID
        k = next(i for i, s in enumerate(searches) if len(s.nodes) >= 2)
        _, flags, off, nid, nfl = R.snapshot([searches[k]])
        nid[[0, 1]] = nid[[1, 0]]
        with pytest.raises(KadError) as e:  # a list that does not ascend in distance
            DS.patch(np.array([k], np.uint32), flags, off, nid, nfl)
        assert e.value.code == _lib.KAD_ERR_INVALID
        assert_export(DS, searches)
    big = [R.make_search(np.random.default_rng(3), 5, "cap", CAP + 1)]
    with pytest.raises(KadError) as e:
        device_set(big, cap=CAP)
    assert e.value.code == _lib.KAD_ERR_UNSUPPORTED
    with device_set(big, cap=CAP + 1) as DS:  # recreated with a larger cap
        assert_export(DS, big)
