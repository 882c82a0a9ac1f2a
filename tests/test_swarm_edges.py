"""Config 5 at its edges on the GPU, bit-exact against the oracle under the device's capacities
(list_cap = 32, silent_cap = 64): the case swarms of swarm_cases.py — tiny swarms, the depth cap, one-sided tables, ties
among three peers, distances equal to the padding key, offline sources — table by table, query by query and hop by hop
at offline shares up to every peer; out-of-range sources, batch sizes around a block, the state pool after a search
that hit the list capacity, and every hop variant kad_search_hop can be switched to, each in a process of its own."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle as O
import swarm_cases as SC
import swarm_ref as R
from swarm_variant_worker import variant_case
from test_swarm import _check_lookup_properties_vec

pytestmark = pytest.mark.gpu

SHAPED = ("clustered", "oneprefix", "lopsided") + SC.TINY_NAMES
MAX_HOPS = 32
HERE = os.path.dirname(os.path.abspath(__file__))


def _dev(gpu, a, dtype=None):
    a = np.array(a)  # (a copy: the cases are read-only)
    return torch.from_numpy(a.view(dtype) if dtype else a).to(gpu)


def _search(W, gpu, src, tg, off):
    return W.search(_dev(gpu, np.asarray(src, np.uint32), np.int32), _dev(gpu, tg), off)


def _check_state(got, want, where):
    """got: Search.get(full=True); want: the capped oracle's tuple. Every field, the padding and the overflow count."""
    for a, b, f in zip(got[:6], want, R.FIELDS):
        np.testing.assert_array_equal(a, b, err_msg=f"{where}: {f}")
    assert got[6] == int(want[8].sum()), f"{where}: overflow {got[6]}, the oracle's capacity events {int(want[8].sum())}"
    lst, q, bad, n = got[:4]
    assert n.max(initial=0) <= R.LIST_CAP
    pad = np.arange(lst.shape[1])[None, :] >= n.astype(np.int64)[:, None]
    assert (lst[pad] == O.NO_NODE).all() and not q[pad].any() and not bad[pad].any(), f"{where}: padding"
    assert (got[5] != 4).all(), f"{where}: the tie hand-off (done = 4) is visible after a hop"


def _check_properties(ids, tg, got, want, off):
    """_check_lookup_properties_vec; a lookup that forgot a silent peer (the oracle remembered silent_cap of them) may
    hold that peer queried and non-bad again, so it is checked without that clause."""
    lst, q, bad, n, hops, done = got[:6]
    kept = want[7] < R.SILENT_CAP
    _check_lookup_properties_vec(ids, lst[kept], q[kept], bad[kept], n[kept], done[kept], off, tg[kept])
    if not kept.all():
        d, valid = R.top64_distances(ids, tg[~kept], lst[~kept], n[~kept])
        assert ((d[:, 1:] >= d[:, :-1]) | ~valid[:, 1:]).all()
        assert ((~bad[~kept].astype(bool) & valid).sum(axis=1) <= 14).all()


def _run_hop_by_hop(X, want_at, where, max_hops=MAX_HOPS):
    """Hops until no lookup is active, every hop's state against want_at(h); returns the last state and oracle."""
    got = want = None
    for h in range(1, max_hops + 1):
        active = X.hop()
        got, want = X.get(full=True), want_at(h)
        _check_state(got, want, f"{where} hop {h}")
        assert active == int((want[5] == 0).sum())
        if active == 0:
            return got, want
    raise AssertionError(f"{where}: lookups still active after {max_hops} hops")


@pytest.mark.parametrize("name", SHAPED)
def test_swarm_edges_tables_and_closest(gpu, name):
    """Every peer's table equals the oracle's, and Swarm.closest at counts 1, 8, 14 and 16 over the case's targets."""
    from opendht_amd.swarm import Swarm
    ids, src, tg = SC.case(name)
    M = R.model(name)
    with Swarm(ids, device=gpu.index or 0) as W:
        for p in range(ids.shape[0]):
            d, c, e = W.table(p)
            wd, wc, we = M.table(p)
            assert d == wd, f"peer {p}: depth"
            np.testing.assert_array_equal(c, wc, err_msg=f"peer {p}: counts")
            np.testing.assert_array_equal(e, we, err_msg=f"peer {p}: entries")
        pt, tt = _dev(gpu, src, np.int32), _dev(gpu, tg)
        for count in (1, 8, 14, 16):
            idx, cnt = W.closest(pt, tt, count)
            torch.cuda.synchronize()
            want, wcnt = M.closest(src, tg, count)
            np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt, err_msg=f"count {count}")
            np.testing.assert_array_equal(idx.cpu().numpy().view(np.uint32), want, err_msg=f"count {count}")


@pytest.mark.parametrize("name,off", [(n, o) for n in SC.NAMES for o in SC.offline_shares(n)])
def test_swarm_edges_lookups_hop_by_hop(gpu, name, off):
    """Every case at every offline share, sources unfiltered: each hop's lists, flags, lengths, hop counts, done and
    overflow equal to the capped oracle, and the model's invariants on the end state."""
    from opendht_amd.swarm import Swarm
    ids, src, tg = SC.case(name)
    with Swarm(ids, device=gpu.index or 0) as W:
        X = _search(W, gpu, src, tg, off)
        got, want = _run_hop_by_hop(X, lambda h: R.capped(name, off, h), f"{name} at {off}")
        X.close()
    for a, b in zip(want, R.capped(name, off)):  # (the oracle's run to the end is the same state)
        np.testing.assert_array_equal(a, b)
    _check_properties(ids, tg, got, want, off)
    if (name, off) in (("random5k", 8000), ("clustered", 6000)):
        assert got[6] >= 20 and (got[5] == 3).sum() >= 50  # the capacity branch and expired lookups did run


def test_swarm_edges_out_of_range_sources(gpu):
    """Sources >= n spliced into a batch: empty lists, done = 2 (stalled), hops = 0, at every hop; the rows around
    them equal to the oracle's run of the in-range rows alone."""
    from opendht_amd.swarm import Swarm
    name, off = "clustered", 3000
    ids, src, tg = SC.case(name)
    n = ids.shape[0]
    src, tg = src[:700].copy(), tg[:700]
    out = np.zeros(700, bool)
    out[[0, 1, 63, 64, 255, 256, 257, 511, 699]] = True
    out[300:310] = True
    src[out] = np.resize(np.array([n, n + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32), int(out.sum()))
    M = R.model(name)
    with Swarm(ids, device=gpu.index or 0) as W:
        X = _search(W, gpu, src, tg, off)
        for h in range(0, MAX_HOPS + 1):
            active = X.hop() if h else None
            got = X.get(full=True)
            want = M.search_cap(src[~out], tg[~out], off, R.LIST_CAP, R.SILENT_CAP, max_hops=h)
            _check_state([a[~out] for a in got[:6]] + [got[6]], want, f"hop {h}, in-range rows")
            lst, q, bad, nn, hops, done = (a[out] for a in got[:6])
            assert (lst == O.NO_NODE).all() and not q.any() and not bad.any() and not nn.any()
            assert (done == 2).all() and not hops.any()
            if active == 0:
                break
        assert active == 0
        X.close()


@pytest.mark.parametrize("S", [0, 1, 255, 256, 257])
def test_swarm_edges_batch_sizes(gpu, S):
    """Batches of no lookup, one, and one less, exactly and one more than a block of 256 (offline peers and none)."""
    from opendht_amd.swarm import Swarm
    name = "lopsided"
    ids, src, tg = SC.case(name)
    M = R.model(name)
    with Swarm(ids, device=gpu.index or 0) as W:
        for off in (0, 6000):
            s, t = src[100:100 + S], tg[100:100 + S]
            X = _search(W, gpu, s, t, off)
            if S == 0:
                assert X.hop() == 0
                got = X.get(full=True)
                assert all(a.shape[0] == 0 for a in got[:6]) and got[6] == 0
            else:
                _run_hop_by_hop(X, lambda h: M.search_cap(s, t, off, R.LIST_CAP, R.SILENT_CAP, max_hops=h),
                                f"S = {S} at {off}")
            X.close()


def test_swarm_edges_pool_reuse_after_capacity(gpu):
    """A search that hit the list capacity (overflow > 0, silent peers remembered) hands its state to the swarm's pool;
    the next searches, smaller and all online, then with offline peers again, start from overflow = 0 and no silent
    peer: each equal to the oracle hop by hop."""
    from opendht_amd.swarm import Swarm
    name = "clustered"
    ids, src, tg = SC.case(name)
    M = R.model(name)
    with Swarm(ids, device=gpu.index or 0) as W:
        X = _search(W, gpu, src, tg, 8000)
        got, want = _run_hop_by_hop(X, lambda h: R.capped(name, 8000, h), "first search")
        assert got[6] > 0 and want[7].max() > 8
        X.close()
        for off, cut in ((0, 1500), (6000, 1995), (3000, 900)):
            s, t = src[:cut], tg[:cut]
            X = _search(W, gpu, s, t, off)
            assert X.get(full=True)[6] == 0
            # a silent peer left over from the pooled state would turn a re-inserted offline node bad too early; an
            # overflow count left over would show at the first hop
            _run_hop_by_hop(X, lambda h: M.search_cap(s, t, off, R.LIST_CAP, R.SILENT_CAP, max_hops=h),
                            f"reuse at {off}")
            X.close()


def test_swarm_edges_close_order(gpu):
    """Swarm.close() closes the searches still open on it first (a search hands its state to its swarm's pool when it
    is destroyed: destroyed after the swarm it would write to freed memory); closing either again is harmless."""
    from opendht_amd.swarm import Swarm
    ids, src, tg = SC.case("tiny17")
    W = Swarm(ids, device=gpu.index or 0)
    Xa, Xb = _search(W, gpu, src, tg, 0), _search(W, gpu, src[:50], tg[:50], 5000)
    Xa.hop()
    Xb.close()
    W.close()
    assert Xa._h is None and Xb._h is None and W._h is None
    Xa.close()
    W.close()


# ---- hop variants: one child process each (the switches are read once per process) --------------------------------
VARIANTS = {
    "default": {},
    "netpf0": {"KAD_SWARM_NETPF": "0"},
    "seq": {"KAD_SWARM_SEQ": "1"},
    "wide": {"KAD_SWARM_WIDE": "1"},
    "query_ins": {"KAD_SWARM_QUERY": "ins"},
    "fused": {"KAD_SWARM_FUSED": "1"},
    "query_ins_seq": {"KAD_SWARM_QUERY": "ins", "KAD_SWARM_SEQ": "1"},
}
VARIANT_CASES = ("clustered@0", "clustered@6000", "tinyskew@0", "tied_pairs")
_child_trouble = []  # a child that ended on a signal or at its time limit: no further child in this session
_default_run = {}


@functools.lru_cache(maxsize=None)
def _variant_want(case, h):
    """The capped oracle's state of a variant case after h hops (shared by the variants)."""
    if "@" in case:
        name, off = case.rsplit("@", 1)
        return R.capped(name, int(off), h)
    ids, src, tg, off = variant_case(case)
    M = O.SwarmModel(ids)
    want = M.search_cap(src, tg, off, R.LIST_CAP, R.SILENT_CAP, max_hops=h)
    M.close()
    return want


def _run_worker(case, variant, tmp_path):
    if _child_trouble:
        pytest.fail(f"no further child is started: {_child_trouble[0]}")
    env = {k: v for k, v in os.environ.items() if not k.startswith("KAD_SWARM_")}
    env.update(VARIANTS[variant])
    out = tmp_path / f"{variant}.npz"
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "swarm_variant_worker.py"), case, str(out)], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _child_trouble.append(f"{case} / {variant} hit its time limit")
        pytest.fail(_child_trouble[0])
    if r.returncode < 0:
        _child_trouble.append(f"{case} / {variant} ended on signal {-r.returncode}")
        pytest.fail(_child_trouble[0] + "\n" + r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", VARIANT_CASES)
def test_swarm_edges_hop_variants(gpu, tmp_path, case, variant):
    """Every form of the hop — the merge network with and without its prefetch, the narrow and the wide sequential
    merge, the query by network and by inserts, the fused kernel — gives the oracle's state after every hop; on the
    all-online cases the variants' bytes are identical to the default's, and done = 4 never shows."""
    off = variant_case(case)[3]
    got = _run_worker(case, variant, tmp_path)
    H = got["active"].shape[0]
    assert H <= MAX_HOPS and got["active"][-1] == 0
    for h in range(1, H + 1):
        want = _variant_want(case, h)
        state = [got[f][h - 1] for f in R.FIELDS] + [int(got["overflow"][h - 1])]
        _check_state(state, want, f"{case} / {variant} hop {h}")
        assert got["active"][h - 1] == (want[5] == 0).sum()
    if off == 0:
        if case not in _default_run:
            _default_run[case] = got if variant == "default" else _run_worker(case, "default", tmp_path)
        for k, v in _default_run[case].items():
            assert v.tobytes() == got[k].tobytes(), f"{case} / {variant}: {k} differs from the default hop's"
