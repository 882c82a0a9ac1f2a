"""The dual-family query calls over every branch of their dispatch: kad_rt_closest_batch_dual (seventeen launches)
and kad_nc_closest_batch_dual (five), the calls Dht::onGetValues and Dht::refill make. Each pair of dual_cases.py
runs every count of its call on adversarial targets of both families (node IDs, bucket bounds, 00..0, FF..F) with
the per-query family drawn six ways (alternating, random, uniform per wave, uniform per workgroup, all 0, all 1),
bit for bit against the oracle's closed form per family (pinned to the structure-faithful restatement on these
tables by test_dual_cases.py), and against the single-table call on the same table as a diagnosis aid. The tables
are held to the line sets their class must carry, and every pair to the launch its line of the list names, so the
branch under test is the one that ran. Then: a different index_base per family, a NULL count pointer, and a status
patch of both families before one launch reads both rebuilt line sets."""
import ctypes as C

import numpy as np
import pytest
import torch

import dual_cases as DC
from opendht_amd import DeviceTable
from opendht_amd._lib import KAD_NO_NODE, check, lib, ptr

pytestmark = pytest.mark.gpu

FILL = 0x7B7B7B7B  # rows are written whole: no entry of a result keeps the buffer's fill


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _make(cls, gpu, index_base=0):
    t = DC.table(cls)
    T = DeviceTable(t["ids"], t["status"], t["first"], t["off"], device=gpu.index or 0, index_base=index_base,
                    sorted=t["sorted"])
    T.prepare()
    return T


@pytest.fixture(scope="module")
def dt(gpu):
    """The catalogue on the device, each table built once (per index_base) and prepared; None for a missing family."""
    built = {}

    def get(cls, index_base=0):
        if cls == "NONE":
            return None
        if (cls, index_base) not in built:
            built[cls, index_base] = _make(cls, gpu, index_base)
        return built[cls, index_base]

    yield get
    for T in built.values():
        T.close()
    DC.release()


def _state(cls, T):
    """The family's dispatch state, held to what its class must carry (a failure of the fixture, never a skip)."""
    s = DC.state(None if T is None else T.info())
    for k, v in DC.MUST_CARRY.get(cls, {}).items():
        assert s[k] == v, f"{cls} must carry {k}={v}: {s}"
    return s


def _dual(kind, T4, T6, tg, afd, count, with_cnt=True):
    """The ABI call on buffers filled beforehand. Returns (rows uint32, counts or None) on the host."""
    q = tg.shape[0]
    out = torch.full((q, count), FILL, dtype=torch.int32, device=tg.device)
    cnt = torch.full((q,), 0xEE, dtype=torch.uint8, device=tg.device) if with_cnt else None
    fn = lib().kad_rt_closest_batch_dual if kind == "rt" else lib().kad_nc_closest_batch_dual
    s = C.c_void_p(torch.cuda.current_stream(tg.device).cuda_stream)
    check(fn(T4.handle if T4 else None, T6.handle if T6 else None, ptr(tg), ptr(afd), q, count, ptr(out), ptr(cnt), s),
          f"kad_{kind}_closest_batch_dual")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), (cnt.cpu().numpy() if with_cnt else None)


def _single(kind, T, tg, count):
    """The single-table call's rows (the diagnosis aid); empty rows for a missing family."""
    if T is None:
        return np.full((tg.shape[0], count), KAD_NO_NODE, np.uint32)
    idx, _ = (T.rt_closest if kind == "rt" else T.nc_closest)(tg, count)
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint32)


def _want(kind, cls, fam4, fam6, count, base=0, status=None):
    rows = DC.expected_pair(kind, cls, fam4, fam6, count, status)
    if base:
        rows = np.where(rows == KAD_NO_NODE, rows, rows + np.uint32(base))
    return rows


def _check_pair(kind, gpu, dt, fam4, fam6, counts, patterns_for, base6=0, tables=None, status=None):
    """One pair, every count of `counts`, the af patterns patterns_for(count): the launch its list line names, rows
    and counts against the oracle per family, rows against the single-table call."""
    T4, T6 = tables if tables is not None else (dt(fam4), dt(fam6, base6))
    s4, s6 = _state(fam4, T4), _state(fam6, T6)
    all_counts = DC.RT_COUNTS if kind == "rt" else DC.NC_COUNTS
    named = {k: br.launch for br in DC.branches_of(DC.RT_BRANCHES if kind == "rt" else DC.NC_BRANCHES, fam4, fam6)
             for k in DC.branch_counts(br, all_counts)}
    model = DC.rt_launch if kind == "rt" else DC.nc_launch
    targets, _, _ = DC.pair_targets(fam4, fam6)
    tg = _dev(targets, gpu)
    q = targets.shape[0]
    afs = {name: DC.af_pattern(name, q) for name in DC.AF_PATTERNS}
    afd = {name: _dev(af, gpu) for name, af in afs.items()}
    st4, st6 = status if status is not None else (None, None)
    for k in counts:
        where = f"{kind} {fam4}+{fam6} count={k}"
        assert model(s4, s6, k) == named[k], f"{where}: the tables take {model(s4, s6, k)}, the list says {named[k]}"
        w4, w6 = _want(kind, fam4, fam4, fam6, k, 0, st4), _want(kind, fam6, fam4, fam6, k, base6, st6)
        one4, one6 = _single(kind, T4, tg, k), _single(kind, T6, tg, k)
        for name in patterns_for(k):
            six = afs[name] != 0
            rows, cnt = _dual(kind, T4, T6, tg, afd[name], k)
            want = np.where(six[:, None], w6, w4)
            one = np.where(six[:, None], one6, one4)
            msg = (f"{where} af={name} ({named[k]}; the single-table calls "
                   f"{'agree' if np.array_equal(one, want) else 'DISAGREE'} with the oracle)")
            np.testing.assert_array_equal(rows, want, err_msg=msg + " rows")
            # the count byte saturates at 255; beyond it the row's padding gives the length
            np.testing.assert_array_equal(cnt, np.minimum(DC.rows_len(want), 255), err_msg=msg + " counts")
            np.testing.assert_array_equal(rows, one, err_msg=msg + " rows against the single-table call")
            if base6:  # every non-padding entry carries its own family's base
                real = rows != KAD_NO_NODE
                lo = np.where(six, np.uint32(base6), np.uint32(0))[:, None]
                n = np.where(six, s6["n"], s4["n"])[:, None]
                assert ((rows >= lo) & (rows - lo < n))[real].all(), msg + " index_base"


def _patterns(k):
    return DC.AF_PATTERNS if k in DC.PATTERN_COUNTS else ("random",)


@pytest.mark.parametrize("cls", [c for c in DC.CLASSES if c != "NONE"])
def test_catalogue_carries_its_lines(gpu, dt, cls):
    """Every catalogue table carries the line sets its class must (the others' are printed for the record)."""
    s = _state(cls, dt(cls))
    t = DC.table(cls)
    assert s["B"] == t["first"].shape[0] and s["n"] == t["ids"].shape[0]
    print(cls, " ".join(sorted(k for k, v in s.items() if v is True)), f"B={s['B']} n={s['n']}")


@pytest.mark.parametrize("fam4,fam6", DC.pairs(DC.RT_BRANCHES), ids=lambda c: c)
def test_rt_dual(gpu, dt, fam4, fam6):
    """kad_rt_closest_batch_dual: counts 1..32, 33, 40, 64, 65, 100, 300."""
    _check_pair("rt", gpu, dt, fam4, fam6, DC.RT_COUNTS, _patterns)


@pytest.mark.parametrize("fam4,fam6", DC.pairs(DC.NC_BRANCHES), ids=lambda c: c)
def test_nc_dual(gpu, dt, fam4, fam6):
    """kad_nc_closest_batch_dual: counts 1..32, 33, 40, 48, 63, 64, 65, 100, 300."""
    _check_pair("nc", gpu, dt, fam4, fam6, DC.NC_COUNTS, _patterns)


@pytest.mark.parametrize("kind,fam4,fam6", [("rt",) + p for p in DC.RT_BASE_PAIRS] + [("nc",) + p for p in DC.NC_BASE_PAIRS],
                         ids=lambda c: c)
def test_index_base_per_family(gpu, dt, kind, fam4, fam6):
    """Family 4 at index_base 0, family 6 at 0x40000000: each row's entries carry the base of the row's family."""
    _check_pair(kind, gpu, dt, fam4, fam6, DC.BASE_COUNTS, lambda k: ("random", "alternating"), base6=DC.BASE6)


@pytest.mark.parametrize("fam4,fam6", DC.NULL_CNT_PAIRS, ids=lambda c: c)
def test_null_count_pointer(gpu, dt, fam4, fam6):
    """out_cnt == NULL: the same rows as with the pointer (and as the oracle's)."""
    T4, T6 = dt(fam4), dt(fam6)
    _state(fam4, T4), _state(fam6, T6)
    targets, _, _ = DC.pair_targets(fam4, fam6)
    tg = _dev(targets, gpu)
    af = DC.af_pattern("random", targets.shape[0])
    afd = _dev(af, gpu)
    for k in DC.NULL_CNT_COUNTS:
        rows, _ = _dual("rt", T4, T6, tg, afd, k)
        bare, none = _dual("rt", T4, T6, tg, afd, k, with_cnt=False)
        assert none is None
        want = np.where(af[:, None] != 0, _want("rt", fam6, fam4, fam6, k), _want("rt", fam4, fam4, fam6, k))
        np.testing.assert_array_equal(bare, rows, err_msg=f"{fam4}+{fam6} count={k}: rows without out_cnt")
        np.testing.assert_array_equal(bare, want, err_msg=f"{fam4}+{fam6} count={k}: rows without out_cnt, oracle")


def test_after_status_patch(gpu):
    """1 % of each family's nodes patched to random 0 / 1 / 2: one dual launch reads the rebuilt lines of both."""
    fam4, fam6 = DC.STATUS_PAIR
    rng = np.random.default_rng(0x57A)
    T4, T6 = _make(fam4, gpu), _make(fam6, gpu)
    try:
        status = []
        for cls, T in ((fam4, T4), (fam6, T6)):
            st = DC.table(cls)["status"].copy()
            nodes = rng.choice(st.shape[0], size=st.shape[0] // 100, replace=False).astype(np.uint32)
            st[nodes] = rng.integers(0, 3, nodes.shape[0]).astype(np.uint8)
            T.patch_status(nodes, st[nodes])
            status.append(st)
        _check_pair("rt", gpu, None, fam4, fam6, DC.STATUS_COUNTS, lambda k: DC.AF_PATTERNS, tables=(T4, T6),
                    status=tuple(status))
    finally:
        T4.close()
        T6.close()
