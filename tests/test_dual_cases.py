"""CPU side of the dual-family matrix (test_dual_matrix.py): the pair list names every launch of the two dual
dispatches, its lines agree with the dispatch model on the tables whose line sets are required, and the closed form
the GPU tests compare against equals the structure-faithful restatement on every catalogue table."""
import numpy as np
import pytest

import dual_cases as DC
import oracle as O
import tables as TB


def test_pair_list_names_every_launch():
    """Seventeen RoutingTable launches (the three instances of rt_dual_gl_kernel and of launch_rt_dual counted each)
    and five NodeCache launches, every one the stated purpose of at least one line of the pair list."""
    assert len(DC.RT_LAUNCHES) == 17 and len(set(DC.RT_LAUNCHES)) == 17
    assert len(DC.NC_LAUNCHES) == 5 and len(set(DC.NC_LAUNCHES)) == 5
    for launches, branches, counts in ((DC.RT_LAUNCHES, DC.RT_BRANCHES, DC.RT_COUNTS),
                                       (DC.NC_LAUNCHES, DC.NC_BRANCHES, DC.NC_COUNTS)):
        named = {br.launch for br in branches if DC.branch_counts(br, counts)}
        assert named == set(launches), set(launches) ^ named
        # the lines of a pair split the counts among them: each count in exactly one line
        for fam4, fam6 in DC.pairs(branches):
            got = sorted(k for br in DC.branches_of(branches, fam4, fam6) for k in DC.branch_counts(br, counts))
            assert got == sorted(counts), (fam4, fam6)
    for fam4, fam6 in DC.pairs(DC.RT_BRANCHES + DC.NC_BRANCHES):
        assert fam4 in DC.CLASSES and fam6 in DC.CLASSES and (fam6, fam4) in DC.pairs(DC.RT_BRANCHES + DC.NC_BRANCHES)
    for p in DC.RT_BASE_PAIRS + DC.NULL_CNT_PAIRS + (DC.STATUS_PAIR,):
        assert p in DC.pairs(DC.RT_BRANCHES), p
    for p in DC.NC_BASE_PAIRS:
        assert p in DC.pairs(DC.NC_BRANCHES), p
    # NodeCache pairs hold sorted tables only
    for fam4, fam6 in DC.pairs(DC.NC_BRANCHES):
        for cls in (fam4, fam6):
            assert DC.table(cls) is None or DC.table(cls)["sorted"], cls


def _required_state(cls):
    """The dispatch state of a class whose line sets MUST_CARRY fixes, built from the requirement alone."""
    t, req = DC.table(cls), DC.MUST_CARRY.get(cls, {})
    s = DC.state(None)
    if t is None:
        return s
    s.update(B=t["first"].shape[0], n=t["ids"].shape[0])
    s.update({k: v for k, v in req.items() if k in s})
    s["wl16"], s["wl32"] = s["window"] and s["rt16"], s["window"] and s["rt32"]
    s["ncl"], s["ncl32"] = s["nc16"], s["nc32"]
    return s


def test_pair_list_agrees_with_dispatch_model():
    """On the pairs made of classes with required line sets (and missing / bucketless families), each line's launch
    is what the dispatch model picks for every count of its range; these pairs alone reach all 22 launches."""
    fixed = set(DC.MUST_CARRY) | {"NONE"}
    reached = set()
    for branches, counts, model in ((DC.RT_BRANCHES, DC.RT_COUNTS, DC.rt_launch),
                                    (DC.NC_BRANCHES, DC.NC_COUNTS, DC.nc_launch)):
        for br in branches:
            if br.fam4 not in fixed or br.fam6 not in fixed or "EMPTY_B1" in (br.fam4, br.fam6):
                continue
            s4, s6 = _required_state(br.fam4), _required_state(br.fam6)
            for k in DC.branch_counts(br, counts):
                assert model(s4, s6, k) == br.launch and model(s6, s4, k) == br.launch, (br, k)
                reached.add(br.launch)
    assert reached == set(DC.RT_LAUNCHES) | set(DC.NC_LAUNCHES), (set(DC.RT_LAUNCHES) | set(DC.NC_LAUNCHES)) - reached


def test_af_patterns_and_targets():
    for fam4, fam6 in DC.pairs(DC.RT_BRANCHES + DC.NC_BRANCHES):
        tg, n4, n6 = DC.pair_targets(fam4, fam6)
        assert tg.shape == (n4 + n6, 20) and tg.shape[0] % 2 == 1 and 2049 <= tg.shape[0] <= 3000, (fam4, fam6)
    q = 2501
    for name in DC.AF_PATTERNS:
        af = DC.af_pattern(name, q)
        assert af.dtype == np.uint8 and af.shape == (q,) and set(np.unique(af)) <= {0, 1}
    for name, run in (("runs64", 64), ("runs256", 256)):  # uniform per wave / per workgroup, both values present
        whole = DC.af_pattern(name, q)[:q // run * run].reshape(-1, run)
        assert (whole == whole[:, :1]).all() and set(whole[:, 0]) == {0, 1}
    assert DC.af_pattern("runs64", q)[63] != DC.af_pattern("runs64", q)[64]
    assert 0.4 < DC.af_pattern("random", q).mean() < 0.6


RESTATEMENT_COUNTS = tuple(range(1, 33)) + (33, 64)


@pytest.mark.parametrize("cls", [c for c in DC.CLASSES if c != "NONE"])
def test_restatements_agree_on_catalogue(cls):
    """flat_rt_closest / flat_nc_closest (the expected side of test_dual_matrix.py) against FaithfulTable on every
    catalogue table, for every count 1..32, 33 and 64; the NodeCache pair on the sorted tables."""
    t = DC.table(cls)
    targets = TB.adversarial_targets(t, extra=256)
    if "near" in t:
        near = t["near"].copy()
        near[:, 19] ^= 0x5A
        targets = np.ascontiguousarray(np.concatenate([targets, near]))
    T = O.FaithfulTable(t["ids"], t["status"], t["first"], t["off"], with_nc=t["sorted"])
    for k in RESTATEMENT_COUNTS:
        a, ac = T.rt_closest(targets, k, nthreads=8)
        b, bc = O.flat_rt_closest(t["ids"], t["status"], t["first"], t["off"], targets, k, nthreads=8)
        np.testing.assert_array_equal(ac, bc, err_msg=f"{cls} k={k} counts")
        np.testing.assert_array_equal(a, b, err_msg=f"{cls} k={k} rows")
        if t["sorted"]:
            a, ac = T.nc_closest(targets, k, nthreads=8)
            b, bc = O.flat_nc_closest(t["ids"], t["status"], targets, k, nthreads=8)
            np.testing.assert_array_equal(ac, bc, err_msg=f"{cls} nc k={k} counts")
            np.testing.assert_array_equal(a, b, err_msg=f"{cls} nc k={k} rows")
    T.close()
