"""kad_searches_apply against its model in apply_ref.py: delete from the list, add empty searches,
sort by ID. After every apply the set must equal one freshly created from the model at the final cap: all seven export
arrays, the device bytes, and the trySearchInsert verdicts of make_cands plus every search ID, its neighbours in the
last byte, 00..0 and FF..F, against the fresh set and searches_ref.verdicts.

The shapes are the smallest at which each mechanism can break: sets of 0 to 5 searches for the positions; runs of 1,
63, 64, 65 and 257 erased or inserted searches (wave and workgroup edges of the relayout); 4095 to 4097 and 8192 to
8193 searches at cap 14 for the switch between the dense key array and the prefix directory and for a change of its
bit count; every pair of old and new cap around the multiples of 16 that select the 16-byte path (16->32, 32->64) or
the narrow one (everything else)."""
import ctypes as C

import numpy as np
import pytest

import apply_ref as A
import refill_ref as F
import searches_ref as R
from opendht_amd import DeviceSearches, DeviceTable, KadError, _lib, expire_searches, start_searches

NOW = A.NOW
GUARD = 0xA5A5A5A5
p = _lib.ptr


def make(model, cap, stray=False):
    return DeviceSearches(*A.snap(model, stray), cap=cap, device=0)


# ---- set size and positions -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_empty_to_five_and_back(gpu):
    five = A.base(5, 32)
    with make([], 32) as DS:
        m = A.apply(DS, [])                                     # 0 -> 0: nothing to do
        A.compare(DS, m, 32, tag="0->0")
        m = A.apply(DS, m, cap=64)                              # 0 -> 0 with larger slabs: still no device arrays
        assert DS.device_bytes == 0
        A.compare(DS, m, 64, tag="0->0 cap")
        m = A.apply(DS, m, ins=[s.id for s in five][::-1], expired=[0, 1, 0, 1, 1])  # 0 -> 5, descending input
        assert [s.expired for s in m] == [True, True, False, True, False]
        A.compare(DS, m, 64, tag="0->5")
        m = A.apply(DS, m, erase=range(5))                      # 5 -> 0
        assert DS.device_bytes == 0
        A.compare(DS, m, 64, tag="5->0")
        m = A.apply(DS, m, ins=[7])                             # and a set emptied by apply accepts inserts
        A.compare(DS, m, 64, tag="0->1")
    with make(five, 32) as DS:                                  # 5 -> 0 on a created set, then destroy
        A.compare(DS, A.apply(DS, five, erase=range(5)), 32, tag="created 5->0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["before_first", "after_last", "between", "erase_first", "erase_last", "all_but_one"])
def test_positions(gpu, case):
    model = A.base(40, 32)
    S = len(model)
    erase, ins = {
        "before_first": ((), [0]),
        "after_last": ((), [R.MAX_ID]),
        "between": ((), A.free_between(model, 20, 1)),
        "erase_first": ([0], ()),
        "erase_last": ([S - 1], ()),
        "all_but_one": ([i for i in range(S) if i != 17], ()),
    }[case]
    with make(model, 32) as DS:
        A.compare(DS, A.apply(DS, model, erase, ins), 32, tag=case)


@pytest.mark.gpu
def test_ids_tied_on_the_top_64_bits_with_a_kept_search(gpu):
    """Inserted IDs share the 64-bit key of a kept search and differ in the tail only, on both sides of it: the lower
    bound over skey settles them from the record tails."""
    model = A.base(40, 32)
    have = set(s.id for s in model)
    lonely = [i for i, s in enumerate(model) if not {A.last_byte(s.id, 1), A.last_byte(s.id, -1)} & have]
    ins = []
    for i in (lonely[0], lonely[len(lonely) // 2], lonely[-1]):
        k, key = model[i].id, model[i].id >> 96 << 96
        below, above = key | ((k & ((1 << 96) - 1)) // 2), key | ((k & ((1 << 96) - 1)) // 2 + (1 << 95))
        assert below < k < above and below >> 96 == k >> 96 == above >> 96
        ins += [above, below, A.last_byte(k, 1), A.last_byte(k, -1)]
    assert len(set(ins) | set(s.id for s in model)) == len(ins) + len(model)
    with make(model, 32) as DS:
        m = A.apply(DS, model, ins=ins)
        A.compare(DS, m, 32, tag="tied")
        # and the kept searches between tied neighbours go: the inserted ones stay in order
        A.compare(DS, A.apply(DS, m, erase=[i for i, s in enumerate(m) if s in model and i % 2]), 32, tag="tied erase")


@pytest.mark.gpu
def test_erase_and_reinsert_the_same_id(gpu):
    model = A.base(40, 32)
    full = [i for i, s in enumerate(model) if len(s.nodes) >= 14][:3]
    assert len(full) == 3
    with make(model, 32) as DS:
        before = DS.export()
        remap, new_index = DS.apply(np.array(full, np.uint32), R.id_bytes([model[i].id for i in full]))
        assert (remap[full] == A.NO_NODE).all() and np.array_equal(new_index, np.array(full, np.uint32))
        after = DS.export()
        assert np.array_equal(after["ids"], before["ids"])
        assert (after["n"][full] == 0).all() and (after["t"][full] == 0).all() and (after["full"][full] == 0).all()
        assert not after["node_ids"][full].any() and not after["node_flags"][full].any()
        assert before["n"][full].all()
        m, _, _ = A.model_apply(model, full, [model[i].id for i in full])
        A.compare(DS, m, 32, tag="reuse")


# ---- runs: wave and workgroup edges ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("run", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["erase", "insert"])
def test_runs_of_consecutive_searches(gpu, kind, run):
    model = A.base(600, 14)
    with make(model, 14) as DS:
        if kind == "erase":
            m = A.apply(DS, model, erase=range(171, 171 + run))
        else:
            m = A.apply(DS, model, ins=A.free_between(model, 171, run))
        A.compare(DS, m, 14, tag=f"{kind} {run}")


# ---- the lookup forms: dense keys up to 4096 searches, the prefix directory beyond ----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S0,n_erase,n_ins", [(4095, 0, 2), (4097, 2, 0), (4096, 0, 1), (4097, 1, 0), (8192, 0, 1),
                                              (8193, 1, 0)])
def test_lookup_form_edges(gpu, S0, n_erase, n_ins):
    """S' crosses 4096 (skey <-> rdx) or 8192 (B = 13 <-> 14) in one apply; the changed neighbourhood is then
    refilled, so the rebuilt structures are read by the verdicts and the new records by the refill."""
    model = A.base(S0, 14)
    at = S0 // 3
    erase = [at + 5 * k for k in range(n_erase)]
    ins = [A.free_between(model, at + 7 * k, 1)[0] for k in range(n_ins)]
    m, remap, new_index = A.model_apply(model, erase, ins)
    with A.cache_table() as NC, make(model, 14) as DS:
        A.apply(DS, model, erase, ins)
        assert DS.S == S0 - n_erase + n_ins
        A.compare(DS, m, 14, tag=f"{S0}->{DS.S}")
        which = set()
        for c in [int(i) for i in new_index] + [int(remap[e + 1]) for e in erase]:
            which |= set(range(max(c - 2, 0), min(c + 3, len(m))))
        A.refill_and_compare(DS, NC, m, which, 14, tag=f"{S0}->{DS.S}")


# ---- caps -----------------------------------------------------------------------------------------------------------
def cap_model(cap):
    """Every make_set state of this cap, with lists of exactly cap entries and empty ones among them."""
    model = A.base(67, cap)
    assert any(len(s.nodes) == cap for s in model) and any(not s.nodes for s in model)
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("cap,cap2", [(14, 14), (14, 15), (15, 16), (16, 32), (32, 33), (33, 64), (64, 65), (65, 65)])
def test_caps_with_membership_changes(gpu, cap, cap2):
    model = cap_model(cap)
    S = len(model)
    erase = [0, 1, 2, 30, 31, S - 1]
    ins = A.free_between(model, 10, 3) + [0, R.MAX_ID] + A.free_between(model, 40, 1)
    with make(model, cap, stray=True) as DS:
        ex = DS.export()
        assert (ex["node_flags"] & A.STRAY).any() and (ex["node_flags"] & 1).any() and (ex["node_flags"] & 2).any()
        m = A.apply(DS, model, erase, ins, expired=[0, 1, 0, 0, 1, 0], cap=cap2)
        A.compare(DS, m, cap2, stray=True, tag=f"{cap}->{cap2}")


@pytest.mark.gpu
def test_cap_alone(gpu):
    model = cap_model(32)
    with make(model, 32, stray=True) as DS:
        remap, new_index = DS.apply(cap=64)
        assert np.array_equal(remap, np.arange(len(model), dtype=np.uint32)) and new_index.size == 0
        A.compare(DS, model, 64, stray=True, tag="32->64")
        DS.grow(64)                                            # the cap it has: nothing to do
        A.compare(DS, model, 64, stray=True, tag="64->64")


# ---- refill after apply ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [14, 32, 64])
def test_refill_of_inserted_searches(gpu, cap):
    """The inserted searches are empty; their refill is Dht::search's (dht.cpp:1728) and equals the restatement."""
    model = A.base(300, cap)
    c = A.cache()
    ins = [c.ids[k] ^ (1 << (k % 90)) for k in range(5, 3000, 130)] + A.free_between(model, 100, 3) + [0, R.MAX_ID]
    with A.cache_table() as NC, make(model, cap) as DS:
        m, _, new_index = A.model_apply(model, ins=ins)
        A.apply(DS, model, ins=ins)
        after, status = A.refill_and_compare(DS, NC, m, new_index, cap, tag=f"cap {cap}")
        assert all(len(after[int(i)].nodes) for i in new_index) and not status.any()


@pytest.mark.gpu
def test_start_and_expire_searches(gpu):
    model = A.base(300, 32)
    c = A.cache()
    new_ids = [c.ids[k] ^ (1 << (k % 90)) for k in range(9, 3000, 170)] + [0, R.MAX_ID]
    host = A.Host(model)
    with A.cache_table() as NC, make(model, 32) as DS:
        counts = start_searches(DS, NC, host, R.id_bytes(new_ids), NOW)
        assert counts["refilled"] == len(new_ids) and counts["overflowed"] == 0 and counts["inserts"] >= len(new_ids)
        assert [host.searches[int(i)].id for i in counts["new_index"]] == new_ids
        A.compare(DS, host.searches, 32, tag="start")
        gone = np.sort(counts["new_index"])[::2]
        remap = expire_searches(DS, host, gone)
        assert (remap[gone] == A.NO_NODE).all() and (remap != A.NO_NODE).sum() == len(host.searches)
        A.compare(DS, host.searches, 32, tag="expire")


@pytest.mark.gpu
def test_overflow_then_grow_and_patch(gpu):
    """A refill reports KAD_SR_REFILL_OVERFLOW for lists that outgrow the slabs; the slabs grow on the device and only
    the overflowed searches are uploaded."""
    c = F.case("n3000_s65_cap64")
    cap, which = c["cap"], c["which"]
    ids, status = c["cache"].table_arrays()
    with DeviceTable(ids, status, device=0, index_base=c["base"], sorted=True) as NC, \
            DeviceSearches(*F.snapshot(c["searches"], NOW), cap=cap, device=0) as DS:
        _, _, _, st = DS.refill(NC, which)
        over = which[st == F.REFILL_OVERFLOW]
        assert over.size >= 1 and np.array_equal(st, c["status"])
        host = list(c["after"])  # the overflowed ones are still as before: the host runs their walk
        for s in over:
            host[int(s)] = c["searches"][int(s)].copy()
            F.refill(host[int(s)], c["cache"], NOW)
        DS.grow(2 * cap)
        DS.patch(over, *F.snapshot([host[int(s)] for s in over], NOW)[1:])
        with DeviceSearches(*F.snapshot(host, NOW), cap=2 * cap, device=0) as fresh:
            got, want = DS.export(), fresh.export()
            assert all(np.array_equal(got[k], want[k]) for k in want) and len(want) == 7
            assert DS.device_bytes == fresh.device_bytes


# ---- rejected calls and the output arrays ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_rejected_calls_in_order_leave_the_set(gpu):
    """Checks 3 to 7 of include/kadgpu.h on a live set, each call violating its check and every later one."""
    L = _lib.lib()
    model = A.base(40, 32)
    S = len(model)
    kept, other = R.id_bytes([model[5].id, 1]), R.id_bytes([2, 3])
    dup = R.id_bytes([1, 1])
    bad_flags, ok_flags = np.array([2, 1], np.uint8), np.array([0, 1], np.uint8)
    remap, new_index = np.full(S + 2, GUARD, np.uint32), np.full(4, GUARD, np.uint32)
    huge = 0x7FFFFFFF // S + 1
    with make(model, 32) as DS:
        before = DS.export()

        def call(erase, ins, fl, cap):
            e = np.array(erase, np.uint32)
            rc = L.kad_searches_apply(DS._h, p(e), e.size, p(ins), p(fl), 2, cap, p(remap[1:]), p(new_index[1:]))
            return rc, L.kad_last_error()

        def unchanged():
            after = DS.export()
            return ((remap == GUARD).all() and (new_index == GUARD).all() and
                    all(np.array_equal(before[k], after[k]) for k in before))

        for erase in ([3, 3], [4, 3], [3, S]):                                         # 3
            rc, msg = call(erase, kept, bad_flags, 31)
            assert rc == _lib.KAD_ERR_INVALID and b"strictly ascending and below S" in msg and unchanged()
        rc, msg = call([3, 4], kept, bad_flags, 31)                                    # 4
        assert rc == _lib.KAD_ERR_INVALID and b"new_cap below cap" in msg and unchanged()
        rc, msg = call([3, 4], kept, bad_flags, huge)                                  # 5
        assert rc == _lib.KAD_ERR_INVALID and b"unknown search flag" in msg and unchanged()
        for ins in (kept, dup):                                                        # 6
            rc, msg = call([3, 4], ins, ok_flags, huge)
            assert rc == _lib.KAD_ERR_INVALID and b"equal" in msg and unchanged()
        rc, msg = call([5], kept, ok_flags, 0)                                         # 6: 5 is erased, its ID is free
        assert rc == 0
        m, want_remap, want_new = A.model_apply(model, [5], [model[5].id, 1], expired=[0, 1])
        assert np.array_equal(remap[1:-1], want_remap) and np.array_equal(new_index[1:3], want_new)
        assert remap[0] == GUARD and remap[-1] == GUARD and new_index[0] == GUARD and new_index[-1] == GUARD
        DS.S, DS._ids = S + 1, A.snap(m)[0]
        A.compare(DS, m, 32, tag="re-use after the rejected calls")
        remap[:], new_index[:] = GUARD, GUARD
        before = DS.export()
        rc, msg = call([3, 4], other, ok_flags, huge)                                  # 7
        assert rc == _lib.KAD_ERR_INVALID and b"too large" in msg and unchanged()
        with pytest.raises(KadError) as e:                                             # and through the class
            DS.apply(cap=31)
        assert e.value.code == _lib.KAD_ERR_INVALID and DS.cap == 32 and DS.S == S + 1
        with pytest.raises(KadError):
            DS.apply(ins_ids=R.id_bytes([4]), ins_flags=[4])
        assert all(np.array_equal(before[k], DS.export()[k]) for k in before)


@pytest.mark.gpu
def test_outputs_sit_between_guard_words(gpu):
    L = _lib.lib()
    model = A.base(40, 32)
    S = len(model)
    erase = np.array([0, 7, 8, S - 1], np.uint32)
    ins = [0, R.MAX_ID] + A.free_between(model, 20, 2)
    want_model, want_remap, want_new = A.model_apply(model, erase, ins)
    ins_b = R.id_bytes(ins)
    for with_outputs in (True, False):
        remap, new_index = np.full(S + 2, GUARD, np.uint32), np.full(len(ins) + 2, GUARD, np.uint32)
        with make(model, 32) as DS:
            rc = L.kad_searches_apply(DS._h, p(erase), erase.size, p(ins_b), None, len(ins), 0,
                                      p(remap[1:]) if with_outputs else None,
                                      p(new_index[1:]) if with_outputs else None)
            assert rc == 0
            S2, cap = C.c_uint32(), C.c_uint32()
            assert L.kad_searches_info(DS._h, C.byref(S2), C.byref(cap), None) == 0
            assert (S2.value, cap.value) == (len(want_model), 32)
        assert remap[0] == GUARD and remap[-1] == GUARD and new_index[0] == GUARD and new_index[-1] == GUARD
        if with_outputs:
            assert np.array_equal(remap[1:-1], want_remap) and np.array_equal(new_index[1:-1], want_new)
        else:
            assert (remap == GUARD).all() and (new_index == GUARD).all()


# ---- ordering towards queries ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_queries_before_read_the_old_set_and_after_the_new(gpu):
    import torch

    model = A.base(600, 14)
    erase = list(range(100, 300, 3))
    ins = A.free_between(model, 400, 40) + [0, R.MAX_ID]
    m2, _, _ = A.model_apply(model, erase, ins)
    rng = np.random.default_rng(9)
    cands = R.id_bytes(A.candidates(model) + A.candidates(m2))
    cands = np.concatenate([cands, rng.integers(0, 256, (200_000, 20), dtype=np.uint8)])
    dev = torch.device("cuda", 0)
    d_cands = torch.from_numpy(cands).to(dev)
    with make(model, 14) as old, make(m2, 14) as new, make(model, 14) as DS:
        want_old = [t.cpu() for t in old.try_insert(d_cands)]
        want_new = [t.cpu() for t in new.try_insert(d_cands)]
        assert not torch.equal(want_old[0], want_new[0])
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            before = DS.try_insert(d_cands, stream=stream)     # enqueued, not waited for
        DS.apply(np.array(erase, np.uint32), R.id_bytes(ins))  # waits for it, then swaps the arrays and frees the old
        with torch.cuda.stream(stream):
            after = DS.try_insert(d_cands, stream=stream)
        stream.synchronize()
        for b, a, wo, wn in zip(before, after, want_old, want_new):
            assert torch.equal(b.cpu(), wo) and torch.equal(a.cpu(), wn)
