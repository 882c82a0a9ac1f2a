"""kad_search_step / kad_search_step_batch (the closed form of opendht_amd/csrc/kad_step.h, the function step_kernel
calls) against step_ref's entry-by-entry loops: every list of up to three entries over all 64 values of
the six flag bits, in both search states and every mode; random lists at the lengths where a count crosses 8, 14, 25,
a word or the 64-bit plane; and the named cases, whose expected answers are also written out by hand here. CPU only."""
import itertools

import numpy as np
import pytest

import step_ref as T
from opendht_amd import _lib, search_step, search_step_batch


def run_batch(lists, expired, mode):
    fl, n = T.pad(lists)
    want = T.step_batch(fl, n, np.full(len(lists), expired), np.full(len(lists), mode))
    off = np.zeros(len(lists) + 1, np.uint32)
    off[1:] = np.cumsum(n)
    flat = np.array([v for x in lists for v in x], np.uint8)
    got = search_step_batch(off, flat, np.full(len(lists), 1 if expired else 0, np.uint8), np.full(len(lists), mode, np.uint8))
    T.assert_step(got, want[:6], (expired, mode))
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_every_short_list(n):
    lists = [list(x) for x in itertools.product(range(64), repeat=n)]
    fl, ln = T.pad(lists)
    off = np.arange(len(lists) + 1, dtype=np.uint32) * n
    flat = fl[:, :n].reshape(-1) if n else np.zeros(0, np.uint8)
    for expired in (False, True):
        for mode in T.MODES:
            want = T.step_batch(fl, ln, np.full(len(lists), expired), np.full(len(lists), mode))
            got = search_step_batch(off, flat, np.full(len(lists), int(expired), np.uint8),
                                    np.full(len(lists), mode, np.uint8))
            T.assert_step(got, want[:6], (n, expired, mode))


@pytest.mark.parametrize("n", T.RANDOM_N)
def test_random_lists(n):
    lists = T.random_lists(np.random.default_rng(100 + n), n, 200)
    seen = 0
    for expired in (False, True):
        for mode in T.MODES:
            seen |= int(np.bitwise_or.reduce(run_batch(lists, expired, mode)[5]))
    if n >= 1:
        assert seen == 0x3F, hex(seen)  # every result bit occurs at every length


@pytest.mark.parametrize("name", list(T.NAMED))
def test_named_case(name):
    fl, expired, mode = T.NAMED[name]
    want = T.step(fl, expired, mode)
    got = search_step(fl, 1 if expired else 0, mode)
    assert [e for e in range(64) if (got["picks"] >> e) & 1] == want[0]
    assert (got["n"], got["bad"], got["lead_bad"], got["solicited"], got["bits"]) == want[1:6]
    # APPLY and NO_EXPIRE change what is written, never the answer
    assert search_step(fl, 1 if expired else 0, mode | T.APPLY | T.NO_EXPIRE) == got


def test_named_cases_by_hand():
    """The answers the issue spells out, independent of both implementations."""
    S = T.step
    assert S(*T.NAMED["solicited_4"])[:6] == ([], 10, 0, 0, 4, T.SHORT)
    assert S(*T.NAMED["solicited_5"])[:6] == ([], 11, 0, 0, 5, T.SHORT)
    assert S(*T.NAMED["solicited_3_and_one_bad"])[:6] == ([4], 6, 1, 0, 4, T.SHORT)
    assert S(*T.NAMED["room_th_pick_is_last"])[:6] == ([3, 6], 7, 0, 0, 4, T.SHORT)
    assert S(*T.NAMED["room_th_pick_is_last_of_64"])[0] == [61, 62, 63]
    assert S(*T.NAMED["candidates_around_the_picks"])[:6] == ([0, 1, 2, 3, 4, 5, 6], 9, 4, 1, 4, T.SHORT)
    assert S(*T.NAMED["candidates_then_exhausted"])[:6] == ([0, 1, 2, 3, 4], 5, 3, 1, 2, T.SHORT | T.EXHAUSTED)
    assert S(*T.NAMED["candidates_only"])[:6] == ([0, 1, 2, 3, 4, 5], 6, 6, 6, 0, T.SHORT | T.EXHAUSTED | T.EXPIRE)
    assert S(*T.NAMED["expired_candidate_with_noget"])[0] == [1, 2]
    assert S(*T.NAMED["expired_candidate_without_noget"])[0] == [0, 1, 2]
    assert not S(*T.NAMED["eighth_unsynced"])[5] & T.SYNCED
    assert S(*T.NAMED["ninth_unsynced"])[5] & T.SYNCED
    assert S(*T.NAMED["synced_by_fewer_than_eight"])[:6] == ([], 5, 2, 0, 0, T.SHORT | T.SYNCED | T.EXHAUSTED)
    assert not S(*T.NAMED["bad_synced_does_not_count"])[5] & T.SYNCED
    assert S(*T.NAMED["only_bad"])[:6] == ([], 10, 10, 10, 0, T.SHORT | T.EXHAUSTED | T.EXPIRE)
    assert S(*T.NAMED["empty_live"])[:6] == ([], 0, 0, 0, 0, T.SHORT | T.EXHAUSTED | T.EXPIRE)
    assert S(*T.NAMED["empty_expired"])[:6] == ([], 0, 0, 0, 0, T.SKIPPED)
    assert S(*T.NAMED["expired_search"])[:6] == ([], 4, 1, 0, 1, T.SKIPPED)
    for n in (25, 26, 64):
        assert not S(*T.NAMED[f"lead_24_of_{n}"])[5] & T.EXPIRE
        assert S(*T.NAMED[f"lead_25_of_{n}"])[5] & T.EXPIRE
    assert S(*T.NAMED["lead_is_n_below_25"])[5] & T.EXPIRE and not S(*T.NAMED["lead_one_short_of_n"])[5] & T.EXPIRE
    assert S(*T.NAMED["done_if_synced_synced"])[:6] == ([], 9, 0, 0, 0, T.SHORT | T.SYNCED | T.DONE)
    assert S(*T.NAMED["done_if_synced_unsynced"])[:6] == ([3, 4, 5, 6], 9, 0, 0, 4, T.SHORT)
    assert S(*T.NAMED["done_and_expiring"])[5] == T.SHORT | T.SYNCED | T.DONE | T.EXPIRE
    assert S(*T.NAMED["no_send"])[:6] == ([], 9, 0, 0, 0, T.SHORT)
    assert S(*T.NAMED["no_send_expiring"])[5] == T.SHORT | T.EXPIRE


def test_step_rejects_what_it_cannot_hold():
    L = _lib.lib()
    out = np.zeros(1, _lib.STEP_OUT_DTYPE)
    fl = np.zeros(65, np.uint8)
    p = _lib.ptr
    assert L.kad_search_step(65, p(fl), 0, 0, p(out)) == _lib.KAD_ERR_INVALID
    assert L.kad_search_step(64, p(fl), 0, 0, p(out)) == 0
    assert L.kad_search_step(3, None, 0, 0, p(out)) == _lib.KAD_ERR_INVALID
    assert L.kad_search_step(0, None, 0, 0, None) == _lib.KAD_ERR_INVALID
    assert L.kad_search_step(0, None, 0, 0x10, p(out)) == _lib.KAD_ERR_INVALID
    assert L.kad_search_step(0, None, 0, 0x0F, p(out)) == 0
