"""kad_search_step_full / kad_search_step_full_batch (kadstep::decide_full of opendht_amd/csrc/kad_step.h, the function
step_full_kernel calls) against stepfull_ref's entry-by-entry loops: every list of up to two entries
over all 256 byte values, in both search states and every valid mode; random lists over all eight bits at the lengths
where a count crosses 4, 8, 14, 25, a word or the 64-bit plane; every mode without LISTEN and ANNOUNCE against
kad_search_step_batch field for field; the named cases with their answers written out by hand; the invalid modes.
CPU only."""
import itertools

import numpy as np
import pytest

import step_ref as T
import stepfull_ref as F
from opendht_amd import _lib, search_step_batch, search_step_full, search_step_full_batch


def csr(lists):
    n = np.array([len(x) for x in lists], np.int64)
    off = np.zeros(len(lists) + 1, np.uint32)
    off[1:] = np.cumsum(n)
    return off, np.array([v for x in lists for v in x], np.uint8)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_every_short_list(n):
    N = 256 ** n
    lists = np.array(list(itertools.product(range(256), repeat=n)), np.uint8).reshape(N, n)
    fl = np.zeros((N, n + 1), np.uint8)
    fl[:, :n] = lists
    ln = np.full(N, n, np.int64)
    off = np.arange(N + 1, dtype=np.uint32) * n
    flat = np.ascontiguousarray(lists).reshape(-1)
    for expired in (False, True):
        for mode in F.MODES:
            want = F.step_full_batch(fl, ln, np.full(N, expired), np.full(N, mode))
            got = search_step_full_batch(off, flat, np.full(N, int(expired), np.uint8), np.full(N, mode, np.uint8))
            F.assert_step_full(got, want[:8], (n, expired, mode))


@pytest.mark.parametrize("n", F.RANDOM_N)
def test_random_lists(n):
    lists = F.random_lists(np.random.default_rng(200 + n), n, 200)
    fl, ln = T.pad(lists)
    off, flat = csr(lists)
    N = len(lists)
    seen, sent = 0, [0, 0]
    for expired in (False, True):
        for mode in F.MODES:
            want = F.step_full_batch(fl, ln, np.full(N, expired), np.full(N, mode))
            got = search_step_full_batch(off, flat, np.full(N, int(expired), np.uint8), np.full(N, mode, np.uint8))
            F.assert_step_full(got, want[:8], (n, expired, mode))
            seen |= int(np.bitwise_or.reduce(want[7])) if N else 0
            sent[0] += int((want[1] != 0).sum())
            sent[1] += int((want[2] != 0).sum())
    if n >= 1:
        assert seen == 0x3F, hex(seen)
        assert sent[0] and sent[1]  # both loops send at every length


def test_old_modes_equal_kad_search_step():
    """A mode without LISTEN and ANNOUNCE: kad_search_step_batch's picks, counts and bits, and zero masks, whatever the
    due bits say."""
    for n in (0, 1, 5, 9, 17, 33, 64):
        lists = F.random_lists(np.random.default_rng(300 + n), n, 120)
        off, flat = csr(lists)
        N = len(lists)
        for expired in (0, 1):
            for mode in F.OLD_MODES:
                sf, md = np.full(N, expired, np.uint8), np.full(N, mode, np.uint8)
                got, old = search_step_full_batch(off, flat, sf, md), search_step_batch(off, flat, sf, md)
                for k in ("picks", "n", "bad", "lead_bad", "solicited", "bits"):
                    assert np.array_equal(got[k], old[k]), (n, expired, mode, k)
                assert not got["listen"].any() and not got["announce"].any()


@pytest.mark.parametrize("name", list(F.NAMED))
def test_named_case(name):
    fl, expired, mode = F.NAMED[name]
    want = F.step_full(fl, expired, mode)
    got = search_step_full(fl, 1 if expired else 0, mode)
    assert (F.positions(got["picks"]), F.positions(got["listen"]), F.positions(got["announce"])) == want[:3]
    assert (got["n"], got["bad"], got["lead_bad"], got["solicited"], got["bits"]) == want[3:8]
    # APPLY and NO_EXPIRE change what is written, never the answer
    assert search_step_full(fl, 1 if expired else 0, mode | F.APPLY | F.NO_EXPIRE) == got


def test_named_cases_by_hand():
    """The answers the issue spells out, independent of both implementations, asked of both."""

    def both(name):
        fl, expired, mode = F.NAMED[name]
        w = F.step_full(fl, expired, mode)
        g = search_step_full(fl, 1 if expired else 0, mode)
        assert (F.positions(g["picks"]), F.positions(g["listen"]), F.positions(g["announce"]), g["solicited"],
                g["bits"]) == (w[0], w[1], w[2], w[6], w[7]), name
        return w

    assert both("listen_first_four")[1] == [0, 1, 2, 3]
    assert both("listen_candidates_do_not_count")[1] == [0, 1, 2, 3, 4, 5]
    assert both("listen_not_due_counts")[1] == [0, 1, 2]  # the not-due entry 3 was the fourth
    # entries 1 and 3 carry LISTEN_DUE without SYNCED: never picked, not counted, so the walk reaches entry 5
    assert both("listen_unsynced_entry")[1] == [0, 2, 4, 5]
    assert both("announce_not_due_does_not_count")[2] == [2, 3, 4, 5, 6, 7, 8, 9]  # listen would have stopped at 3
    assert both("announce_ninth_not_picked")[2] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert both("announce_candidate_adds_a_ninth")[2] == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    w = both("unsynced_search_with_due_bits")
    fl = F.NAMED["unsynced_search_with_due_bits"][0]
    assert w[1] == [] and w[2] == [] and not w[7] & T.SYNCED and w[0] == T.step(fl, False, 0)[0] == [0, 1, 2, 3]
    w = both("two_pending_two_probes")
    assert (w[0], w[2], w[6]) == ([], [2, 3], 4)
    w = both("probe_on_pending_entry")
    assert (w[0], w[2], w[6]) == ([], [0], 1) and w[7] & T.EXHAUSTED
    w = both("probe_without_blocks_is_a_get_pick")
    assert (w[0], w[2], w[6]) == ([0], [0], 1)
    w = both("probe_with_blocks_is_no_get_pick")
    assert (w[0], w[2], w[6]) == ([], [0], 1)
    w = both("expired_search_with_due_bits")
    assert w[:3] == ([], [], []) and w[7] == T.SKIPPED
    w = both("both_loops_and_gets")  # listen counts 0, 1, 2 and 4 (3 is a candidate); announce has three due
    assert (w[1], w[2]) == ([0, 1, 3], [0, 2, 3])
    # the probes on 0 and 2 are pending (3 is BAD): room for two more, which are 1 and 4; the gettable entries up to 4
    # are picked, the probed ones included, as their get query is not the probe's
    assert w[0] == [0, 1, 2, 3, 4] and w[6] == 4
    w = both("due_bits_without_their_mode")
    assert (w[1], w[2]) == ([], []) and w[0] == [0, 1, 2, 3]
    w = both("expiring_with_sends")
    assert w[7] & T.EXPIRE and w[1] == [25, 26, 27] and w[2] == [25, 26, 27]
    assert both("listen_in_every_unit_of_64")[1] == [e for e in range(64) if e not in (15, 32, 48)]
    assert both("announce_in_every_unit_of_64")[2] == [e for e in range(64) if not 22 <= e < 34]


def test_invalid_modes_are_refused():
    L, p = _lib.lib(), _lib.ptr
    out = np.zeros(2, _lib.STEP_FULL_OUT_DTYPE)
    fl = np.zeros(65, np.uint8)
    assert len(F.MODES) == 56 and len(F.INVALID_MODES) == 200
    for mode in F.INVALID_MODES:
        assert L.kad_search_step_full(3, p(fl), 0, mode, p(out)) == _lib.KAD_ERR_INVALID, mode
        assert L.kad_search_step_full_batch(2, p(np.array([0, 1, 2], np.uint32)), p(fl), None,
                                            p(np.array([0, mode], np.uint8)), p(out)) == _lib.KAD_ERR_INVALID, mode
    for mode in F.MODES:
        assert L.kad_search_step_full(3, p(fl), 0, mode, p(out)) == 0, mode
    for mode in (F.DONE_IF_SYNCED | F.LISTEN, F.DONE_IF_SYNCED | F.ANNOUNCE, F.PROBE_BLOCKS, F.PROBE_BLOCKS | F.LISTEN, 0x80):
        assert mode in F.INVALID_MODES
    assert L.kad_search_step_full(65, p(fl), 0, 0, p(out)) == _lib.KAD_ERR_INVALID
    assert L.kad_search_step_full(64, p(fl), 0, 0, p(out)) == 0
    assert L.kad_search_step_full(3, None, 0, 0, p(out)) == _lib.KAD_ERR_INVALID
    assert L.kad_search_step_full(0, None, 0, 0, None) == _lib.KAD_ERR_INVALID
    # the old calls still refuse the new modes
    assert L.kad_search_step(0, None, 0, F.LISTEN, p(np.zeros(1, _lib.STEP_OUT_DTYPE))) == _lib.KAD_ERR_INVALID
