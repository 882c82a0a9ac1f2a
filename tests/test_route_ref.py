"""tests/route_ref.py against itself and against the header's words (no GPU): the packed-row layout of
include/kadgpu.h (word 0 the smallest index, one byte per entry, 0xFF past the count, KAD_ROUTE_PACKED_WORDS(count)
little-endian words, a row packs iff max - min <= 254), the owner rule and sub-block rule of kad_route_pack, the fold of
kad_route_unpack_packed_fold, and the constants the model shares with opendht_amd/_lib.py."""
import os
import re

import numpy as np
import pytest

import route_ref as R
from opendht_amd import _lib

NONE = R.NO_NODE


def test_constants_match_the_header_and_the_binding():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kadgpu.h")).read()
    for name, val in (("KAD_ROUTE_CSTRIDE", R.CSTRIDE), ("KAD_ROUTE_MAX_WORLD", R.MAX_WORLD),
                      ("KAD_ROUTE_SUBS", R.SUBS), ("KAD_ROUTE_QPW", R.QPW),
                      ("KAD_ROUTE_PACKED_MAX_COUNT", R.PACKED_MAX_COUNT),
                      ("KAD_ROUTE_PACKED", R.PACKED), ("KAD_ROUTE_KEYS", R.KEYS), ("KAD_ROUTE_ZEROED", R.ZEROED)):
        assert re.search(rf"#define {name} {val}u\b", hdr), name
        assert getattr(_lib, name) == val, name
    assert "#define KAD_ROUTE_PACKED_WORDS(count) (1u + ((count) + 3u) / 4u)" in hdr
    assert "#define KAD_ROUTE_CTR_WORDS(world) (((world) * KAD_ROUTE_SUBS + 1u) * KAD_ROUTE_CSTRIDE)" in hdr
    assert "#define KAD_ROUTE_OVERFLOW_WORD(world) ((world) * KAD_ROUTE_SUBS * KAD_ROUTE_CSTRIDE)" in hdr
    for w in (1, 3, 16):
        assert R.ctr_words(w) == _lib.route_ctr_words(w) and R.overflow_word(w) == _lib.route_overflow_word(w)
    for c in range(1, 33):
        assert R.packed_words(c) == _lib.route_packed_words(c)
    assert R.packed_words(8) * 4 == 12  # "count 8: 12 bytes instead of 33"
    assert _lib.KAD_NO_NODE == NONE


def test_hand_worked_count8_row():
    """Five entries of a count-8 row, the smallest not first, the largest exactly 254 above it: 12 bytes."""
    row = np.array([1003, 1000, 1254, 1001, 1002, 7, 7, 7], np.uint32)  # (entries past cnt = 5 are not the row's)
    words = R.pack_row(row, 5, 8)
    assert words.dtype == np.uint32 and words.tolist() == [1000, 0x01FE0003, 0xFFFFFF02]
    assert words.astype("<u4").tobytes() == bytes([0xE8, 0x03, 0, 0, 3, 0, 0xFE, 1, 2, 0xFF, 0xFF, 0xFF])
    got, cnt = R.decode_row(words, 8)
    assert cnt == 5 and got.tolist() == [1003, 1000, 1254, 1001, 1002, NONE, NONE, NONE]
    assert not R.escapes(row, 5) and R.escapes(np.array([1000, 1255] + [0] * 6, np.uint32), 2)
    assert not R.escapes(np.array([0, 10 ** 6] + [0] * 6, np.uint32), 1)  # one entry: the second is not the row's
    assert not R.escapes(row, 0)
    # an empty row: word 0 KAD_NO_NODE, every byte 0xFF
    assert R.pack_row(row, 0, 8).tolist() == [NONE, NONE, NONE]
    assert R.decode_row([NONE, NONE, NONE], 8)[1] == 0
    # a base below the minimum decodes to the same row (the fused query kernel's "base no larger than any entry")
    got2, cnt2 = R.decode_row([990, 0x0BFF0A0D, 0xFFFFFFFF], 8)
    assert cnt2 == 3 and got2.tolist() == [1003, 1000, NONE, 1001, NONE, NONE, NONE, NONE]
    # the largest index a table can hold
    top = np.array([0xFFFFFFFE, 0xFFFFFFFE - 254], np.uint32)
    assert R.pack_row(top, 2, 2).tolist() == [0xFFFFFFFE - 254, 0xFFFF00FE]
    assert R.decode_row(R.pack_row(top, 2, 2), 2)[0].tolist() == top.tolist()


@pytest.mark.parametrize("count", range(1, 33))
def test_decode_inverts_pack(count):
    rows, cnt = R.synth_rows(count)
    assert rows.shape == (600, count) and set(cnt.tolist()) == set(range(count + 1))
    live = np.arange(count)[None, :] < cnt[:, None]
    esc = R.escapes_rows(rows, cnt)
    span = np.where(live, rows.astype(np.int64), -1).max(1) - np.where(live, rows.astype(np.int64), 1 << 40).min(1)
    if count > 1:  # both sides of the edge, and the extreme entry at the first, a middle and the last place
        assert {253, 254, 255, 256} <= set(span[cnt > 1].tolist())
        assert esc.any() and (~esc).any() and np.array_equal(esc, (cnt > 0) & (span > 254))
        hi_at, last = np.where(live, rows, 0).argmax(1)[cnt > 2], cnt[cnt > 2] - 1
        assert count == 2 or ((hi_at == 0).any() and (hi_at == last).any() and ((hi_at > 0) & (hi_at < last)).any())
        assert rows[live].max() == 0xFFFFFFFE and rows[live].min() == 0
    packed = R.pack_rows(rows, cnt, count)
    assert packed.shape == (600, R.packed_words(count)) and packed.dtype == np.uint32
    got, gcnt = R.decode_rows(packed[~esc], count)
    np.testing.assert_array_equal(gcnt, cnt[~esc])
    np.testing.assert_array_equal(got, np.where(live, rows, NONE)[~esc])
    for i in np.nonzero(~esc)[0][:40]:  # the one-row forms agree with the batched ones
        np.testing.assert_array_equal(R.pack_row(rows[i], int(cnt[i]), count), packed[i])
        r1, c1 = R.decode_row(packed[i], count)
        assert c1 == cnt[i] and np.array_equal(r1, np.where(live[i], rows[i], NONE))
        assert R.escapes(rows[i], int(cnt[i])) is False
    np.testing.assert_array_equal(packed[cnt == 0], NONE)


def test_owner_and_sub_blocks():
    t = np.zeros((3000, 20), np.uint8)
    t[:, 0] = np.arange(3000) % 256
    assert R.owner(t, 5, 0).tolist() == [0] * 3000
    np.testing.assert_array_equal(R.owner(t, 4, 2), t[:, 0] >> 6)
    np.testing.assert_array_equal(R.owner(t, 3, 2), (t[:, 0] >> 6) % 3)  # the `% world` arm: owner 3 wraps to 0
    np.testing.assert_array_equal(R.owner(t, 16, 8), t[:, 0] % 16)
    e = R.expect_pack(t, 3, 2, 8 * 300)
    assert e["ctr"].sum() == 3000 and e["ctr"][:, 3:].sum() == 0  # workgroups 0..2 -> sub-blocks 0..2
    assert e["ctr"][:, 0].sum() == 1024 and e["ctr"][:, 2].sum() == 3000 - 2048
    assert e["overflow"] == 1 and (e["placed"] <= 300).all() and e["placed"][0, 0] == 300  # owner 0 has half of them
    assert R.expect_pack(t, 3, 2, 8 * 512)["overflow"] == 0
    for d in range(3):
        for r in range(8):
            assert e["queries"][d][r].size == e["ctr"][d, r]
    assert sorted(np.concatenate([x for row in e["queries"] for x in row]).tolist()) == list(range(3000))
    assert R.expect_pack(t[:1], 1, 0, 8)["overflow"] == 0 and R.expect_pack(t[:2], 1, 0, 8)["overflow"] == 1


def test_fold_model():
    c = R.ctr_image(np.arange(24), 3, overflow=1, tail=1)
    assert c.size == R.ctr_words(3) and c[23 * 32] == 23 and c[R.overflow_word(3)] == 1
    assert R.expect_fold(c, 3, [0, 0, 0, 0]).tolist() == [1, 0, 1, 8 * 23]
    assert R.expect_fold(c, 3, [0, 1, 0, 1000]).tolist() == [1, 1, 1, 1000]
    assert R.expect_fold(np.zeros(R.ctr_words(1), np.uint32), 1, [0, 0, 0, 0]).tolist() == [0, 0, 0, 0]
