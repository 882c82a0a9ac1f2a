"""The routing primitives of csrc/kad_route.hip called directly through the C ABI and compared with
tests/route_ref.py, the numpy model of include/kadgpu.h: kad_route_pack / _pack_keys / _pack_ex, kad_route_unpack,
kad_route_compress, kad_route_unpack_packed, kad_route_unpack_packed_fold and kad_route_fold_flags. No driver
(OwnerRoute, serve_owner, kad_route_run) stands between a kernel and the assertion, so nothing answers a batch again.

Every count 1..32 is launched with 16-byte aligned buffers and from views one word further on, so that the vector
kernels (compress4<G>, unpack_packed4<G>, unpack<true>) and the scalar ones both run at the counts that are multiples
of 4; kad_route_pack runs at worlds that are not powers of two, at world 16 and at shard_bits 0. Every output lies
between guard words that must survive the call."""
import ctypes as C
import math

import numpy as np
import pytest

import route_ref as R
from opendht_amd import _lib

p = _lib.ptr
NONE, SUBS = R.NO_NODE, R.SUBS
GUARD = 0xA5
INVALID = _lib.KAD_ERR_INVALID


# ---- argument checks: before any device call, so they need no GPU --------------------------------------------------
def test_pack_argument_checks():
    L = _lib.lib()
    t = np.zeros((8, 20), np.uint8)
    send = np.full(16 * 64 * 20 + 8, GUARD, np.uint8)
    slot = np.full(8, 0xA5A5A5A5, np.uint32)
    ctr = np.full(R.ctr_words(16), 0xA5A5A5A5, np.uint32)
    assert send.ctypes.data % 8 == 0

    def forms(q, world, bits, cap, tp=p(t), sp=p(send), slp=p(slot), cp=p(ctr)):
        yield L.kad_route_pack(tp, q, world, bits, cap, sp, slp, cp, 0, None)
        yield L.kad_route_pack_keys(tp, q, world, bits, cap, sp, slp, cp, 0, None)
        for mode in (0, R.KEYS, R.ZEROED, R.KEYS | R.ZEROED):
            yield L.kad_route_pack_ex(tp, q, world, bits, cap, sp, slp, cp, mode, 0, None)

    def off(a, n):
        return C.c_void_p(a.ctypes.data + n)

    bad = [dict(world=0), dict(world=17), dict(bits=9), dict(cap=0), dict(cap=12), dict(cap=4),
           dict(world=2, cap=0x80000000), dict(world=16, cap=0x10000000), dict(world=3, cap=0x55555558),
           dict(cp=None), dict(tp=None), dict(sp=None), dict(slp=None),
           dict(tp=off(t, 1)), dict(tp=off(t, 2)), dict(sp=off(send, 2)), dict(slp=off(slot, 1)), dict(cp=off(ctr, 2))]
    for kw in bad:
        a = dict(q=8, world=4, bits=2, cap=64)
        a.update(kw)
        for q in (8, 0) if set(kw) & {"world", "bits", "cap", "cp"} else (8,):  # the shape is checked at q = 0 too
            a["q"] = q
            assert list(forms(**a)) == [INVALID] * 6, (kw, q)
    # 8-byte keys: send_keys aligned to 8, not only to 4
    assert L.kad_route_pack_keys(p(t), 8, 4, 2, 64, off(send, 4), p(slot), p(ctr), 0, None) == INVALID
    assert b"8-byte aligned" in L.kad_last_error()
    for mode in (R.KEYS, R.KEYS | R.ZEROED):
        assert L.kad_route_pack_ex(p(t), 8, 4, 2, 64, off(send, 4), p(slot), p(ctr), mode, 0, None) == INVALID
    # mode: KAD_ROUTE_KEYS and KAD_ROUTE_ZEROED alone (KAD_ROUTE_PACKED is kad_route_run's)
    for mode in (R.PACKED, 8, 16, 0x80000000, R.KEYS | 8, 0xFFFFFFFF):
        assert L.kad_route_pack_ex(p(t), 8, 4, 2, 64, p(send), p(slot), p(ctr), mode, 0, None) == INVALID
        assert b"mode" in L.kad_last_error()
    assert (send == GUARD).all() and (slot == 0xA5A5A5A5).all() and (ctr == 0xA5A5A5A5).all()


def test_packed_row_argument_checks():
    L = _lib.lib()
    w = np.full(64, 0xA5A5A5A5, np.uint32)
    b = np.full(64, GUARD, np.uint8)
    for count in (0, 33, 64, 0xFFFFFFFF):
        for n in (4, 0):
            assert L.kad_route_compress(p(w), p(b), n, count, p(w), p(w), 0, None) == INVALID
            assert L.kad_route_unpack_packed(p(w), n, count, p(w), p(w), p(b), 0, None) == INVALID
            assert L.kad_route_unpack_packed_fold(p(w), n, count, p(w), p(w), p(b), p(w), 1, p(w), 0, None) == INVALID
        assert b"count" in L.kad_last_error()
    for a in ((None, p(b), p(w), p(w)), (p(w), None, p(w), p(w)), (p(w), p(b), None, p(w)), (p(w), p(b), p(w), None)):
        assert L.kad_route_compress(a[0], a[1], 4, 8, a[2], a[3], 0, None) == INVALID
    for a in ((None, p(w), p(w), p(b)), (p(w), None, p(w), p(b)), (p(w), p(w), None, p(b)), (p(w), p(w), p(w), None)):
        assert L.kad_route_unpack_packed(a[0], 4, 8, a[1], a[2], a[3], 0, None) == INVALID
        assert L.kad_route_unpack_packed_fold(a[0], 4, 8, a[1], a[2], a[3], p(w), 1, p(w), 0, None) == INVALID
    for world, ctr, flags in ((0, p(w), p(w)), (17, p(w), p(w)), (1, None, p(w)), (1, p(w), None)):
        for q in (4, 0):  # (q = 0 is the fold and reset alone: its arguments are checked all the same)
            assert L.kad_route_unpack_packed_fold(p(w), q, 8, p(w), p(w), p(b), ctr, world, flags, 0, None) == INVALID
        if ctr is None or flags is None:
            assert L.kad_route_fold_flags(ctr, world, flags, 0, None) == INVALID
        else:
            assert L.kad_route_fold_flags(p(w), world, p(w), 0, None) == INVALID
    for a in ((None, p(b), p(b)), (p(w), None, p(b)), (p(w), p(b), None)):
        assert L.kad_route_unpack(a[0], 4, 0, None, a[1], None, a[2], 0, None) == INVALID
    assert L.kad_route_unpack(p(w), 4, 8, None, p(b), p(w), p(b), 0, None) == INVALID
    assert L.kad_route_unpack(p(w), 4, 8, p(w), p(b), None, p(b), 0, None) == INVALID
    # nothing to do: KAD_OK without touching a device
    assert L.kad_route_compress(None, None, 0, 8, None, None, 0, None) == 0
    assert L.kad_route_unpack_packed(None, 0, 8, None, None, None, 0, None) == 0
    assert L.kad_route_unpack(None, 0, 8, None, None, None, None, 0, None) == 0
    assert (w == 0xA5A5A5A5).all() and (b == GUARD).all()


# ---- device buffers between guards ---------------------------------------------------------------------------------
class Buf:
    """A device byte buffer whose payload starts `shift` words after a 256-byte aligned address (shift 0: 16-byte
    aligned; shift 1: 4-byte aligned only), with guard bytes on both sides."""

    def __init__(self, gpu, data=None, nbytes=None, shift=0, fill=GUARD):
        import torch

        raw = None if data is None else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.n = raw.size if raw is not None else nbytes
        self.lo = 64 + 4 * shift
        self.t = torch.full((self.lo + self.n + 64,), GUARD, dtype=torch.uint8, device=gpu)
        assert self.t.data_ptr() % 256 == 0
        if raw is not None and raw.size:
            self.t[self.lo:self.lo + self.n] = torch.from_numpy(raw.copy()).to(gpu)
        elif fill != GUARD and self.n:
            self.t[self.lo:self.lo + self.n] = fill

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.lo)

    def get(self, dtype=np.uint32, nbytes=None):
        """The payload (its first nbytes); the bytes around it (and after nbytes) must still be the guard."""
        h = self.t.cpu().numpy()
        n = self.n if nbytes is None else nbytes
        assert (h[:self.lo] == GUARD).all() and (h[self.lo + n:] == GUARD).all(), "a kernel wrote outside its output"
        return h[self.lo:self.lo + n].copy().view(dtype)


def _sync():
    import torch

    torch.cuda.synchronize()


def _slots(n_rows_ok, q, rng):
    """q places among the given rows, about every tenth KAD_NO_NODE (the second always, when q allows)."""
    s = rng.choice(n_rows_ok, q, replace=q > n_rows_ok.size).astype(np.uint32)
    s[rng.random(q) < 0.1] = NONE
    if q > 2:
        s[1] = NONE
    return s


# ---- kad_route_compress / kad_route_unpack_packed ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("count", range(1, 33))
def test_compress_and_unpack_packed(gpu, count, shift):
    L = _lib.lib()
    rows, cnt = R.synth_rows(count)
    W = R.packed_words(count)
    esc = R.escapes_rows(rows, cnt)
    model = R.pack_rows(rows, cnt, count)
    full = np.where(np.arange(count)[None, :] < cnt[:, None], rows, NONE).astype(np.uint32)
    rng = np.random.default_rng(count)
    d_rows, d_cnt = Buf(gpu, rows, shift=shift), Buf(gpu, cnt)
    assert d_rows.ptr.value % 16 == 4 * shift
    for n in (600, 1, 255, 256, 257):
        out, escape = Buf(gpu, nbytes=4 * n * W, shift=shift), Buf(gpu, np.zeros(1, np.uint32))
        # a batch of rows that all pack leaves escape as it was (0, or 1 from an earlier batch); one with a row that
        # does not sets it
        ok = np.nonzero(~esc[:n])[0]
        clean, clean_cnt = Buf(gpu, rows[ok], shift=shift), Buf(gpu, cnt[ok])
        for e0 in (0, 1):
            e = Buf(gpu, np.full(1, e0, np.uint32))
            o = Buf(gpu, nbytes=4 * ok.size * W, shift=shift)
            _lib.check(L.kad_route_compress(clean.ptr, clean_cnt.ptr, ok.size, count, o.ptr, e.ptr, 0, None), "clean")
            _sync()
            assert e.get()[0] == e0, f"count {count} n {n}: escape {e0} -> {e.get()[0]} on rows that pack"
            np.testing.assert_array_equal(o.get().reshape(-1, W), model[ok], err_msg=f"count {count} n {n} clean")
        _lib.check(L.kad_route_compress(d_rows.ptr, d_cnt.ptr, n, count, out.ptr, escape.ptr, 0, None), "compress")
        _sync()
        got = out.get().reshape(n, W)
        np.testing.assert_array_equal(got[~esc[:n]], model[:n][~esc[:n]], err_msg=f"count {count} n {n}")
        assert (escape.get()[0] != 0) == bool(esc[:n].any()), f"count {count} n {n}: escape"
        # the way back: q places into the n packed rows (only rows that pack are ever read back), some KAD_NO_NODE
        for q in (n, 1) if n == 600 else (n,):
            if ok.size == 0:
                continue
            slot = _slots(ok, q, rng)
            want, wcnt = R.unpack_rows(slot, full[:n], cnt[:n], count)
            d_slot, o_idx, o_cnt = Buf(gpu, slot), Buf(gpu, nbytes=4 * q * count, shift=shift), Buf(gpu, nbytes=q)
            _lib.check(L.kad_route_unpack_packed(d_slot.ptr, q, count, out.ptr, o_idx.ptr, o_cnt.ptr, 0, None),
                       "unpack_packed")
            _sync()
            np.testing.assert_array_equal(o_cnt.get(np.uint8), wcnt, err_msg=f"count {count} n {n} q {q} counts")
            np.testing.assert_array_equal(o_idx.get().reshape(q, count), want, err_msg=f"count {count} n {n} q {q}")
    if count == 1:
        return
    # the edge alone: batches whose only rows that cannot be packed span exactly 255 (the batches above also hold
    # spans of 256 and 10^6, which would set the word for them), and batches of one such row, the extreme entry at
    # each of its three places
    span = R.spans_rows(rows, cnt)
    at255, ok = np.nonzero(span == 255)[0], np.nonzero(~esc)[0]
    assert at255.size >= 3 and esc[at255].all() and (span[ok] <= 254).all() and (span[ok] == 254).any()
    one = [at255[at255 % 3 == k][:1] for k in range(3)]
    for sel in [np.concatenate([ok, at255]), np.concatenate([at255[:1], ok])] + [s for s in one if s.size]:
        d_r, d_c, e = Buf(gpu, rows[sel], shift=shift), Buf(gpu, cnt[sel]), Buf(gpu, np.zeros(1, np.uint32))
        o = Buf(gpu, nbytes=4 * sel.size * W, shift=shift)
        _lib.check(L.kad_route_compress(d_r.ptr, d_c.ptr, sel.size, count, o.ptr, e.ptr, 0, None), "compress")
        _sync()
        assert e.get()[0] != 0, f"count {count}: a row spanning 255 did not set escape ({sel.size} rows)"
        keep = ~esc[sel]
        np.testing.assert_array_equal(o.get().reshape(-1, W)[keep], model[sel][keep], err_msg=f"count {count} span 255")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("count", [0, 1, 4, 7, 8, 14, 32])
def test_unpack_plain(gpu, count, shift):
    L = _lib.lib()
    rng = np.random.default_rng(100 + count)
    nb = 300
    back = rng.integers(0, 1 << 32, (nb, max(count, 1)), dtype=np.uint32)[:, :count]
    bcnt = rng.integers(0, count + 1, nb).astype(np.uint8)
    d_back, d_bcnt = Buf(gpu, back, shift=shift), Buf(gpu, bcnt)
    for q in (1, 257, 600):
        slot = _slots(np.arange(nb), q, rng)
        if q == 1:
            slot[0] = nb - 1
        want, wcnt = R.unpack_rows(slot, back, bcnt, count)
        d_slot = Buf(gpu, slot)
        for out_shift in (shift, 1 - shift) if count % 4 == 0 and count else (shift,):  # either side unaligned
            o_idx, o_cnt = Buf(gpu, nbytes=4 * q * count, shift=out_shift), Buf(gpu, nbytes=q)
            _lib.check(L.kad_route_unpack(d_slot.ptr, q, count, d_back.ptr, d_bcnt.ptr, o_idx.ptr, o_cnt.ptr, 0, None),
                       "unpack")
            _sync()
            np.testing.assert_array_equal(o_cnt.get(np.uint8), wcnt, err_msg=f"count {count} q {q} counts")
            np.testing.assert_array_equal(o_idx.get().reshape(q, count), want, err_msg=f"count {count} q {q}")
    # a query without a place: KAD_NO_NODE and 0
    d_slot = Buf(gpu, np.full(1, NONE, np.uint32))
    o_idx, o_cnt = Buf(gpu, nbytes=4 * count, shift=shift), Buf(gpu, nbytes=1)
    _lib.check(L.kad_route_unpack(d_slot.ptr, 1, count, d_back.ptr, d_bcnt.ptr, o_idx.ptr, o_cnt.ptr, 0, None), "none")
    _sync()
    assert o_cnt.get(np.uint8)[0] == 0 and (o_idx.get() == NONE).all()


# ---- kad_route_pack / _pack_keys / _pack_ex ------------------------------------------------------------------------
_TARGETS = None


def _targets():
    global _TARGETS
    if _TARGETS is None:
        t = np.random.default_rng(0x9AC).integers(0, 256, (9000, 20), dtype=np.uint8)
        t[:256, 0] = np.arange(256)  # every first byte, so every owner of every (world, shard_bits)
        t.setflags(write=False)
        _TARGETS = t
    return _TARGETS


def _check_pack(where, t, world, bits, cap, keys, slot, send, ctr, before=0):
    """Counters, overflow word, owners, sub-blocks, uniqueness and record contents against expect_pack. `before`:
    the count every sub-block's counter held on entry (KAD_ROUTE_ZEROED on a counter block that is not zero)."""
    e = R.expect_pack(t, world, bits, cap)
    q, sub, rec = t.shape[0], cap // SUBS, 8 if keys else 20
    room = np.clip(sub - before, 0, None)
    placed = np.minimum(e["ctr"], room)
    overflow = int((e["ctr"] > room).any())
    want = R.ctr_image(e["ctr"] + before, world, overflow=overflow)
    np.testing.assert_array_equal(ctr, want, err_msg=where + ": ctr")
    none = slot == NONE
    s = slot[~none].astype(np.int64)
    d, r = e["owner"][~none], e["sub"][~none]
    np.testing.assert_array_equal(s // cap, d, err_msg=where + ": a record outside its owner's block")
    np.testing.assert_array_equal((s % cap) // sub, r, err_msg=where + ": a record outside its workgroup's sub-block")
    at = s % sub
    assert ((at >= before) & (at < before + placed[d, r])).all(), where + ": a record past its sub-block's count"
    assert np.unique(s).size == s.size, where + ": two queries share a record"
    dropped = np.zeros((world, SUBS), np.int64)
    np.add.at(dropped, (e["owner"][none], e["sub"][none]), 1)
    np.testing.assert_array_equal(dropped, e["ctr"] - placed, err_msg=where + ": KAD_NO_NODE slots per sub-block")
    recs = send.reshape(world * cap, rec)
    want = np.ascontiguousarray(t[:, :8]).view(">u8").astype("<u8").view(np.uint8).reshape(q, 8) if keys else t
    np.testing.assert_array_equal(recs[s], want[~none], err_msg=where + ": record contents")
    rest = np.ones(world * cap, bool)
    rest[s] = False
    assert (recs[rest] == GUARD).all(), where + ": a record no query owns was written"


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 5, 8, 16])
def test_pack_against_the_model(gpu, world):
    L = _lib.lib()
    T = _targets()
    d_t = Buf(gpu, T)
    for bits in sorted({0, math.ceil(math.log2(world)), 8}):
        for q in (1, 1023, 1024, 1025, 5000, 9000):
            t = T[:q]
            fullest = int(R.expect_pack(t, world, bits, SUBS)["ctr"].max())
            for cap in sorted({SUBS * fullest, SUBS * (fullest + 3), SUBS}):  # exactly enough, roomy, one record each
                forms = [("pack", False, lambda s, sl, c: L.kad_route_pack(d_t.ptr, q, world, bits, cap, s, sl, c, 0, None)),
                         ("pack_keys", True,
                          lambda s, sl, c: L.kad_route_pack_keys(d_t.ptr, q, world, bits, cap, s, sl, c, 0, None))]
                for mode in (0, R.KEYS, R.ZEROED, R.KEYS | R.ZEROED):
                    forms.append((f"pack_ex({mode})", bool(mode & R.KEYS),
                                  lambda s, sl, c, mode=mode: L.kad_route_pack_ex(d_t.ptr, q, world, bits, cap, s, sl, c,
                                                                                 mode, 0, None)))
                for name, keys, fn in forms:
                    where = f"{name} world {world} bits {bits} q {q} cap {cap}"
                    zeroed = name in ("pack_ex(4)", "pack_ex(6)")
                    send = Buf(gpu, nbytes=world * cap * (8 if keys else 20))
                    slot = Buf(gpu, nbytes=4 * q)
                    # the plain forms zero the counters themselves: hand them junk
                    ctr = Buf(gpu, nbytes=4 * R.ctr_words(world), fill=0 if zeroed else 0x5C)
                    _lib.check(fn(send.ptr, slot.ptr, ctr.ptr), where)
                    _sync()
                    _check_pack(where, t, world, bits, cap, keys, slot.get(), send.get(np.uint8), ctr.get())
    # KAD_ROUTE_ZEROED really does not clear: on counters holding 2 it appends from place 2 on
    for bits, q in ((8 if world > 1 else 0, 5000), (math.ceil(math.log2(world)), 1025)):
        t = T[:q]
        fullest = int(R.expect_pack(t, world, bits, SUBS)["ctr"].max())
        for cap in (SUBS * (fullest + 2), SUBS * (fullest + 1)):  # exactly enough after the 2, one too few
            for mode in (R.ZEROED, R.KEYS | R.ZEROED):
                keys = bool(mode & R.KEYS)
                where = f"pack_ex({mode}) on counters of 2: world {world} bits {bits} q {q} cap {cap}"
                send, slot = Buf(gpu, nbytes=world * cap * (8 if keys else 20)), Buf(gpu, nbytes=4 * q)
                ctr = Buf(gpu, R.ctr_image(np.full(world * SUBS, 2), world))
                _lib.check(L.kad_route_pack_ex(d_t.ptr, q, world, bits, cap, send.ptr, slot.ptr, ctr.ptr, mode, 0, None), where)
                _sync()
                _check_pack(where, t, world, bits, cap, keys, slot.get(), send.get(np.uint8), ctr.get(), before=2)
    # q = 0: the plain forms still zero the counters, the ZEROED form leaves them
    for mode, want in ((0, 0), (R.KEYS, 0), (R.ZEROED, 0x5C5C5C5C)):
        ctr = Buf(gpu, nbytes=4 * R.ctr_words(world), fill=0x5C)
        _lib.check(L.kad_route_pack_ex(None, 0, world, 0, SUBS, None, None, ctr.ptr, mode, 0, None), "q = 0")
        _sync()
        assert (ctr.get() == want).all()


# ---- kad_route_unpack_packed_fold / kad_route_fold_flags -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3, 16])
def test_fold_and_reset(gpu, world):
    L = _lib.lib()
    T = _targets()[:5000]
    bits = math.ceil(math.log2(world))
    e = R.expect_pack(T, world, bits, SUBS)
    fullest = int(e["ctr"].max())
    rng = np.random.default_rng(world)
    nw, ov = R.ctr_words(world), R.overflow_word(world)
    # the counters of a real pack (cap that fits, and one record per sub-block: the overflow word set by the kernel),
    # then images written by hand: the fullest sub-block the first, the last, and none at all
    images = []
    d_t = Buf(gpu, T)
    for cap in (SUBS * fullest, SUBS):
        send, slot, ctr = Buf(gpu, nbytes=world * cap * 20), Buf(gpu, nbytes=4 * 5000), Buf(gpu, nbytes=4 * nw)
        _lib.check(L.kad_route_pack(d_t.ptr, 5000, world, bits, cap, send.ptr, slot.ptr, ctr.ptr, 0, None), "pack")
        _sync()
        img = ctr.get()
        np.testing.assert_array_equal(img, R.ctr_image(e["ctr"], world, overflow=int(cap == SUBS and fullest > 1)))
        images.append(img)
    hand = rng.integers(1, 1000, world * SUBS)
    hand[0] = 70_000
    images.append(R.ctr_image(hand, world))
    hand = hand.copy()
    hand[0], hand[-1] = 5, 0x0FFFFFFF
    images.append(R.ctr_image(hand, world))
    images.append(R.ctr_image(np.zeros(world * SUBS), world))
    starts = ([0, 0, 0, 0], [1, 0, 1, 10 ** 6], [0, 1, 0, 5], [4, 2, 0, 0xFFFFFFFF])
    for count, shift in ((8, 0), (8, 1), (14, 0), (20, 0), (32, 1)):
        rows, cnt = R.synth_rows(count, n=300, seed=world)
        ok = np.nonzero(~R.escapes_rows(rows, cnt))[0]
        full = np.where(np.arange(count)[None, :] < cnt[:, None], rows, NONE).astype(np.uint32)
        back = Buf(gpu, R.pack_rows(rows, cnt, count))
        for k, img in enumerate(images):
            for words in ((0, 0), (1, 0), (0, 1), (3, 9)):  # escape and tail set by hand (any non-zero word counts)
                img = img.copy()
                img[ov + 1:ov + 3] = words
                f0 = np.array(starts[(k + sum(words)) % len(starts)], np.uint32)
                where = f"world {world} count {count} shift {shift} image {k} escape/tail {words} flags {f0.tolist()}"
                for q in (257, 0):
                    slot = _slots(ok, max(q, 1), rng)
                    d_slot = Buf(gpu, slot)
                    ctr, flags = Buf(gpu, img), Buf(gpu, f0)
                    o_idx, o_cnt = Buf(gpu, nbytes=4 * q * count, shift=shift), Buf(gpu, nbytes=q)
                    if q == 0 and k % 2:  # the fold alone needs no row buffers (kad_route_run's plain way back)
                        _lib.check(L.kad_route_unpack_packed_fold(None, 0, count, None, None, None, ctr.ptr, world,
                                                                  flags.ptr, 0, None), where)
                    else:
                        _lib.check(L.kad_route_unpack_packed_fold(d_slot.ptr, q, count, back.ptr, o_idx.ptr, o_cnt.ptr,
                                                                  ctr.ptr, world, flags.ptr, 0, None), where)
                    _sync()
                    np.testing.assert_array_equal(flags.get(), R.expect_fold(img, world, f0), err_msg=where + f" q {q}")
                    assert not ctr.get().any(), where + f" q {q}: ctr is not zero afterwards"
                    if q == 0:
                        o_idx.get(), o_cnt.get(np.uint8)  # (empty outputs: only their guards)
                        continue
                    p_idx, p_cnt = Buf(gpu, nbytes=4 * q * count, shift=shift), Buf(gpu, nbytes=q)
                    _lib.check(L.kad_route_unpack_packed(d_slot.ptr, q, count, back.ptr, p_idx.ptr, p_cnt.ptr, 0, None), where)
                    _sync()
                    want, wcnt = R.unpack_rows(slot, full, cnt, count)
                    for got_i, got_c in ((o_idx, o_cnt), (p_idx, p_cnt)):
                        np.testing.assert_array_equal(got_c.get(np.uint8), wcnt, err_msg=where)
                        np.testing.assert_array_equal(got_i.get().reshape(q, count), want, err_msg=where)
                # kad_route_fold_flags: words 0..2 OR-ed, flags[3] and the counters left alone
                ctr, flags = Buf(gpu, img), Buf(gpu, f0)
                _lib.check(L.kad_route_fold_flags(ctr.ptr, world, flags.ptr, 0, None), where)
                _sync()
                want = R.expect_fold(img, world, f0)
                want[3] = f0[3]
                np.testing.assert_array_equal(flags.get(), want, err_msg=where + " fold_flags")
                np.testing.assert_array_equal(ctr.get(), img, err_msg=where + " fold_flags wrote the counters")
