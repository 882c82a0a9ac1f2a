"""Pins tests/wire_ref.py (CPU): the plain-Python references equal the oracle wherever the oracle is defined, and the
case lists hold what tests/test_wire_edges.py relies on, computed from the references alone."""
import numpy as np

import oracle as O
import wire_ref as W


def _all_buffer_cases():
    """(table name, table, index_base, case) over the three tables and every k."""
    for name, t, base in W.buffer_tables():
        for k in W.BUFFER_KS:
            for c in W.buffer_cases(t["ids"], base, k):
                yield name, t, base, c


def test_buffer_ref_known_answers():
    """The rules the oracle cannot speak for, on rows small enough to check by eye."""
    ids = np.zeros((4, 20), np.uint8)
    ids[0, 19], ids[1, 19], ids[2, 19], ids[3, 19] = 9, 4, 4, 1  # nodes 1 and 2 tie
    addrs = W.make_addrs(4, 6)
    t = np.zeros((1, 20), np.uint8)

    def nodes_of(row, cnt, base=0):
        out, n = W.buffer_nodes_ref(t, ids, addrs, np.array([row], np.uint32), None if cnt is None else [cnt], base)
        rec = out[0].reshape(8, 26)
        assert not rec[n[0]:].any()
        return [int(rec[s, 20]) * 256 + int(rec[s, 21]) for s in range(n[0])]  # make_addrs numbers the nodes

    assert nodes_of([0, 1, 2, 3], 4) == [3, 1, 2, 0]
    assert nodes_of([0, 2, 1, 3], 4) == [3, 2, 1, 0]  # the tie keeps row order
    assert nodes_of([W.NO_NODE, 0, W.NO_NODE, 3], None) == [3, 0]  # gaps are skipped, what follows is kept
    assert nodes_of([0, 1, 2, 3], 2) == [1, 0]
    assert nodes_of([0, 1, 2, 3], 200) == [3, 1, 2, 0]  # cnt > k is clamped
    assert nodes_of([7, 8, 11, 6], None, base=7) == [1, 0]  # 7 + 4 and 7 - 1 lie outside [7, 11)
    assert nodes_of([3, 3, 0], 3) == [3, 3, 0]


def test_buffer_ref_matches_oracle():
    """Every case in the oracle's domain: index_base 0, cnt given and within k, no gap, no tie."""
    checked = 0
    for al in (6, 18):
        for name, t, base in W.buffer_tables():
            if base:
                continue
            ids_int = [W.to_int(r) for r in t["ids"]]
            addrs = W.make_addrs(len(ids_int), al)
            for k in W.BUFFER_KS:
                cases = []
                for c in W.buffer_cases(t["ids"], base, k):
                    head = [int(g) for g in c.row[:min(c.cnt, k)]]
                    dist = [ids_int[g] ^ W.to_int(c.target) for g in head if g < len(ids_int)]
                    if c.cnt <= k and len(dist) == len(head) and len(set(dist)) == len(dist):
                        cases.append(c)
                assert cases, (name, k)
                tg = np.stack([c.target for c in cases])
                idx = np.stack([c.row for c in cases]).reshape(len(cases), k)
                cnt = np.array([c.cnt for c in cases], np.uint8)
                want, wn = O.buffer_nodes(tg, t["ids"], addrs, idx, cnt)
                got, gn = W.buffer_nodes_ref(tg, t["ids"], addrs, idx, cnt, 0)
                for i, c in enumerate(cases):
                    assert gn[i] == wn[i] and np.array_equal(got[i], want[i]), (name, al, c.name)
                checked += len(cases)
    assert checked > 400


def test_buffer_cases_cover():
    words = [0] * 5
    kept_classes = {"zero": 0, "fewer": 0, "eight": 0, "more": 0}
    true_ties = 0
    rows = 0
    names = set()
    for name, t, base, c in _all_buffer_cases():
        ids_int = [W.to_int(r) for r in t["ids"]]
        assert (name, c.name) not in names, "case names are unique within a table"
        names.add((name, c.name))
        for cnt in (c.cnt, None):
            rows += 1
            order = W.buffer_order_ref(c.target, ids_int, c.row, cnt, base)
            kept_classes["zero" if not order else "fewer" if len(order) < 8 else "eight" if len(order) == 8
                         else "more"] += 1
            sent = order[:W.SEND_NODES + 1]  # the ninth decides what is cut off
            tt = W.to_int(c.target)
            for x, y in zip(sent, sent[1:]):
                w = W.deciding_word(ids_int[x] ^ tt, ids_int[y] ^ tt)
                if w is None:
                    true_ties += x != y  # different nodes, so different addresses (make_addrs)
                else:
                    words[w] += 1
    assert all(words), f"adjacent output pairs decided per 32-bit word of the distance: {words}"
    assert all(kept_classes.values()), f"rows by number of valid candidates: {kept_classes}"
    assert true_ties >= 8, true_ties
    assert rows > 600
    for al in (6, 18):
        a = W.make_addrs(384, al)
        assert len({r.tobytes() for r in a}) == 384


def test_buffer_cases_hold_what_they_name():
    for name, t, base, c in _all_buffer_cases():
        k, n = len(c.row), t["ids"].shape[0]
        kind = c.name.split("/", 1)[1]
        if kind == "out_of_range":
            assert base + n in c.row
            assert k < 3 or (base - 1 if base else 0x80000000) in c.row
        if kind.startswith("none_") or kind == "all_none":
            assert W.NO_NODE in c.row
        if kind == "none_front":
            assert c.row[0] == W.NO_NODE
        if kind == "none_end":
            assert c.row[-1] == W.NO_NODE
        if kind == "cnt_gt":
            assert c.cnt > k
        if kind == "cnt_lt":
            assert c.cnt < k
        if kind == "same_twice":
            assert c.row[0] == c.row[-1]
        if kind.startswith("true_tie"):
            assert name == "dups"
    kinds = {c.name.split("/", 1)[1] for name, t, base, c in _all_buffer_cases() if name == "base1000"}
    assert {f"word{w}_decides" for w in range(5)} <= kinds  # the hand-made table alone reaches every word
    assert sorted({len(c.row) for _, _, _, c in _all_buffer_cases()}) == sorted(W.BUFFER_KS)


def test_martian_ref_matches_oracle():
    rng = np.random.default_rng(1)
    for al in (6, 18):
        cases = W.addr_cases(al) + [(f"random{i}", rng.integers(0, 256, al, dtype=np.uint8).tobytes())
                                    for i in range(2000)]
        for i in range(2000):  # random addresses almost never reach the IPv6 clauses: start from the cases
            b = bytearray(cases[i % len(W.addr_cases(al))][1])
            b[int(rng.integers(al))] ^= 1 << int(rng.integers(8))
            cases.append((f"flip{i}", bytes(b)))
        for name, a in cases:
            assert W.is_martian_ref(a) == bool(O.lib().orc_is_martian(a, al)), (al, name, a.hex())


def test_martian_cases_cover():
    for al, clauses in ((6, W.V4_CLAUSES), (18, W.V6_CLAUSES)):
        cases = W.addr_cases(al)
        assert len({n for n, _ in cases}) == len(cases)
        sane = [a for _, a in cases if not W.martian_reasons(a)]
        for c in clauses:
            sole = [a for _, a in cases if W.martian_reasons(a) == {c}]
            assert sole, (al, c)
            assert any(W.hamming(m, s) == 1 for m in sole for s in sane), f"no sane one-bit neighbour of {c} ({al})"
    first = {a[0] for _, a in W.addr_cases(6)}
    assert {0, 1, 126, 127, 128, 223, 224, 255} <= first
    six = {n: a for n, a in W.addr_cases(18)}
    assert [bool(W.martian_reasons(six[n])) for n in ("fe7f::1", "fe80::1", "febf::1", "fec0::1")] == [False, True, True,
                                                                                                     False]
    assert [bool(W.martian_reasons(six[n])) for n in ("::0", "::1", "::2")] == [True, True, False]
    assert W.martian_reasons(six["::ffff:8.8.8.8"]) == {"v4mapped"}
    assert not any(W.martian_reasons(six[f"v4mapped/byte{j}^1"]) for j in range(12))


def test_parse_ref_matches_oracle_and_cases_cover():
    for rec_len in (26, 38):
        names, rec, myid = W.parse_cases(rec_len)
        assert len(set(names)) == len(names) >= 300
        keep = W.parse_nodes_ref(rec, rec_len, myid)
        np.testing.assert_array_equal(keep, O.parse_nodes(rec, rec_len, myid))
        by = dict(zip(names, keep))
        me = W.to_int(myid)
        near = {W.to_int(r[:20]) ^ me for n, r in zip(names, rec) if n.endswith("/sane") and n.startswith("myid^")}
        assert near == {W.bit(p) for p in range(W.ID_BITS)}
        assert all(by[f"myid^bit{p}/sane"] == 1 for p in range(W.ID_BITS))
        assert by["myid/sane"] == 0 and by["myid/martian"] == 0 and by["myid^bit159/martian"] == 0
        for (n, a) in W.addr_cases(rec_len - 20):
            assert by["addr/" + n] == (not W.martian_reasons(a)), n
        assert 0 < keep[:255].sum() < 255 and keep[0] == 0


def test_primitive_refs_match_oracle_and_cases_cover():
    names, T, A, B = W.pair_cases()
    cb = [W.common_bits_ref(a, b) for a, b in zip(A, B)]
    xc = [W.xor_cmp_ref(t, a, b) for t, a, b in zip(T, A, B)]
    for i, n in enumerate(names):
        assert cb[i] == O.common_bits(A[i].tobytes(), B[i].tobytes()), n
        assert xc[i] == O.xor_cmp(T[i].tobytes(), A[i].tobytes(), B[i].tobytes()), n
    for p in range(W.ID_BITS):
        assert {xc[i] for i in range(len(names)) if cb[i] == p} == {-1, 1}, f"bit {p}: both signs of xorCmp"
    assert [(cb[i], xc[i]) for i, n in enumerate(names) if n.startswith("equal")] == [(160, 0)] * 6
    names, A = W.lowbit_cases()
    lb = [W.lowbit_ref(a) for a in A]
    for i, n in enumerate(names):
        assert lb[i] == O.lowbit(A[i].tobytes()) & 0xFFFFFFFF, n
    assert set(range(W.ID_BITS)) <= set(lb) and lb[0] == W.NO_NODE
    for p in range(W.ID_BITS):
        assert lb[names.index(f"single{p}")] == p == lb[names.index(f"high{p}")]
    rng = np.random.default_rng(2)  # and away from the cases
    for _ in range(300):
        t, a, b = (rng.integers(0, 256, 20, dtype=np.uint8) for _ in range(3))
        k = int(rng.integers(0, 21))
        b[:k] = a[:k]
        assert W.xor_cmp_ref(t, a, b) == O.xor_cmp(t.tobytes(), a.tobytes(), b.tobytes())
        assert W.common_bits_ref(a, b) == O.common_bits(a.tobytes(), b.tobytes())
        assert W.lowbit_ref(a) == O.lowbit(a.tobytes()) & 0xFFFFFFFF


def test_sha1_ref_matches_oracle_and_cases_cover():
    names, data, off = W.sha1_pack()
    keys = W.sha1_keys(data, off)
    assert len(keys) == len(names) and int(off[-1]) == data.size
    got = O.infohash_get(keys)
    for n, k, g in zip(names, keys, got):
        assert g.tobytes() == W.sha1_ref(k), n
    grid = {(len(k) % 64, int(o) % 4) for k, o in zip(keys, off)}
    assert grid == {(m, a) for m in range(64) for a in range(4)}
    pairs = {(len(k), int(o) % 4) for k, o in zip(keys, off)}
    for n in tuple(range(201)) + W.SHA1_EDGE_LENS:
        assert {(n, a) for a in range(4)} <= pairs, n
    assert len(keys[-1]) == W.SHA1_LONG_LEN and int(off[-1]) % 4 != 0  # the last dword of the buffer is partly key
    assert names[0] == "len0/align0" and len(keys) > 257
