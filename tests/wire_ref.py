"""Plain-Python references and named edge cases for the kernels that finish a request: kad_buffer_nodes_batch,
kad_parse_nodes_batch, kad_xor_cmp_batch, kad_common_bits_batch, kad_lowbit_batch and kad_infohash_get_batch.

The references use Python ints, `sorted` and hashlib; numpy only carries arrays. They do not load liboracle.so:
tests/test_wire_ref.py pins them to the oracle wherever the oracle is defined, and they go on where it is not (ties,
gaps, index_base != 0, cnt == NULL). Bit p of an ID counts from the most significant bit of byte 0 (InfoHash::getBit).
Every case builder returns named cases, so that a failing comparison can say which case it was."""
from __future__ import annotations

import hashlib
from collections import namedtuple

import numpy as np

NO_NODE = 0xFFFFFFFF
SEND_NODES = 8
ID_BITS = 160


def to_bytes(b) -> bytes:
    return bytes(b) if isinstance(b, (bytes, bytearray)) else np.asarray(b, np.uint8).tobytes()


def to_int(b) -> int:
    return int.from_bytes(to_bytes(b), "big")


def to_id(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(20, "big"), np.uint8).copy()


def bit(p: int) -> int:
    """The ID with only bit p set."""
    return 1 << (ID_BITS - 1 - p)


def _ids2d(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.uint8).reshape(-1, 20)


# ---------------------------------------------------------------------------------------------------------------
# InfoHash primitives
# ---------------------------------------------------------------------------------------------------------------
def xor_cmp_ref(t, a, b) -> int:
    x, y = to_int(a) ^ to_int(t), to_int(b) ^ to_int(t)
    return -1 if x < y else (1 if x > y else 0)


def common_bits_ref(a, b) -> int:
    return ID_BITS - (to_int(a) ^ to_int(b)).bit_length()


def lowbit_ref(a) -> int:
    x = to_int(a)
    if x == 0:
        return NO_NODE
    return ID_BITS - 1 - ((x & -x).bit_length() - 1)  # 159 - ctz


def sha1_ref(key: bytes) -> bytes:
    return hashlib.sha1(key).digest()


# ---------------------------------------------------------------------------------------------------------------
# NetworkEngine::bufferNodes, as the kernel defines it beyond the oracle's domain
# ---------------------------------------------------------------------------------------------------------------
def buffer_order_ref(target, ids_int, row, cnt, index_base=0):
    """The row's valid candidates (node numbers without index_base) in output order, all of them."""
    k = len(row)
    m = k if cnt is None else min(int(cnt), k)
    t = to_int(target)
    n_nodes = len(ids_int)
    kept = [int(g) - index_base for g in row[:m]
            if int(g) != NO_NODE and index_base <= int(g) < index_base + n_nodes]
    return sorted(kept, key=lambda v: ids_int[v] ^ t)  # sorted() is stable: equal distances keep row order


def buffer_nodes_ref(targets, ids, addrs, idx, cnt, index_base=0):
    """(out (q, 8 * (20 + addr_len)) uint8, n (q,) uint8); cnt None reads all k entries of every row."""
    targets, ids = _ids2d(targets), _ids2d(ids)
    addrs = np.ascontiguousarray(addrs, np.uint8)
    idx = np.asarray(idx, np.uint32)
    q = idx.shape[0]
    rec = 20 + addrs.shape[1]
    ids_int = [to_int(r) for r in ids]
    out = np.zeros((q, SEND_NODES * rec), np.uint8)
    n = np.zeros(q, np.uint8)
    for i in range(q):
        order = buffer_order_ref(targets[i], ids_int, idx[i], None if cnt is None else cnt[i], index_base)
        n[i] = min(len(order), SEND_NODES)
        for s, v in enumerate(order[:SEND_NODES]):
            out[i, s * rec:s * rec + 20] = ids[v]
            out[i, s * rec + 20:(s + 1) * rec] = addrs[v]
    return out, n


def deciding_word(x: int, y: int):
    """Index (0..4) of the first 32-bit word in which two 160-bit values differ; None if they are equal."""
    d = x ^ y
    return None if d == 0 else (ID_BITS - d.bit_length()) // 32


# ---------------------------------------------------------------------------------------------------------------
# NetworkEngine::isMartian and the deserializeNodes filter
# ---------------------------------------------------------------------------------------------------------------
V4_CLAUSES = ("port0", "this_net", "loopback", "class_de")
V6_CLAUSES = ("port0", "multicast", "link_local", "unspecified", "loopback", "v4mapped")


def martian_reasons(addr) -> set:
    """Every clause of isMartian that holds for a 6-byte (IPv4 + port) or 18-byte (IPv6 + port) address."""
    a = to_bytes(addr)
    if len(a) not in (6, 18):
        raise ValueError(f"address of {len(a)} bytes")
    r = set()
    if int.from_bytes(a[-2:], "big") == 0:
        r.add("port0")
    if len(a) == 6:
        if a[0] == 0:
            r.add("this_net")  # 0.0.0.0/8
        if a[0] == 127:
            r.add("loopback")  # 127.0.0.0/8
        if a[0] >= 224:
            r.add("class_de")  # 224.0.0.0/3: multicast and reserved
        return r
    ip = int.from_bytes(a[:16], "big")
    if ip >> 120 == 0xFF:
        r.add("multicast")  # ff00::/8
    if ip >> 118 == 0xFE80 >> 6:
        r.add("link_local")  # fe80::/10
    if ip == 0:
        r.add("unspecified")  # ::
    if ip == 1:
        r.add("loopback")  # ::1
    if ip >> 32 == 0xFFFF:
        r.add("v4mapped")  # ::ffff:0:0/96
    return r


def is_martian_ref(addr) -> bool:
    return bool(martian_reasons(addr))


def parse_nodes_ref(records, rec_len, myid) -> np.ndarray:
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, rec_len)
    me = to_bytes(myid)
    return np.array([int(r[:20].tobytes() != me and not is_martian_ref(r[20:])) for r in rec], np.uint8)


def hamming(a: bytes, b: bytes) -> int:
    return bin(int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).count("1")


def _v4(a0, a1, a2, a3, port):
    return bytes([a0, a1, a2, a3]) + port.to_bytes(2, "big")


def _v6(words, port):
    """words: the eight 16-bit groups of the address."""
    return b"".join(w.to_bytes(2, "big") for w in words) + port.to_bytes(2, "big")


def addr_cases(addr_len):
    """[(name, address bytes)]: every boundary of every isMartian clause, each with one-bit neighbours."""
    out = []
    if addr_len == 6:
        for a0 in (0, 1, 126, 127, 128, 223, 224, 255):
            out.append((f"a0={a0}", _v4(a0, 2, 3, 4, 4222)))
        for a0 in (0xC0, 0xA0, 0x60):  # one bit from 224
            out.append((f"a0={a0}", _v4(a0, 2, 3, 4, 4222)))
        out += [("port0", _v4(8, 8, 8, 8, 0)), ("port1", _v4(8, 8, 8, 8, 1)), ("port256", _v4(8, 8, 8, 8, 256)),
                ("0.0.0.0:0", _v4(0, 0, 0, 0, 0)), ("a1=127", _v4(8, 127, 0, 1, 4222)), ("a3=0", _v4(8, 8, 8, 0, 4222))]
        return out
    doc = [0x2001, 0xDB8, 0, 0, 0, 0, 0, 1]
    out += [("2001:db8::1", _v6(doc, 4222)), ("port0", _v6(doc, 0)), ("port1", _v6(doc, 1)), ("port256", _v6(doc, 256))]
    for w0 in (0xFF02, 0xFE02, 0x7F02, 0xFF00, 0xFFFF):  # ff00::/8 and the neighbours of ff02
        out.append((f"{w0:x}::1", _v6([w0, 0, 0, 0, 0, 0, 0, 1], 4222)))
    for w0 in (0xFE7F, 0xFE80, 0xFE81, 0xFEBF, 0xFEC0, 0xFE00, 0xFC80, 0xFE40, 0xFEFF, 0x7E80, 0x0080):  # fe80::/10
        out.append((f"{w0:x}::1", _v6([w0, 0, 0, 0, 0, 0, 0, 1], 4222)))
    for last in (0, 1, 2, 3, 0x100, 0x8000):  # ::, ::1 and what follows
        out.append((f"::{last:x}", _v6([0] * 7 + [last], 4222)))
    out += [("8000::", _v6([0x8000] + [0] * 7, 4222)), ("100::1", _v6([0x100] + [0] * 6 + [1], 4222)),
            ("0:0:0:0:0:0:1:0", _v6([0] * 6 + [1, 0], 4222)), ("0:0:0:0:0:0:1:1", _v6([0] * 6 + [1, 1], 4222))]
    mapped = _v6([0, 0, 0, 0, 0, 0xFFFF, 0x0808, 0x0808], 4222)
    out += [("::ffff:8.8.8.8", mapped), ("::ffff:0.0.0.0", _v6([0, 0, 0, 0, 0, 0xFFFF, 0, 0], 4222)),
            ("::ffff:255.255.255.255", _v6([0, 0, 0, 0, 0, 0xFFFF, 0xFFFF, 0xFFFF], 4222))]
    for j in range(12):  # ::ffff:0:0/96 with one prefix byte one bit off
        b = bytearray(mapped)
        b[j] ^= 1
        out.append((f"v4mapped/byte{j}^1", bytes(b)))
    return out


def _sane_addr(addr_len):
    return _v4(8, 8, 4, 4, 4222) if addr_len == 6 else _v6([0x2001, 0xDB8, 0, 0, 0, 0, 0, 2], 4222)


def parse_cases(rec_len, seed=11):
    """(names, records (n, rec_len) uint8, myid (20,) uint8), n >= 300: the boundary addresses under random IDs, the
    160 IDs one bit from myid and myid itself under a sane and a martian address, then random records."""
    al = rec_len - 20
    rng = np.random.default_rng([seed, rec_len])
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    me = to_int(myid)
    sane = np.frombuffer(_sane_addr(al), np.uint8)
    names, recs = [], []

    def add(name, id_, addr):
        names.append(name)
        recs.append(np.concatenate([np.asarray(id_, np.uint8), np.frombuffer(bytes(addr), np.uint8)]))

    add("myid/sane", myid, sane)  # first, so that the n = 1 prefix holds a dropped record
    for name, a in addr_cases(al):
        add("addr/" + name, rng.integers(0, 256, 20, dtype=np.uint8), a)
    for p in range(ID_BITS):
        add(f"myid^bit{p}/sane", to_id(me ^ bit(p)), sane)
    add("myid/martian", myid, addr_cases(al)[0][1])
    add("myid^bit159/martian", to_id(me ^ 1), _v4(127, 0, 0, 1, 80) if al == 6 else _v6([0] * 7 + [1], 80))
    add("myid/sane/again", myid, sane)
    k = 0
    while len(recs) < 300:
        add(f"random{k}", rng.integers(0, 256, 20, dtype=np.uint8), rng.integers(0, 256, al, dtype=np.uint8))
        k += 1
    return names, np.stack(recs), myid


# ---------------------------------------------------------------------------------------------------------------
# Primitive cases
# ---------------------------------------------------------------------------------------------------------------
def _rand160(rng) -> int:
    return to_int(rng.integers(0, 256, 20, dtype=np.uint8))


def pair_cases(seed=5):
    """(names, t, a, b), each (m, 20) uint8. For every bit p: a and b agree above p, differ at p, are random below; once
    under a target with bit p clear and once with bit p set (the sign of xorCmp flips). Then a == b under random t."""
    rng = np.random.default_rng(seed)
    names, T, A, B = [], [], [], []
    for p in range(ID_BITS):
        low = bit(p) - 1  # the bits below p
        hi = _rand160(rng) & ~(low | bit(p))
        a, b = hi | (_rand160(rng) & low), hi | bit(p) | (_rand160(rng) & low)
        if p & 1:
            a, b = b, a
        t = _rand160(rng)
        for name, tt in ((f"bit{p}/t_clear", t & ~bit(p)), (f"bit{p}/t_set", t | bit(p))):
            names.append(name), T.append(to_id(tt)), A.append(to_id(a)), B.append(to_id(b))
    for i, a in enumerate((0, (1 << ID_BITS) - 1, _rand160(rng), _rand160(rng), bit(0), 1)):
        names.append(f"equal{i}"), T.append(to_id(_rand160(rng))), A.append(to_id(a)), B.append(to_id(a))
    return names, np.stack(T), np.stack(A), np.stack(B)


def lowbit_cases(seed=6):
    """(names, a (m, 20) uint8): the zero ID, a single bit at every p, and bit p below random higher bits."""
    rng = np.random.default_rng(seed)
    names, A = ["zero"], [to_id(0)]
    for p in range(ID_BITS):
        names.append(f"single{p}"), A.append(to_id(bit(p)))
        high = _rand160(rng) & ~(2 * bit(p) - 1)
        names.append(f"high{p}"), A.append(to_id(high | bit(p)))
    names.append("ones"), A.append(to_id((1 << ID_BITS) - 1))
    return names, np.stack(A)


# ---------------------------------------------------------------------------------------------------------------
# SHA-1 keys
# ---------------------------------------------------------------------------------------------------------------
SHA1_EDGE_LENS = (55, 56, 63, 64, 119, 120, 127, 128, 1000)
SHA1_LONG_LEN = 70_001


def sha1_pack(seed=9):
    """(names, data uint8, offsets uint64 (m + 1)): keys packed back to back as kad_infohash_get_batch takes them. Every
    length 0..200, the lengths around the one- and two-block padding limits and 1000 each start at every alignment
    0..3 (filler keys of 1..3 bytes, hashed like any other, shift the next start); the last key is 70 001 bytes and
    ends the buffer."""
    rng = np.random.default_rng(seed)
    names, lens = [], []
    pos = 0

    def add(name, n):
        nonlocal pos
        names.append(name)
        lens.append(n)
        pos += n

    def add_at(name, n, align):
        if pos % 4 != align:
            add("fill", (align - pos) % 4)
        add(f"{name}/align{align}", n)

    for align in range(4):
        for n in range(201):
            add_at(f"len{n}", n, align)
    for n in SHA1_EDGE_LENS:
        for align in range(4):
            add_at(f"edge_len{n}", n, align)
    add_at(f"len{SHA1_LONG_LEN}", SHA1_LONG_LEN, 2)  # ends one byte short of a dword boundary
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return names, data, off


def sha1_keys(data, off):
    b = data.tobytes()
    return [b[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


# ---------------------------------------------------------------------------------------------------------------
# bufferNodes cases
# ---------------------------------------------------------------------------------------------------------------
BUFFER_KS = (0, 1, 7, 8, 9, 14, 16, 17, 31, 32)  # P = 8, 16 and 32 lanes per query, and k < P
BUFFER_QS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 257)  # a short last block for 32, 16 and 8 queries per block
BASE_TABLE_INDEX_BASE = 1000

BufCase = namedtuple("BufCase", "name target row cnt")  # row: (k,) uint32 with index_base added; cnt: what cnt[i] holds


def base_table(seed=0xBA5E):
    """40 sorted IDs for a table created with index_base = 1000. Three 8-byte heads: the second differs from the first
    in word 0, the third from the second in word 1 only. Under each head the nodes take one of two values for bytes
    8..11 and one of two for bytes 12..15, so groups share their first 8, 12 and 16 bytes and every one of the five
    32-bit words decides some order."""
    rng = np.random.default_rng(seed)
    h0 = rng.integers(0, 256, 8, dtype=np.uint8)
    h1 = h0.copy()
    h1[1] ^= 0x10
    h2 = h1.copy()
    h2[5] ^= 0x04
    ids = []
    for h, m in ((h0, 13), (h1, 13), (h2, 14)):
        w2 = rng.integers(0, 256, (2, 4), dtype=np.uint8)
        w3 = rng.integers(0, 256, (2, 4), dtype=np.uint8)
        for j in range(m):
            ids.append(np.concatenate([h, w2[j & 1], w3[(j >> 1) & 1], rng.integers(0, 256, 4, dtype=np.uint8)]))
    ids = np.stack(ids)
    order = sorted(range(len(ids)), key=lambda v: to_int(ids[v]))
    ids = np.ascontiguousarray(ids[order])
    assert len({to_int(r) for r in ids}) == len(ids)
    return ids


def make_addrs(n, addr_len, seed=5):
    """(n, addr_len) uint8, every row different (the first two bytes count the node), so that nodes with equal IDs
    still show which of them a record came from."""
    rng = np.random.default_rng([seed, addr_len])
    a = rng.integers(0, 256, (n, addr_len), dtype=np.uint8)
    a[:, 0], a[:, 1] = np.arange(n) >> 8, np.arange(n) & 255
    return a


def buffer_cases(ids, index_base, k, seed=3):
    """The named rows of width k for one table (host IDs in table order)."""
    ids = _ids2d(ids)
    n = ids.shape[0]
    ids_int = [to_int(r) for r in ids]
    rng = np.random.default_rng([seed, k, n, index_base])
    cases = []

    def rand_target():
        return rng.integers(0, 256, 20, dtype=np.uint8)

    def distinct(m, exclude=()):
        skip = set(exclude)
        return [int(v) for v in rng.permutation(n) if v not in skip][:m]

    def add(name, target, nodes, cnt, raw=()):
        """nodes: table-local node numbers; raw: {position: value} written as is."""
        row = np.array([v + index_base for v in nodes], np.uint32)
        for pos, val in dict(raw).items():
            row[pos] = val
        assert row.shape == (k,)
        cases.append(BufCase(f"k{k}/{name}", np.asarray(target, np.uint8).copy(), row, cnt))

    if k == 0:
        add("cnt0", rand_target(), [], 0)
        add("cnt5", rand_target(), [], 5)
        add("target_zero", np.zeros(20, np.uint8), [], 0)
        return cases

    groups = {}
    for v in range(n):
        groups.setdefault(ids[v, :8].tobytes(), []).append(v)
    groups = [g for g in groups.values() if len(g) >= 2]
    dups = {}
    for v in range(n):
        dups.setdefault(ids_int[v], []).append(v)
    dups = [d for d in dups.values() if len(d) >= 2]

    for r in range(2):
        g = groups[int(rng.integers(len(groups)))]
        inside = [int(v) for v in rng.permutation(g)[:k]]
        nodes = inside + distinct(k - len(inside), exclude=g)
        target = np.concatenate([ids[g[0], :8], rng.integers(0, 256, 12, dtype=np.uint8)])
        add(f"perm_in_group{r}", target, [nodes[j] for j in rng.permutation(k)], k)
        add(f"perm_across{r}", rand_target(), distinct(k), k)
    t = rand_target()
    add("reversed", t, sorted(distinct(k), key=lambda v: ids_int[v] ^ to_int(t), reverse=True), k)
    if k >= 2:
        nodes = distinct(k - 1)
        add("same_twice", rand_target(), nodes + nodes[:1], k)
        add("same_adjacent", ids[nodes[0]], nodes[:1] + nodes, k)
    for name, pos in (("front", 0), ("middle", k // 2), ("end", k - 1)):
        add(f"none_{name}", rand_target(), distinct(k), k, {pos: NO_NODE})
    add("all_none", rand_target(), distinct(k), k, {p: NO_NODE for p in range(k)})
    add("none_every_other", rand_target(), distinct(k), k, {p: NO_NODE for p in range(0, k, 2)})
    add("cnt0", rand_target(), distinct(k), 0)
    nodes = distinct(k)
    add("cnt_lt", ids[nodes[-1]], nodes, k // 2)  # the target is a node beyond cnt: reading it would put it first
    if k >= 3:
        add("cnt1", ids[nodes[1]], nodes, 1)
    add("cnt_eq", rand_target(), distinct(k), k)
    add("cnt_gt", rand_target(), distinct(k), k + 7)
    add("cnt255", rand_target(), distinct(k), 255)
    nodes = distinct(k)
    add("target_is_candidate", ids[nodes[k // 2]], nodes, k)
    add("target_zero", np.zeros(20, np.uint8), distinct(k), k)
    add("target_ones", np.full(20, 255, np.uint8), distinct(k), k)
    # node numbers just outside the table, next to valid ones (index_base - 1 would be NO_NODE at index_base 0)
    below = index_base - 1 if index_base else 0x80000000
    nodes = distinct(k)
    raw = {0: index_base + n}
    if k >= 3:
        raw[2] = below
    if k >= 5:
        raw[k - 1] = index_base + n + 1000
    add("out_of_range", rand_target(), nodes, k, raw)
    if k >= 2:
        by_value = sorted(range(n), key=lambda v: ids_int[v])
        for w in range(5):  # two nodes whose order only word w decides, the farther one first in the row
            pairs = [(x, y) for x, y in zip(by_value, by_value[1:]) if deciding_word(ids_int[x], ids_int[y]) == w]
            if not pairs:
                continue
            x, y = pairs[int(rng.integers(len(pairs)))]
            t = ids_int[x] >> (32 * (5 - w)) << (32 * (5 - w))  # the shared words, then zeros: distance = the rest
            far = max(ids_int[x] ^ t, ids_int[y] ^ t)
            fill = [v for v in distinct(n) if (ids_int[v] ^ t) > far][:k - 2]
            raw = {p: NO_NODE for p in range(2 + len(fill), k)}
            add(f"word{w}_decides", to_id(t), [y, x] + fill + [0] * (k - 2 - len(fill)), k, raw)
        for r, d in enumerate(dups):  # equal IDs under different addresses: row order must show in the output
            for name, order in (("a", d[::-1]), ("b", d[1:] + d[:1])):
                tie = order[:k]
                fill = distinct(k - len(tie), exclude=d)
                add(f"true_tie{r}{name}/first", ids[d[0]], tie + fill, k)
                add(f"true_tie{r}{name}/spread", rand_target(), tie[:1] + fill[:1] + tie[1:] + fill[1:], k)
    return cases


def buffer_tables():
    """[(name, table dict of tests/tables.py, index_base)]: the tie table, its sibling with duplicate IDs (unsorted), and
    the hand-made table at index_base 1000 (NodeCache-only: no buckets)."""
    import tables as TB

    ties, dups = TB.tie_table()
    base = base_table()
    return [("ties", ties, 0), ("dups", dups, 0),
            ("base1000", TB.table(base, np.ones(len(base), np.uint8), None, None, sorted_=True, name="base1000"),
             BASE_TABLE_INDEX_BASE)]
