"""Config 5 edge cases: swarms and lookups outside the random regime of test_swarm.py — tiny
swarms, peers at the table's depth cap, one-sided tables, top-64 ties among three and more peers, distances equal to
the kernels' padding value, sources that are offline themselves. Deterministic, numpy only, no GPU work.

A case is (ids, src, targets): ascending 160-bit peer IDs (n, 20), and one source index and target per lookup."""
import functools

import numpy as np

LEVELS = 28  # KAD_SWARM_LEVELS: a peer's depth is capped at LEVELS - 1
CAP_DEPTH = LEVELS - 1
TINY = (2, 3, 9, 10, 11, 17)
BIG = ("random5k", "clustered", "oneprefix", "lopsided")
NAMES = tuple(f"tiny{n}" for n in TINY) + BIG + ("tinyskew",)
TINY_NAMES = tuple(x for x in NAMES if x.startswith("tiny"))
OFFLINE_BIG = (0, 3000, 6000, 8000, 9700, 10000)
OFFLINE_TINY = (0, 5000, 10000)


def offline_shares(name):
    return OFFLINE_TINY if name.startswith("tiny") else OFFLINE_BIG


def key64(ids):
    return ids[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)


def _put_key(ids, rows, key):
    ids[rows, :8] = np.asarray(key, np.uint64).astype(">u8").view(np.uint8).reshape(-1, 8)


def _sorted_unique(ids):
    ids = ids[np.lexsort(ids.T[::-1])]
    keep = np.ones(ids.shape[0], bool)
    keep[1:] = (ids[1:] != ids[:-1]).any(axis=1)
    return np.ascontiguousarray(ids[keep])


def _rand_ids(rng, n):
    return rng.integers(0, 256, size=(n, 20), dtype=np.uint8)


def _under_prefix(rng, n, prefix, bits):
    """n random IDs whose top `bits` bits (<= 64) are those of the 64-bit value `prefix`."""
    ids = _rand_ids(rng, n)
    if bits:
        keep = np.uint64(((1 << bits) - 1) << (64 - bits))
        _put_key(ids, slice(None), (key64(ids) & ~keep) | (np.uint64(prefix) & keep))
    return ids


def offline(p, per10k):
    """swarm_offline (kad_swarm.hip / kad_oracle.cpp): splitmix64 of p * 0x9E37 + 0xBAD, mod 10000 < per10k."""
    with np.errstate(over="ignore"):  # (the products wrap, as in C)
        x = (np.asarray(p, np.uint64) * np.uint64(0x9E37) + np.uint64(0xBAD)) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x % np.uint64(10000)) < np.uint64(per10k)


def run_of(key, p, bits):
    """[lo, hi): the peers sharing their top `bits` bits with peer p (key ascending)."""
    if bits == 0:
        return 0, key.shape[0]
    sh = np.uint64(64 - bits)
    pre = key >> sh
    return int(np.searchsorted(pre, pre[p], "left")), int(np.searchsorted(pre, pre[p], "right"))


def depth_of(key, p):
    """The model's depth: the least D with at most 8 other peers sharing >= D leading bits, capped."""
    for D in range(CAP_DEPTH + 1):
        lo, hi = run_of(key, p, D)
        if hi - lo - 1 <= 8 or D == CAP_DEPTH:
            return D


# ---- swarms ---------------------------------------------------------------------------------------------------
def _tiny(n):
    return _sorted_unique(_rand_ids(np.random.default_rng(0x71 + n), n))


def _tinyskew(seed=0x5E1):
    """14 peers, four in five of them with a 0 in each of the top three bits: a peer of a small subtree knows 8 of the
    more than 8 peers of a large one, so a lookup's list has room left (fewer than SEARCH_NODES nodes known) when an
    answer names the rest — among them, for a complement target, the node at the padding distance."""
    rng = np.random.default_rng(seed)
    ids = _rand_ids(rng, 14)
    for b in range(3):
        ids[rng.random(14) < 0.8, 0] &= np.uint8(0xFF ^ (0x80 >> b))
    return _sorted_unique(ids)


def _random5k():
    return _sorted_unique(_rand_ids(np.random.default_rng(0x5C1), 5000))


def _clustered(seed=0x5C7):
    """Groups of 12 to 40 peers sharing exactly 27, 28, 40 or all 64 leading bits (the last: identical top-64 keys,
    the order among them in the 96-bit tails), under random group prefixes."""
    rng = np.random.default_rng(seed)
    parts = []
    for bits in (27, 28, 40, 64):
        for _ in range(6):
            m = int(rng.integers(12, 41))
            pre = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
            g = _under_prefix(rng, m, pre, bits)
            if bits < 64:  # exactly `bits`: both values of the next bit occur
                k = key64(g)
                nb = np.uint64(1 << (63 - bits))
                k[0], k[1] = k[0] | nb, k[1] & ~nb
                _put_key(g, slice(0, 2), k[:2])
            parts.append(g)
    return _sorted_unique(np.concatenate(parts))


def _oneprefix():
    """400 peers under one 28-bit prefix: every peer sits at the depth cap with an empty level above it."""
    rng = np.random.default_rng(0x5C3)
    return _sorted_unique(_under_prefix(rng, 400, 0xA5C3_9E10_0000_0000, 28))


def _lopsided():
    """A comb of keys 1...10xxxx: the peers sharing exactly d bits with a peer all have a 0 where it has a 1, so its
    levels all lie below its own bucket and the closest-node windows run into the table's ends."""
    rng = np.random.default_rng(0x5C4)
    parts = []
    for ones in range(0, 58):
        xs = rng.choice(16, size=10, replace=False)
        g = _rand_ids(rng, 10)
        top = ((1 << ones) - 1) << (64 - ones) if ones else 0
        k = (key64(g) & np.uint64((1 << (59 - ones)) - 1)) | np.uint64(top)
        k |= xs.astype(np.uint64) << np.uint64(59 - ones)  # (bit `ones` stays 0)
        _put_key(g, slice(None), k)
        parts.append(g)
    return _sorted_unique(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def swarm(name):
    if name == "tinyskew":
        ids = _tinyskew()
    elif name.startswith("tiny"):
        ids = _tiny(int(name[4:]))
    else:
        ids = {"random5k": _random5k, "clustered": _clustered, "oneprefix": _oneprefix, "lopsided": _lopsided}[name]()
    ids.setflags(write=False)
    return ids


# ---- targets --------------------------------------------------------------------------------------------------
def _share_exactly(rng, idv, d):
    """A target sharing exactly d leading bits with the ID idv (d < 160)."""
    t = _rand_ids(rng, 1)[0]
    byte, bit = divmod(d, 8)
    t[:byte] = idv[:byte]
    keep = (0xFF << (8 - bit)) & 0xFF  # the first `bit` bits of this byte
    flip = 0x80 >> bit
    t[byte] = (idv[byte] & keep) | ((idv[byte] ^ 0xFF) & flip) | (t[byte] & (flip - 1))
    return t


def prefix_target(name, ids, p, d):
    """The case's target sharing exactly d leading bits with peer p (its other bits drawn from (swarm, p, d) alone)."""
    return _share_exactly(np.random.default_rng([0xD817, NAMES.index(name), p, d]), ids[p], d)


# The 64 sources of the one-target-per-d lookups are a random choice of peers, except on `clustered`: at 60 % offline
# a lookup expires only if every node of its seed list is offline (an online seed stays in the list as a non-bad node),
# one lookup in a few hundred, so there the 44 peers that have such a lookup expire come first (found by running the
# oracle over every peer's 29; most of them are one group's) and a random choice fills the 64.
# test_swarm_cases.py asserts what this buys: >= 50 expired lookups at 6000.
FIRST_SOURCES = {"clustered": (44,) + tuple(range(197, 231)) + (336, 351, 356, 443, 444, 474, 483, 485, 564)}


def _tail_int(idv):
    return int.from_bytes(idv[8:].tobytes(), "big")


def _with_tail(idv, tail):
    t = idv.copy()
    t[8:] = np.frombuffer(int(tail).to_bytes(12, "big"), np.uint8)
    return t


def tied_groups(ids):
    """Runs of >= 2 peers with identical top-64 keys: [(lo, hi)]."""
    key = key64(ids)
    cut = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1], [True]]))
    return [(int(a), int(b)) for a, b in zip(cut[:-1], cut[1:]) if b - a >= 2]


@functools.lru_cache(maxsize=None)
def case(name):
    """(ids, src, targets) of a swarm: every target kind of the module's header, from unfiltered sources."""
    ids = swarm(name)
    n = ids.shape[0]
    key = key64(ids)
    rng = np.random.default_rng(0xCA5E + NAMES.index(name))
    tiny = name.startswith("tiny")
    src, tg = [], []

    def add(s, t):
        src.append(np.asarray(s, np.uint32).reshape(-1))
        tg.append(np.asarray(t, np.uint8).reshape(-1, 20))

    first = np.arange(n) if n <= 64 else rng.choice(n, 64, replace=False)
    if name in FIRST_SOURCES:
        fixed = np.array(FIRST_SOURCES[name])
        first = np.concatenate([fixed, rng.choice(np.setdiff1d(np.arange(n), fixed), 64 - fixed.size, replace=False)])
    for p in first:  # one target per d sharing exactly d leading bits with the source, d = 0..D+1
        for d in range(depth_of(key, int(p)) + 2):
            add([p], prefix_target(name, ids, int(p), d))
    for lo, hi in tied_groups(ids)[:8]:  # on a tied group's top 64 bits: tails below, between and above the group's
        tails = sorted(_tail_int(ids[x]) for x in range(lo, hi))
        want = [tails[0] - 1 if tails[0] else 0, (tails[0] + tails[1]) // 2, tails[-1] + 1 if tails[-1] < (1 << 96) - 1
                else tails[-1]]
        for tl in want:
            add(rng.integers(0, n, 3), np.repeat(_with_tail(ids[lo], tl)[None], 3, axis=0))
    # the other kinds share what is left of 2,000 lookups (the depth-cap swarms spend 64 x 29 above)
    k = 24 if tiny else min(96, (2000 - 8 - sum(x.shape[0] for x in src)) // 7)
    assert k >= 8
    add(rng.integers(0, n, 4 * k), _rand_ids(rng, 4 * k))  # random
    add(rng.integers(0, n, k), ids[rng.integers(0, n, k)])  # peer IDs
    s = rng.integers(0, n, k)
    add(s, ids[s])  # the source's own ID
    # the complement of a peer's top 64 bits: top-64 distance ~0, the kernels' padding value (tiny swarms: of every
    # peer, from every source)
    cs, cp = (np.repeat(np.arange(n), n), np.tile(np.arange(n), n)) if tiny else (rng.integers(0, n, k),
                                                                                 rng.integers(0, n, k))
    t = _rand_ids(rng, cs.shape[0])
    t[:, :8] = ~ids[cp, :8]
    add(cs, t)
    add(rng.integers(0, n, 8), np.repeat(np.array([[0x00] * 20, [0xFF] * 20], np.uint8), 4, axis=0))
    src, tg = np.concatenate(src), np.ascontiguousarray(np.concatenate(tg))
    assert src.shape[0] == tg.shape[0] <= 2000 and n <= 5000
    src.setflags(write=False)
    tg.setflags(write=False)
    return ids, src, tg


def tied_pairs(n=2000):
    """test_swarm_gpu_top64_ties_hop_by_hop's construction at n peers: peer 2i+1 takes peer 2i's top 64 bits; a tenth
    of the targets sit on a pair's top 64 bits."""
    rng = np.random.default_rng(0x5AB)
    ids = _rand_ids(rng, n)
    ids[1::2, :8] = ids[0::2, :8]
    ids = _sorted_unique(ids)
    S = 600
    src = rng.integers(0, ids.shape[0], S).astype(np.uint32)
    tg = _rand_ids(rng, S)
    tg[:60, :8] = ids[rng.integers(0, ids.shape[0], 60), :8]
    return ids, src, tg
