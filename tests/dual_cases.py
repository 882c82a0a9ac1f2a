"""Table catalogue, pair list and dispatch model of the dual-family query tests (test_dual_matrix.py, and the
CPU tests of test_dual_cases.py).

kad_rt_closest_batch_dual picks among sixteen launches and kad_nc_closest_batch_dual among five, by the count and
by the line sets each family carries. `rt_launch` / `nc_launch` restate that choice from a family's public state
(kad_table_get_info flags, kad_table_line_sets mask, bucket count), so that every pair of the list can say which
launch it is there for and the GPU test can confirm that the tables it built take it."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import oracle as O
import tables as TB
from opendht_amd._lib import (KAD_INFO_GENERAL_LINES, KAD_INFO_GENERAL_LINES16, KAD_INFO_GENERAL_LINES32,
                              KAD_INFO_NODECACHE_LINES32, KAD_INFO_SHORT_LINES, KAD_INFO_SLOT_LINES,
                              KAD_INFO_SLOT_LINES16, KAD_INFO_WINDOW_LINES, KAD_NO_NODE)

RT_LAUNCHES = (
    "rt_dual_wl_lean_kernel", "rt_dual_wl_kernel", "rt_dual_sl_kernel",
    "rt_dual_gl_kernel<8>", "rt_dual_gl_kernel<16>", "rt_dual_gl_kernel<32>",
    "launch_rt_dual<8>", "launch_rt_dual<16>", "launch_rt_dual<32>",
    "rt_dual_wl16_kernel<true>", "rt_dual_wl16_kernel<false>", "rt_dual_sl16_kernel",
    "rt_dual_wl32q_kernel<false>", "rt_dual_wl32q_kernel<true>",
    "rt_dual_wl32_kernel<true>", "rt_dual_wl32_kernel<false>",
    "rt_wave_kernel",
)
NC_LAUNCHES = ("ncl2_lane_kernel<0,true>", "nc_line_kernel<0,true,false>", "nc32_line_kernel<0,true>",
               "nc_two_pass_dual_kernel", "nc_closest_dual_kernel")

RT_COUNTS = tuple(range(1, 33)) + (33, 40, 64, 65, 100, 300)
NC_COUNTS = tuple(range(1, 33)) + (33, 40, 48, 63, 64, 65, 100, 300)
PATTERN_COUNTS = (8, 14, 20, 24, 32)  # every af pattern; the other counts run the random pattern alone
AF_PATTERNS = ("alternating", "random", "runs64", "runs256", "all0", "all1")
BASE_COUNTS = (5, 8, 14, 16, 20, 32, 40)
BASE6 = 0x40000000
NCL2_COUNT_MAX = 14  # kad_engine.hip: the 128-byte NodeCache lines answer counts up to 14


# ---- catalogue --------------------------------------------------------------------------------------------------
def _named(tables, name):
    return next(t for t in tables if t["name"] == name)


def _build(cls):
    """One catalogue table (a tables.py dict), or None for a missing family."""
    if cls == "NONE":
        return None
    if cls in ("UW_dense", "U_tiny", "CLUSTERED"):
        import test_gpu_parity as GP  # its builders, not copies of them
        if cls == "CLUSTERED":
            return _named(GP._nc_tables(), "clustered")
        return _named(GP._wl_tables(), {"UW_dense": "dense_U8", "U_tiny": "U1_five"}[cls])
    if cls in ("S3", "S257", "EMPTY_B1", "EMPTY_B0"):
        return _named(TB.tiny_tables(), {"S3": "S3", "S257": "S257", "EMPTY_B1": "one_empty_bucket",
                                          "EMPTY_B0": "empty"}[cls])
    if cls in ("TIES48", "DUPS"):
        return _named(TB.tie_table(groups=24, per=48, seed=8, tag="48") if cls == "TIES48" else TB.tie_table(),
                      {"TIES48": "ties48", "DUPS": "dups"}[cls])
    return {
        "UW": lambda: TB.uniform_config(20_000, 11),
        "UW_sparse": lambda: TB.uniform_config(30_000, 13, good=12, expired=44),
        "SG": lambda: TB.split_config(20_000),
        "SG2": lambda: TB.split_config(20_000, seed=0x5E62),
        "SLANE": lambda: TB.split_config(20_000, seed=0x69, good=15, expired=40),
        "SLANE2": lambda: TB.split_config(20_000, seed=0x6A, good=15, expired=40),
        "ALL_BAD": TB.all_bad_table,
        "OFFSET_FIRST": TB.offset_first_table,
        "U_three": lambda: TB.uniform_config(3, 1, seed=0x5EED + 3),  # a sorted map of S3's size
    }[cls]()


CLASSES = ("UW", "UW_dense", "UW_sparse", "U_tiny", "SG", "SG2", "SLANE", "SLANE2", "S3", "S257", "EMPTY_B1",
           "EMPTY_B0", "NONE", "ALL_BAD", "TIES48", "DUPS", "OFFSET_FIRST", "CLUSTERED", "U_three")


@functools.lru_cache(maxsize=None)
def table(cls):
    t = _build(cls)
    if t is not None:
        t = dict(t, name=cls)
    return t


_UNIFORM = dict(window=True, short=True, rt16=True, rt32=True, nc16=True, nc32=True)
_GENERAL = dict(window=False, gl=True, gl16=True, gl32=True, sl=True, sl16=True)
_LANE = dict(window=False, gl=False, gl16=False, gl32=False, sl=False, sl16=False)
# what a class must carry after prepare() (keys of `state`); classes not listed are recorded, not required
MUST_CARRY = {
    "UW": _UNIFORM, "UW_dense": _UNIFORM, "UW_sparse": _UNIFORM,
    "SG": _GENERAL, "SG2": _GENERAL, "SLANE": _LANE, "SLANE2": _LANE,
    "EMPTY_B1": dict(B=1, n=0), "EMPTY_B0": dict(B=0, n=0),
    "CLUSTERED": dict(nc16=True, nc32=True),
}


def state(info):
    """A family's dispatch-relevant state from DeviceTable.info() after prepare(); None for a missing family. The
    uniform tables' count 9..16 / 17..32 lines and the 256-byte NodeCache lines have no info flag of their own: a
    built set on a table with window lines (a sorted non-empty table) is that flag, short of an allocation failure."""
    if info is None:
        return dict(B=0, n=0, window=False, short=False, gl=False, gl16=False, gl32=False, sl=False, sl16=False,
                    wl16=False, wl32=False, ncl=False, ncl32=False, rt16=False, rt32=False, nc16=False, nc32=False)
    f, ls = info["flags"], info["line_sets"]
    s = dict(B=info["n_buckets"], n=info["n_nodes"], window=bool(f & KAD_INFO_WINDOW_LINES),
             short=bool(f & KAD_INFO_SHORT_LINES), gl=bool(f & KAD_INFO_GENERAL_LINES),
             gl16=bool(f & KAD_INFO_GENERAL_LINES16), gl32=bool(f & KAD_INFO_GENERAL_LINES32),
             sl=bool(f & KAD_INFO_SLOT_LINES), sl16=bool(f & KAD_INFO_SLOT_LINES16),
             ncl32=bool(f & KAD_INFO_NODECACHE_LINES32), **{k: v["built"] for k, v in ls.items()})
    s["wl16"] = s["window"] and s["rt16"]
    s["wl32"] = s["window"] and s["rt32"]
    s["ncl"] = s["ncl32"] or (s["nc16"] and ls["nc16"]["bytes"] > 0)
    return s


def rt_launch(s4, s6, count):
    """kad_rt_closest_batch_dual's choice (kad_engine.hip) for two family states and a count >= 1."""
    def any_(k):
        return s4[k] or s6[k]

    def lean(k):  # every family has the set or is empty
        return (s4["B"] == 0 or s4[k]) and (s6["B"] == 0 or s6[k])

    if count > 32:
        return "rt_wave_kernel"
    if count <= 8:
        if any_("window"):
            return "rt_dual_wl_lean_kernel" if lean("window") else "rt_dual_wl_kernel"
        if any_("sl") and lean("sl"):
            return "rt_dual_sl_kernel"
        return "rt_dual_gl_kernel<8>" if any_("gl") else "launch_rt_dual<8>"
    if count <= 16:
        if any_("wl16"):
            return "rt_dual_wl16_kernel<true>" if lean("wl16") else "rt_dual_wl16_kernel<false>"
        if any_("sl16") and lean("sl16"):
            return "rt_dual_sl16_kernel"
        return "rt_dual_gl_kernel<16>" if any_("gl16") else "launch_rt_dual<16>"
    quad = count >= 24 and count % 4 == 0
    if any_("wl32"):
        if lean("wl32"):
            return "rt_dual_wl32q_kernel<false>" if quad else "rt_dual_wl32_kernel<true>"
        return "rt_dual_wl32_kernel<false>"
    if any_("gl32"):
        return "rt_dual_wl32q_kernel<true>" if quad and lean("gl32") else "rt_dual_gl_kernel<32>"
    return "launch_rt_dual<32>"


def nc_launch(s4, s6, count):
    """kad_nc_closest_batch_dual's choice for two family states and a count >= 1."""
    if count <= NCL2_COUNT_MAX:
        return "ncl2_lane_kernel<0,true>"
    if count <= 16:
        return "nc_line_kernel<0,true,false>"
    if count <= 32 and (s4["ncl32"] or s6["ncl32"]):
        return "nc32_line_kernel<0,true>"
    return "nc_two_pass_dual_kernel" if count <= 64 else "nc_closest_dual_kernel"


# ---- pair list: one line per dispatch branch ----------------------------------------------------------------------
# (family 4, family 6, first count, last count, the launch those counts take). Every pair runs every count of
# RT_COUNTS / NC_COUNTS in both orders; the lines say which branch each range of a pair is in the list for, and the
# GPU test holds the tables it built to them.
Branch = namedtuple("Branch", "fam4 fam6 lo hi launch")

_Q = (24, 28, 32)  # the quad kernels' counts


def _uniform_lean(a, b):
    return [Branch(a, b, 1, 8, "rt_dual_wl_lean_kernel"), Branch(a, b, 9, 16, "rt_dual_wl16_kernel<true>"),
            Branch(a, b, 17, 23, "rt_dual_wl32_kernel<true>"), Branch(a, b, 24, 32, "rt_dual_wl32q_kernel<false>"),
            Branch(a, b, 25, 31, "rt_dual_wl32_kernel<true>"), Branch(a, b, 33, 300, "rt_wave_kernel")]


def _uniform_mixed(a, b):
    return [Branch(a, b, 1, 8, "rt_dual_wl_kernel"), Branch(a, b, 9, 16, "rt_dual_wl16_kernel<false>"),
            Branch(a, b, 17, 32, "rt_dual_wl32_kernel<false>"), Branch(a, b, 33, 300, "rt_wave_kernel")]


def _slot(a, b):
    return [Branch(a, b, 1, 8, "rt_dual_sl_kernel"), Branch(a, b, 9, 16, "rt_dual_sl16_kernel"),
            Branch(a, b, 17, 23, "rt_dual_gl_kernel<32>"), Branch(a, b, 24, 32, "rt_dual_wl32q_kernel<true>"),
            Branch(a, b, 25, 31, "rt_dual_gl_kernel<32>"), Branch(a, b, 33, 300, "rt_wave_kernel")]


def _general_lane(a, b):
    return [Branch(a, b, 1, 8, "rt_dual_gl_kernel<8>"), Branch(a, b, 9, 16, "rt_dual_gl_kernel<16>"),
            Branch(a, b, 17, 32, "rt_dual_gl_kernel<32>"), Branch(a, b, 33, 300, "rt_wave_kernel")]


def _lane(a, b):
    return [Branch(a, b, 1, 8, "launch_rt_dual<8>"), Branch(a, b, 9, 16, "launch_rt_dual<16>"),
            Branch(a, b, 17, 32, "launch_rt_dual<32>"), Branch(a, b, 33, 300, "rt_wave_kernel")]


def branch_counts(br, counts):
    """The counts of `counts` a branch line stands for: a quad line (24..32) its multiples of four, the 25..31 line
    beside it the others."""
    quad = br.launch.startswith("rt_dual_wl32q")
    return tuple(k for k in counts if br.lo <= k <= br.hi and (not quad or k in _Q)
                 and not (br.lo == 25 and br.hi == 31 and k in _Q))


RT_BRANCHES = (
    # LEAN uniform kernels: both families with the lines, or one of them missing / without a bucket
    _uniform_lean("UW", "UW_dense") + _uniform_lean("UW", "UW_sparse") + _uniform_lean("UW", "NONE")
    + _uniform_lean("UW", "EMPTY_B0")
    # non-lean uniform kernels: the other family answers on the lane path and its own exact tail
    + _uniform_mixed("UW", "SG") + _uniform_mixed("UW", "SLANE") + _uniform_mixed("UW", "EMPTY_B1")
    + _uniform_mixed("UW", "S3") + _uniform_mixed("S257", "ALL_BAD")
    # slot-line kernels and the general-line quad kernel; the tiny split tables and a table of one empty bucket
    # carry every general line set too (no line of theirs is deferred)
    + _slot("SG", "SG2") + _slot("SG", "S257") + _slot("S3", "EMPTY_B1")
    # general lines beside a lane-only family
    + _general_lane("SG", "SLANE") + _general_lane("S257", "SLANE")
    # neither family has lines (a missing family: the lane path's own empty rows)
    + _lane("SLANE", "SLANE2") + _lane("SLANE", "NONE")
    # ties, duplicate IDs, a first bucket above zero, a five-node table
    + _uniform_lean("TIES48", "DUPS") + _uniform_lean("OFFSET_FIRST", "UW") + _uniform_lean("U_tiny", "UW_dense")
)


def _nc(a, b, lines32=True):
    return [Branch(a, b, 1, 14, "ncl2_lane_kernel<0,true>"), Branch(a, b, 15, 16, "nc_line_kernel<0,true,false>"),
            Branch(a, b, 17, 32, "nc32_line_kernel<0,true>" if lines32 else "nc_two_pass_dual_kernel"),
            Branch(a, b, 33, 64, "nc_two_pass_dual_kernel"), Branch(a, b, 65, 300, "nc_closest_dual_kernel")]


NC_BRANCHES = (_nc("UW", "UW_sparse") + _nc("UW", "CLUSTERED") + _nc("UW", "TIES48") + _nc("UW", "NONE")
               + _nc("UW", "EMPTY_B0") + _nc("U_tiny", "UW_dense") + _nc("U_three", "UW"))


def pairs(branches):
    """The (fam4, fam6) pairs of a branch list in list order, each followed by its swap."""
    out = []
    for br in branches:
        for p in ((br.fam4, br.fam6), (br.fam6, br.fam4)):
            if p not in out:
                out.append(p)
    return out


def branches_of(branches, fam4, fam6):
    return [br for br in branches if (br.fam4, br.fam6) in ((fam4, fam6), (fam6, fam4))]


# the pairs that run once more with family 6 at index_base BASE6, the out_cnt == NULL pairs, the status-change pair
RT_BASE_PAIRS = (("UW", "UW_dense"), ("UW", "SG"), ("SG", "SG2"))
NC_BASE_PAIRS = (("UW", "UW_sparse"),)
NULL_CNT_PAIRS = (("UW", "SG"), ("SG", "SLANE"))
NULL_CNT_COUNTS = (8, 16, 27, 32)
STATUS_PAIR = ("UW", "SG")
STATUS_COUNTS = (5, 8, 14, 20, 32)


# ---- targets and the expected side --------------------------------------------------------------------------------
_EMPTY = TB.table(np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8), np.zeros((0, 20), np.uint8),
                  np.zeros(1, np.uint32), sorted_=True, name="NONE")


@functools.lru_cache(maxsize=None)
def class_targets(cls, extra=1024):
    """adversarial_targets of one catalogue table (node IDs, bucket bounds and their neighbours, 00..0, FF..F, random
    ones), and for the clustered map the targets inside its clusters."""
    t = table(cls) or _EMPTY
    parts = [TB.adversarial_targets(t, extra=extra)]
    if "near" in t:
        near = t["near"].copy()
        near[:, 19] ^= 0x5A
        parts.append(near)
    tg = np.ascontiguousarray(np.concatenate(parts), np.uint8)
    tg.setflags(write=False)
    return tg


def pair_targets(fam4, fam6):
    """Both families' adversarial targets, cut to an odd length (the last wave and workgroup are partial). Returns
    (targets, the part of family 4's class, the part of family 6's class) with the parts' lengths after the cut."""
    a, b = class_targets(fam4), class_targets(fam6)
    if (a.shape[0] + b.shape[0]) % 2 == 0:
        b = b[:-1]
    return np.ascontiguousarray(np.concatenate([a, b])), a.shape[0], b.shape[0]


def af_pattern(name, q):
    i = np.arange(q)
    if name == "alternating":
        af = i & 1
    elif name == "random":
        af = np.random.default_rng(0xAF).integers(0, 2, q)
    elif name == "runs64":
        af = (i >> 6) & 1
    elif name == "runs256":
        af = (i >> 8) & 1
    else:
        af = np.full(q, {"all0": 0, "all1": 1}[name])
    return af.astype(np.uint8)


def rows_len(rows):
    """Entries before the first KAD_NO_NODE of each row (the result length for count > 255)."""
    pad = rows == KAD_NO_NODE
    return np.where(pad.any(axis=1), pad.argmax(axis=1), rows.shape[1])


_oracle_cache = {}


def expected(kind, cls, tcls, count, status=None):
    """The oracle's rows of table `cls` for class_targets(tcls): flat_rt_closest (kind "rt") or flat_nc_closest
    ("nc"), computed once per (table, targets, count) and shared by every pair, order and af pattern that needs it.
    A missing family and a table without nodes give empty rows. `status` overrides the table's status (not cached).
    Returns rows only; the count byte is min(rows_len, 255)."""
    key = (kind, cls, tcls, count)
    if status is None and key in _oracle_cache:
        return _oracle_cache[key]
    t, tg = table(cls), class_targets(tcls)
    if t is None or t["ids"].shape[0] == 0:
        rows = np.full((tg.shape[0], count), KAD_NO_NODE, np.uint32)
    elif kind == "rt":
        rows, _ = O.flat_rt_closest(t["ids"], t["status"] if status is None else status, t["first"], t["off"], tg,
                                    count, nthreads=8)
    else:
        rows, _ = O.flat_nc_closest(t["ids"], t["status"] if status is None else status, tg, count, nthreads=8)
    if status is None and count <= 64:  # the few larger counts are cheaper to compute again than to hold
        rows.setflags(write=False)
        _oracle_cache[key] = rows
    return rows


def release():
    """Drop the cached oracle rows (a few hundred MB once every pair has run)."""
    _oracle_cache.clear()


def expected_pair(kind, cls, fam4, fam6, count, status=None):
    """The oracle's rows of table `cls` over pair_targets(fam4, fam6)."""
    _, n4, n6 = pair_targets(fam4, fam6)
    return np.concatenate([expected(kind, cls, fam4, count, status)[:n4], expected(kind, cls, fam6, count, status)[:n6]])
