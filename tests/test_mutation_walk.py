"""Every order of table mutations against a freshly built table. A DeviceTable created with every line set and a lazy
twin are walked through scripts of mutation steps (mutation_model.KINDS: kad_table_apply with and without splits and
in its removals-only form, kad_table_expire, whole-array and listed status updates on both sides of the 2,048-node
limit, set_times, refreshes passing 0, 1..128, 129..2,048 and more deadlines, patch_times, prepare, set_addrs) that the
CPU model of tests/mutation_model.py follows step by step. After every step the walked table must be what a table
created from the model's state is: the same info, the same exported arrays, every derived line set byte for byte,
and every query equal to the oracle and the project's restatements on the model's state.

The scripts together hold every ordered pair of kinds (X directly followed by Y, X not refused) on S3000 and on
U9_6000; patch_large and refresh_flag need more nodes than those tables can lose and run on the 24,000-node tables,
where the scripts hold their pairs with each other and with the structural kinds. (refresh_flag, refresh_flag) is the
one pair left out: two refreshes past more than 2,048 deadlines each take over 17 % of 24,000 nodes' good bits, which
the model's floor of 85 % good nodes forbids. A refresh or patch_times is refused only directly after the apply that
dropped the node times. An expire removes at least one node, except directly after another expire, where it must remove
none. The scripts were written once against the model and are fixed; test_scripts_hold_on_the_model_and_cover_every_pair
checks all of this on the model alone."""
import functools

import numpy as np
import pytest
import torch

import mutation_model as M
import oracle as O
import sweep_ref as R
import tables as TB
import triage_ref
from opendht_amd import DeviceTable, KadError
from opendht_amd import synth as S
from opendht_amd._lib import (KAD_INFO_GENERAL_LINES, KAD_INFO_GENERAL_LINES16, KAD_INFO_GENERAL_LINES32,
                              KAD_INFO_SLOT_LINES, KAD_INFO_SLOT_LINES16, KAD_LINESET_GL, KAD_LINESET_GL16,
                              KAD_LINESET_GL32, KAD_LINESET_NCL, KAD_LINESET_NCL32, KAD_LINESET_SL, KAD_LINESET_SL16,
                              KAD_SERVE_MAX_Q)
from test_responsible import expected as responsible_expected

LINESETS = range(13)
# kad_engine.hip, comment above count_deferred: a general-line set is kept only when at most 1/16 of its lines are
# deferred at build time, so a walked table may still hold a set (built on an earlier status) that a fresh build on
# the current status declines; the reverse, and any other set, must agree
GENERAL = {KAD_LINESET_GL: KAD_INFO_GENERAL_LINES, KAD_LINESET_GL16: KAD_INFO_GENERAL_LINES16,
           KAD_LINESET_GL32: KAD_INFO_GENERAL_LINES32, KAD_LINESET_SL: KAD_INFO_SLOT_LINES,
           KAD_LINESET_SL16: KAD_INFO_SLOT_LINES16}
SMALL = tuple(k for k in M.KINDS if k not in M.BIG_ONLY)
APPLY = ("apply_mix", "apply_split", "apply_removals")
SELF = np.random.default_rng(0x5E1F).integers(0, 256, size=20, dtype=np.uint8)

# (model seed, kinds): on S3000 and on U9_6000
SCRIPTS_SMALL = (
    (0, ("set_times", "patch_times", "set_times", "patch_small", "prepare", "patch_times", "prepare", "update_status",
         "set_addrs", "set_times", "refresh_small", "patch_times", "patch_times", "refresh_inline", "refresh_none",
         "patch_times", "patch_small", "update_status", "apply_mix", "set_times", "expire", "apply_removals",
         "apply_split", "set_times")),
    (1, ("set_times", "apply_split", "refresh_small", "set_times", "apply_removals", "set_times", "refresh_inline",
         "expire", "expire", "set_addrs", "prepare", "prepare", "apply_split", "apply_split", "refresh_inline",
         "set_times", "refresh_none", "refresh_none", "prepare", "apply_mix", "refresh_inline", "set_times",
         "update_status", "refresh_none")),
    (2, ("set_times", "set_addrs", "update_status", "expire", "patch_small", "patch_small", "apply_split",
         "patch_small", "set_times", "set_times", "apply_mix", "apply_mix", "apply_split", "update_status",
         "set_times", "prepare", "apply_removals", "update_status", "apply_split", "apply_removals", "apply_removals",
         "prepare", "set_times", "patch_times")),
    (3, ("set_times", "expire", "prepare", "refresh_none", "set_addrs", "apply_mix", "refresh_small", "set_times",
         "refresh_inline", "prepare", "refresh_small", "apply_removals", "set_addrs", "apply_split", "patch_times",
         "set_times", "refresh_inline", "update_status", "refresh_inline", "set_addrs", "refresh_small", "expire",
         "apply_split", "refresh_none")),
    (4, ("set_times", "patch_times", "refresh_none", "refresh_inline", "refresh_inline", "apply_split", "prepare",
         "set_addrs", "patch_small", "set_addrs", "apply_removals", "refresh_inline", "set_times", "patch_small",
         "apply_mix", "refresh_none", "set_times", "refresh_none", "apply_removals", "refresh_none", "set_times",
         "expire", "refresh_none", "apply_split")),
    (5, ("set_times", "refresh_none", "apply_mix", "set_addrs", "expire", "set_times", "patch_small",
         "refresh_inline", "refresh_small", "update_status", "prepare", "expire", "patch_times", "apply_mix",
         "expire", "apply_mix", "apply_removals", "apply_mix", "update_status", "patch_small", "apply_removals",
         "patch_times", "apply_split", "apply_mix")),
    (6, ("set_times", "refresh_inline", "apply_mix", "patch_small", "expire", "update_status", "update_status",
         "apply_removals", "patch_small", "set_times", "patch_times", "refresh_small", "refresh_inline",
         "patch_small", "refresh_none", "update_status", "patch_times", "set_addrs", "patch_times", "apply_split",
         "set_addrs", "set_addrs", "set_times", "refresh_small")),
    (7, ("set_times", "refresh_none", "refresh_small", "refresh_none", "patch_small", "patch_times", "expire",
         "refresh_small", "set_addrs", "refresh_inline", "apply_removals", "refresh_small", "set_times",
         "refresh_small", "prepare", "patch_small", "refresh_none", "expire", "refresh_inline", "patch_times",
         "apply_removals", "expire", "apply_split", "expire")),
    (8, ("set_times", "refresh_small", "apply_mix", "patch_times", "set_times", "refresh_small", "patch_small",
         "refresh_small", "apply_split", "set_times", "refresh_small", "refresh_small", "set_times", "prepare",
         "refresh_inline", "set_times", "refresh_none", "set_times", "patch_times", "update_status", "refresh_small",
         "set_addrs", "apply_removals", "set_times")),
    (9, ("set_times", "apply_mix", "prepare", "set_times", "set_addrs", "refresh_none", "apply_split", "apply_mix",
         "refresh_small", "update_status", "set_addrs", "set_addrs", "set_times", "set_times", "patch_small",
         "update_status", "apply_split", "update_status", "prepare", "apply_mix", "set_addrs", "prepare",
         "apply_removals", "apply_split")),
)
# on S24000 and on U11_24000
SCRIPTS_BIG = (
    (100, ("set_times", "refresh_flag", "patch_large", "patch_large", "apply_mix", "refresh_flag", "set_times",
           "refresh_flag", "apply_split", "patch_large", "apply_removals", "patch_large", "expire", "patch_large")),
    (101, ("set_times", "refresh_flag", "apply_mix", "patch_large", "apply_split", "refresh_flag", "set_times",
           "refresh_flag", "apply_removals", "refresh_flag", "set_times", "refresh_flag", "expire", "expire")),
    (102, ("set_times", "patch_large", "refresh_flag", "expire", "expire", "set_addrs", "prepare", "patch_times",
           "refresh_inline", "update_status", "apply_removals", "apply_split", "set_times", "refresh_small")),
    (103, ("set_times", "expire", "refresh_flag", "patch_small", "apply_split", "patch_small", "update_status",
           "update_status", "set_times", "refresh_none", "apply_split", "apply_removals", "refresh_flag",
           "apply_removals")),
)
SCRIPTS_OTHER = {
    "S3000nosl": SCRIPTS_SMALL[:2],
    "ties": (
        (200, ("set_times", "patch_times", "set_times", "patch_small", "prepare", "patch_times", "prepare",
               "update_status", "set_addrs", "set_times", "refresh_none", "patch_times", "patch_times",
               "refresh_inline", "refresh_none", "prepare", "patch_small", "update_status", "apply_mix", "set_times",
               "expire", "apply_removals", "apply_split", "set_times")),
        (201, ("set_times", "apply_split", "refresh_small", "set_times", "apply_removals", "set_times",
               "refresh_inline", "expire", "expire", "set_addrs", "prepare", "prepare", "apply_split", "apply_split",
               "refresh_inline", "set_times", "set_addrs", "refresh_none", "refresh_none", "apply_mix",
               "refresh_inline", "set_times", "update_status", "refresh_none")),
    ),
    "offset_first": (
        (200, ("set_times", "patch_times", "set_times", "patch_small", "prepare", "patch_times", "prepare",
               "update_status", "set_addrs", "set_times", "refresh_none", "patch_times", "patch_times",
               "refresh_inline", "refresh_none", "prepare", "patch_small", "update_status", "apply_mix", "set_times",
               "expire", "apply_removals", "apply_split", "set_times")),
        # 2.9 nodes per bucket: once it holds general lines their deferred share sits at the 1/16 limit and any status
        # change tips it, so this script does its status work on the window-line table and splits near its end
        (204, ("set_times", "refresh_inline", "set_addrs", "patch_times", "prepare", "expire", "update_status",
               "patch_small", "set_times", "refresh_none", "apply_removals", "set_times", "refresh_inline", "patch_times",
               "expire", "set_addrs", "update_status", "set_times", "refresh_none", "prepare", "apply_mix", "apply_split",
               "set_times", "refresh_none")),
    ),
    "one_empty_bucket": (  # the fresh Dht table: everything it holds was inserted and split from empty
        (200, ("apply_split", "set_times", "set_times", "patch_small", "prepare", "patch_times", "prepare",
               "update_status", "set_addrs", "set_times", "refresh_none", "patch_times", "patch_times", "set_times",
               "apply_mix", "set_times", "patch_times", "update_status", "apply_mix", "update_status", "set_times",
               "expire", "apply_removals", "set_times")),
        (201, ("apply_split", "apply_split", "set_times", "update_status", "expire", "set_times", "set_addrs", "prepare",
               "patch_small", "refresh_none", "patch_times", "patch_times", "apply_removals", "apply_split", "set_times",
               "refresh_none", "patch_small", "set_addrs", "expire", "apply_mix", "apply_split", "set_times", "prepare",
               "apply_removals")),
    ),
}
WALK_SEEDS = (0xA1, 0xA2, 0xA3)
SERVED = {"S3000": 4, "U9_6000": 6}  # the script that also runs with the resident service on


@functools.lru_cache(maxsize=None)
def table(name):
    """(table, slot_lines); built once, never changed (the model copies what it mutates)."""
    if name == "S3000":
        return TB.split_config(3000, seed=0x3131), True
    if name == "S3000nosl":
        return dict(TB.split_config(3000, seed=0x3131), name="S3000nosl"), False
    if name == "U9_6000":
        return TB.uniform_config(6000, 9, seed=0x3132), True
    if name == "ties":
        return TB.tie_table()[0], True
    if name == "offset_first":
        return TB.offset_first_table(), True
    if name == "one_empty_bucket":
        return TB.tiny_tables()[1], True
    if name == "S24000":
        return TB.split_config(24000), True
    if name == "U11_24000":
        return TB.uniform_config(24000, 11), True
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cases():
    """{id: (table name, model seed, kinds, served)}."""
    out = {}
    for name in ("S3000", "U9_6000"):
        for j, (seed, kinds) in enumerate(SCRIPTS_SMALL):
            out[f"{name}-s{j}"] = (name, seed, kinds, False)
        for seed in WALK_SEEDS:
            out[f"{name}-walk{seed:x}"] = (name, seed, M.random_walk(table(name)[0], seed), False)
        seed, kinds = SCRIPTS_SMALL[SERVED[name]]
        out[f"{name}-s{SERVED[name]}-served"] = (name, seed, kinds, True)
    for name in ("S24000", "U11_24000"):
        for j, (seed, kinds) in enumerate(SCRIPTS_BIG):
            out[f"{name}-b{j}"] = (name, seed, kinds, False)
    for name, scripts in SCRIPTS_OTHER.items():
        for j, (seed, kinds) in enumerate(scripts):
            out[f"{name}-o{j}"] = (name, seed, kinds, False)
    return out


def live_pairs(kinds, steps):
    """The ordered pairs of a script whose first step was not refused."""
    return {(a, b) for a, b, s in zip(kinds[:-1], kinds[1:], steps[:-1]) if s["raises"] is None}


def test_scripts_hold_on_the_model_and_cover_every_pair():
    """Passes on the model alone. Every script keeps the refresh bands, the 85 % floor and the expire rule
    (mutation_model.checked_step), holds at least one split and one removal that empties a bucket, is refused only
    directly after an apply, and has at most 24 steps (walks: 30). The hand-written scripts hold every ordered pair of
    the 13 kinds on S3000 and on U9_6000, and on each 24k table every pair of patch_large / refresh_flag with each
    other and with the structural kinds but (refresh_flag, refresh_flag)."""
    pairs = {}
    for cid, (name, seed, kinds, served) in cases().items():
        assert len(kinds) <= (30 if "walk" in cid else 24), cid
        assert all(k in M.KINDS for k in kinds), cid
        _, steps, shares = M.run_script(table(name)[0], kinds, seed)
        assert sum(s.get("splits", 0) for s in steps) >= 1, f"{cid}: no split"
        assert sum(s.get("emptied", 0) for s in steps if s["kind"] != "expire") >= 1, f"{cid}: no bucket emptied"
        for j, s in enumerate(steps):
            if s["raises"] is not None and "walk" not in cid:
                assert j and kinds[j - 1] in APPLY, f"{cid} step {j}: {s['kind']} refused without an apply before it"
        assert any(x is not None for x in shares), cid
        if "walk" not in cid:
            pairs.setdefault(name, set()).update(live_pairs(kinds, steps))
    want = {(a, b) for a in SMALL for b in SMALL}
    for name in ("S3000", "U9_6000"):
        assert not want - pairs[name], (name, sorted(want - pairs[name]))
    want = set()
    for b in M.BIG_ONLY:
        for s in M.STRUCTURAL + M.BIG_ONLY:
            want |= {(b, s), (s, b)}
    want.discard(("refresh_flag", "refresh_flag"))
    for name in ("S24000", "U11_24000"):
        assert not want - pairs[name], (name, sorted(want - pairs[name]))
    for name, scripts in SCRIPTS_OTHER.items():
        assert len(scripts) == 2, name


# ---- the device side --------------------------------------------------------------------------------------------------
def _u32(x):
    return x.cpu().numpy().view(np.uint32)


def _open(m, slot_lines, gpu, eager):
    return DeviceTable(m.ids, m.status, m.first, m.off, device=gpu.index or 0, sorted=m.sorted, eager=eager,
                       slot_lines=slot_lines)


def perform(T, s, gpu, sync=True):
    """The step's calls on one device table, with what they return checked against the model. sync=False: no
    device-wide wait afterwards (it would only return once a resident service launch has gone idle and ended)."""
    if s["raises"] is not None:
        name, args = s["calls"][0]
        with pytest.raises(KadError) as e:
            getattr(T, name)(*args)
        assert s["raises"] in str(e.value)
        return
    for name, args in s["calls"]:
        if name == "apply":
            remap = torch.full((max(s["n_old"], 1),), 0x55555555, dtype=torch.int32, device=gpu)
            new = T.apply(*args, remap=remap)
            np.testing.assert_array_equal(_u32(remap)[:s["n_old"]], s["remap"], err_msg="apply remap")
            np.testing.assert_array_equal(new, s["new_index"], err_msg="apply new indices")
        elif name == "expire":
            remap = np.full(max(s["n_old"], 1), 0x55555555, np.uint32)
            removed, buckets = T.expire(remap=remap)
            np.testing.assert_array_equal(removed, s["removed"], err_msg="expire removed")
            np.testing.assert_array_equal(buckets, s["buckets"], err_msg="expire buckets")
            np.testing.assert_array_equal(remap[:s["n_old"]], s["remap"], err_msg="expire remap")
        else:
            getattr(T, name)(*args)
    if sync:
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _near():
    """Targets sharing every prefix length with SELF (the responsibility verdict flips around them), and SELF."""
    near = triage_ref.near_targets(SELF, np.random.default_rng(0xBA7C), copies=1)
    return np.concatenate([near, SELF.reshape(1, 20)])


def targets_of(t):
    return np.ascontiguousarray(np.concatenate([TB.adversarial_targets(t, extra=256), _near()]), np.uint8)


def served_rows(T, targets, k):
    parts = [T.rt_closest_host(targets[i:i + KAD_SERVE_MAX_Q], k) for i in range(0, targets.shape[0], KAD_SERVE_MAX_Q)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def check_rows(T, t, targets, tg, counts, what, host=False):
    """rt_closest of every count against the oracle; returns the oracle's (rows, cnt) per count."""
    out = {}
    for k in counts:
        want, wcnt = O.flat_rt_closest(t["ids"], t["status"], t["first"], t["off"], targets, k, nthreads=8)
        if host:
            idx, cnt = served_rows(T, targets, k)
        else:
            idx, cnt = T.rt_closest(tg, k)
            torch.cuda.synchronize()
            idx, cnt = _u32(idx), cnt.cpu().numpy()
        np.testing.assert_array_equal(cnt, wcnt, err_msg=f"{what} rt k={k} counts")
        np.testing.assert_array_equal(idx, want, err_msg=f"{what} rt k={k}")
        out[k] = (want, wcnt)
    return out


def check_verdicts(T, t, targets, tg, rows8, what):
    """rt_responsible (count 8, min_nodes 1 and 8) and rt_triage (bootstrap off and on, with the bucket)."""
    for mn in (1, 8):
        want = responsible_expected(t["ids"], targets, rows8[0], rows8[1], SELF, mn)
        got = T.rt_responsible(tg, SELF, 8, mn)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"{what} responsible min_nodes={mn}")
    facts = triage_ref.BucketFacts(t)
    bucket = triage_ref.find_bucket(t, targets)
    kind, node = triage_ref.base_verdicts(t, facts, targets, bucket)
    for boot in (False, True):
        wv, wn, wb = triage_ref.finish(t, facts, kind, node, bucket, SELF, boot)
        v, nd, b = T.rt_triage(tg, SELF, bootstrap=boot, want_bucket=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(v.cpu().numpy(), wv, err_msg=f"{what} triage verdict bootstrap={boot}")
        np.testing.assert_array_equal(_u32(nd), wn, err_msg=f"{what} triage node bootstrap={boot}")
        np.testing.assert_array_equal(_u32(b), wb, err_msg=f"{what} triage bucket bootstrap={boot}")
    return bucket


def check_eager(T, m, slot_lines, gpu, what):
    """The walked eager table against the model and a fresh build of it; returns whether the general-line presence
    exception was used."""
    t = m.table()
    for got, want, part in zip(T.export(), (m.ids, m.status, m.first, m.off), ("ids", "status", "firsts", "offsets")):
        bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(1)) if got.shape == want.shape else None
        assert bad is not None and bad.size == 0, (what, part, got.shape, want.shape, None if bad is None else bad[:8],
                                                   None if bad is None else (got[bad[:8]], want[bad[:8]]))
    T.prepare()
    mask = 0
    with _open(m, slot_lines, gpu, True) as F:
        for w in LINESETS:
            a, b = T.export_lines(w), F.export_lines(w)
            if a is not None and b is None and w in GENERAL:
                mask |= GENERAL[w]
                continue
            assert (a is None) == (b is None), f"{what}: line set {w} present in {'walked' if b is None else 'fresh'} only"
            if a is not None:
                np.testing.assert_array_equal(a, b, err_msg=f"{what}: line set {w}")
        ia, ib = T.info(), F.info()
    for k in ("n_nodes", "n_buckets", "n_good"):
        assert ia[k] == ib[k], (what, k, ia[k], ib[k])
    assert ia["n_good"] == int((m.status & 1).sum())
    assert ia["flags"] & ~mask == ib["flags"] & ~mask, (what, hex(ia["flags"]), hex(ib["flags"]))
    # queries
    targets = targets_of(t)
    tg = torch.from_numpy(targets).to(gpu)
    rows = check_rows(T, t, targets, tg, (1, 8, 9, 16, 17, 32, 40), what)
    idx, cnt = T.rt_closest_host(targets, 8)
    np.testing.assert_array_equal(idx, rows[8][0], err_msg=f"{what} host k=8")
    np.testing.assert_array_equal(cnt, rows[8][1], err_msg=f"{what} host k=8 counts")
    bucket = check_verdicts(T, t, targets, tg, rows[8], what)
    np.testing.assert_array_equal(_u32(T.find_bucket(tg)), bucket, err_msg=f"{what} find_bucket")
    has_times = m.times is not None
    got = T.sweep(incoming=has_times)
    want = R.sweep_ref(t, time_ns=m.times[0] if has_times else None, reply_ns=m.times[1] if has_times else None)
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    np.testing.assert_array_equal(_u32(got["expired_nodes"]), want["expired_nodes"], err_msg=f"{what} sweep nodes")
    np.testing.assert_array_equal(_u32(got["changed_buckets"]), want["changed_buckets"], err_msg=f"{what} sweep buckets")
    d_idx = torch.from_numpy(rows[8][0].view(np.int32)).to(gpu)
    d_cnt = torch.from_numpy(rows[8][1]).to(gpu)
    if m.addrs is not None:
        out, nn = T.buffer_nodes(tg, d_idx, d_cnt)
        torch.cuda.synchronize()
        want_out, want_n = O.buffer_nodes(targets, m.ids, m.addrs, rows[8][0], rows[8][1])
        np.testing.assert_array_equal(nn.cpu().numpy(), want_n, err_msg=f"{what} buffer_nodes counts")
        np.testing.assert_array_equal(out.cpu().numpy(), want_out, err_msg=f"{what} buffer_nodes")
    elif hasattr(T, "addr_len"):  # the wire records went with an apply: no records come back
        with pytest.raises(KadError) as e:
            T.buffer_nodes(tg, d_idx, d_cnt)
        assert M.NO_ADDRS in str(e.value)
    if m.sorted:
        for k in (14, 32):
            idx, cnt = T.nc_closest(tg, k)
            torch.cuda.synchronize()
            want, wcnt = O.flat_nc_closest(m.ids, m.status, targets, k, nthreads=8)
            np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt, err_msg=f"{what} nc k={k} counts")
            np.testing.assert_array_equal(_u32(idx), want, err_msg=f"{what} nc k={k}")
    return mask != 0


def check_twin(T, m, gpu, what, host=False):
    t = m.table()
    targets = targets_of(t)
    tg = torch.from_numpy(targets).to(gpu)
    rows = check_rows(T, t, targets, tg, (8, 14, 32), what, host=host)
    check_verdicts(T, t, targets, tg, rows[8], what)


def lines_of(T):
    return [T.export_lines(w) for w in LINESETS]


def same_lines(a, b, what):
    for w, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), f"{what}: line set {w} appeared or went"
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: line set {w}")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(cases()))
def test_walk(gpu, cid):
    name, seed, kinds, served = cases()[cid]
    t, slot_lines = table(name)
    m = M.Model(t, seed)
    used = []
    with _open(m, slot_lines, gpu, True) as T, _open(m, slot_lines, gpu, False) as twin:
        if served:
            twin.serve(20_000)
        for j, kind in enumerate(kinds):
            s = M.checked_step(m, kind, kinds[j - 1] if j else None)
            what = f"{cid} step {j} {kind}"
            still = s.get("unchanged") or s["raises"] is not None  # nothing may change on the device
            if still:
                before = (lines_of(T), lines_of(twin))
                if served:
                    served_rows(twin, t["ids"][:1] if t["ids"].shape[0] else np.zeros((1, 20), np.uint8), 8)
                    launches = twin.serve_stats()["launches"]
            if not served:
                perform(T, s, gpu)
            perform(twin, s, gpu, sync=not (served and still))
            if still:
                if served:  # the running launch was not ended: the next request finds it
                    served_rows(twin, np.zeros((1, 20), np.uint8), 8)
                    assert twin.serve_stats()["launches"] == launches, what
                else:
                    same_lines(before[0], lines_of(T), what)
                same_lines(before[1], lines_of(twin), what + " (twin)")
            if served:  # every batch of at most 64 queries through the service, after every mutation
                check_twin(twin, m, gpu, what + " (served twin)", host=True)
                continue
            if check_eager(T, m, slot_lines, gpu, what):
                used.append(j)
            if j % 4 == 3 or j == len(kinds) - 1:
                check_twin(twin, m, gpu, what + " (twin)")
    print(f"general-line presence exception: {cid}: {len(used)} of {len(kinds)} steps {used}")
    if not served:
        if name.startswith("U"):
            assert not used, f"{cid}: steps {used} used the general-line presence exception"
        else:
            assert len(used) * 8 <= len(kinds), f"{cid}: steps {used} of {len(kinds)} used the general-line presence exception"


# ---- NodeCache-only table ---------------------------------------------------------------------------------------------
def _nc_insert(rng, ids, keep, m):
    """m new IDs, a quarter of them next to kept ones, none a kept key."""
    new = S.random_ids(m, int(rng.integers(1, 1 << 30)))
    kept = ids[keep]
    if kept.shape[0]:
        near = kept[rng.choice(kept.shape[0], size=m // 4)].copy()
        near[:, 15:] = rng.integers(0, 256, (near.shape[0], 5), dtype=np.uint8)
        new = np.concatenate([new, near])
    have = {bytes(r) for r in kept}
    out = []
    for r in new:
        if bytes(r) not in have:
            have.add(bytes(r))
            out.append(r)
    return np.array(out, np.uint8).reshape(-1, 20)


def _nc_model_apply(ids, st, erase, ins, ist):
    keep = np.ones(ids.shape[0], bool)
    keep[erase] = False
    allk, alls = np.concatenate([ids[keep], ins]), np.concatenate([st[keep], ist])
    order = np.lexsort(allk.T[::-1]) if allk.shape[0] else np.zeros(0, np.int64)
    pos = np.empty(order.shape[0], np.int64)
    pos[order] = np.arange(order.shape[0])
    remap = np.full(ids.shape[0], 0xFFFFFFFF, np.uint32)
    remap[np.flatnonzero(keep)] = pos[:int(keep.sum())]
    return (np.ascontiguousarray(allk[order]).reshape(-1, 20), np.ascontiguousarray(alls[order]), remap,
            pos[int(keep.sum()):].astype(np.uint32))


@pytest.mark.gpu
def test_nodecache_walk(gpu):
    """A NodeCache-only table (no buckets, 20,000 sorted IDs, every line set built) through kad_nc_apply (erase and
    insert), update_status, patch_status of 7 nodes, prepare, and kad_nc_apply down to empty and back: after every step
    the NodeCache lines of both counts equal a fresh table's byte for byte and getCachedNodes equals the oracle for
    counts on both sides of every line width; set_times / refresh after kad_nc_apply is refused, as after
    kad_table_apply."""
    rng = np.random.default_rng(0x4E43)
    ids, _ = S.sort_ids(S.random_ids(20_000, 0x4E46))
    st = M.mostly_good(rng, ids.shape[0])
    script = ("nc_apply", "update_status", "nc_apply", "patch_small", "prepare", "nc_apply", "patch_small", "update_status",
              "prepare", "nc_apply", "nc_empty", "nc_refill", "update_status", "nc_apply")
    now = M.NOW0
    with DeviceTable(ids, st, device=gpu.index or 0, sorted=True, eager=True) as T:
        T.set_times(*M.draw_times(rng, ids.shape[0], now))  # the times the first kad_nc_apply drops
        for j, kind in enumerate(script):
            what = f"step {j} {kind}"
            n = ids.shape[0]
            if kind in ("nc_apply", "nc_empty", "nc_refill"):
                if kind == "nc_apply":
                    erase = np.sort(rng.choice(n, size=n // 50, replace=False)).astype(np.uint32)
                    keep = np.ones(n, bool)
                    keep[erase] = False
                    ins = _nc_insert(rng, ids, keep, n // 30)
                elif kind == "nc_empty":
                    erase, ins = np.arange(n, dtype=np.uint32), np.zeros((0, 20), np.uint8)
                    saved = ids
                else:
                    erase, ins = np.zeros(0, np.uint32), saved[rng.permutation(saved.shape[0])]
                ist = M.mostly_good(rng, ins.shape[0])
                ids, st, w_remap, w_new = _nc_model_apply(ids, st, erase, ins, ist)
                remap, new = T.nc_apply(erase, ins, ist)
                np.testing.assert_array_equal(remap, w_remap, err_msg=what)
                np.testing.assert_array_equal(new, w_new, err_msg=what)
                with pytest.raises(KadError) as e:
                    T.refresh_status(now + 1)
                assert M.NO_TIMES in str(e.value)
            elif kind == "update_status":
                nodes = rng.choice(n, size=n // 3, replace=False)
                st = st.copy()
                st[nodes] = M.mostly_good(rng, nodes.shape[0])
                T.update_status(st)
            elif kind == "patch_small":
                nodes = np.sort(rng.choice(n, size=7, replace=False)).astype(np.uint32)
                st = st.copy()
                st[nodes] = rng.choice(np.array([0, 1, 1, 2], np.uint8), size=7)
                T.patch_status(nodes, st[nodes])
            else:
                T.prepare()
            gids, gst, _, _ = T.export()
            np.testing.assert_array_equal(gids, ids, err_msg=what)
            np.testing.assert_array_equal(gst, st, err_msg=what)
            T.prepare()
            with DeviceTable(ids, st, device=gpu.index or 0, sorted=True, eager=True) as F:
                for w in (KAD_LINESET_NCL, KAD_LINESET_NCL32):
                    a, b = T.export_lines(w), F.export_lines(w)
                    assert (a is None) == (b is None), f"{what}: line set {w} present in one table only"
                    if a is not None:
                        np.testing.assert_array_equal(a, b, err_msg=f"{what}: line set {w}")
                assert T.info()["flags"] == F.info()["flags"], what
            targets = np.concatenate([rng.integers(0, 256, (256, 20), dtype=np.uint8), np.zeros((1, 20), np.uint8),
                                      np.full((1, 20), 255, np.uint8)] + ([ids[rng.choice(n2, 64)], ids[:1], ids[-1:]]
                                                                          if (n2 := ids.shape[0]) else []))
            tg = torch.from_numpy(np.ascontiguousarray(targets)).to(gpu)
            for k in (1, 14, 16, 17, 32, 64):
                idx, cnt = T.nc_closest(tg, k)
                torch.cuda.synchronize()
                want, wcnt = O.flat_nc_closest(ids, st, targets, k, nthreads=8)
                np.testing.assert_array_equal(cnt.cpu().numpy(), wcnt, err_msg=f"{what} k={k} counts")
                np.testing.assert_array_equal(_u32(idx), want, err_msg=f"{what} k={k}")
