"""CPU model of a DeviceTable walked through its mutation entry points (tests/test_mutation_walk.py): the state
{ids, status, first, off, sorted, times | None, addrs | None, now} and one function per step kind that returns the
arguments of the DeviceTable calls and advances the state. Structural steps go through the oracle's structure-faithful
list table (oracle.FaithfulTable.apply), expiry and isGood / isExpired through sweep_ref; the rest is numpy on the
status bytes. What the API documents as refused is part of the model: a refresh or patch_times on a table whose node
times a structural apply dropped raises "kad_table_set_times was not called" and changes nothing, and
kad_buffer_nodes_batch returns no records once the wire records are gone. No step passes invalid arguments.
Nothing here touches the GPU."""
from __future__ import annotations

import copy

import numpy as np

import oracle as O
import sweep_ref as R
from opendht_amd._lib import KAD_OP_INSERT, KAD_OP_REMOVE, KAD_OP_REPLACE, KAD_OP_SPLIT

KINDS = ("apply_mix", "apply_split", "apply_removals", "expire", "update_status", "patch_small", "patch_large",
         "set_times", "refresh_none", "refresh_inline", "refresh_small", "refresh_flag", "patch_times", "prepare",
         "set_addrs")
BIG_ONLY = ("patch_large", "refresh_flag")          # need more than 2048 nodes to spare: the 24k tables
STRUCTURAL = ("apply_mix", "apply_split", "apply_removals", "expire")
NEEDS_TIMES = ("refresh_none", "refresh_inline", "refresh_small", "refresh_flag", "patch_times")
# nodes whose isGood deadline a refresh passes (kad_table_refresh_status: RF_INLINE = 128, RF_CAP = 2048)
BANDS = {"refresh_none": (0, 0), "refresh_inline": (1, 128), "refresh_small": (129, 2048), "refresh_flag": (2049, None)}
PASS = {"refresh_inline": (1, 2, 7, 60, 128), "refresh_small": (129, 200), "refresh_flag": (2049, 2200)}
FLOOR = 0.85                                        # good share once the statuses come from node times
NO_TIMES = "kad_table_set_times was not called"
NO_ADDRS = "kad_table_set_addrs was not called"
MINUTE = 60 * 10**9
NOW0 = 700 * 3600 * 10**9
N_OPS = 120


def random_ops(t, rng, n_ops, allow_split=True):
    """A random batch: removals, in-bucket replacements, insertions, splits (old nodes used once)."""
    n = t["ids"].shape[0]
    B = t["first"].shape[0]
    order = rng.permutation(n)
    used = 0
    ops, new_ids, new_st = [], [], []
    existing = {bytes(x) for x in t["ids"]}
    cur_B = B
    for _ in range(n_ops):
        r = rng.random()
        if r < 0.3 and used < n:
            ops.append((KAD_OP_REMOVE, int(order[used]), 0))
            used += 1
        elif r < 0.55 and used < n:
            a = int(order[used])
            used += 1
            nid = t["ids"][a].copy()
            nid[12:] = rng.integers(0, 256, 8, dtype=np.uint8)  # same bucket (depth <= 96)
            if bytes(nid) in existing:
                continue
            existing.add(bytes(nid))
            ops.append((KAD_OP_REPLACE, a, len(new_ids)))
            new_ids.append(nid)
            new_st.append(rng.integers(0, 3))
        elif r < 0.9 or not allow_split:
            nid = rng.integers(0, 256, 20, dtype=np.uint8)
            if bytes(nid) in existing:
                continue
            existing.add(bytes(nid))
            ops.append((KAD_OP_INSERT, len(new_ids), 0))
            new_ids.append(nid)
            new_st.append(rng.integers(0, 3))
        else:
            ops.append((KAD_OP_SPLIT, int(rng.integers(0, cur_B)), 0))
            cur_B += 1
    new_ids = np.array(new_ids, np.uint8).reshape(-1, 20)
    return np.array(ops, np.uint32).reshape(-1, 3), new_ids, np.array(new_st, np.uint8)


def mostly_good(rng, m):
    """m status bytes: 90 % good, 5 % dubious, 5 % expired."""
    return rng.choice(np.array([1, 0, 2], np.uint8), size=m, p=[0.9, 0.05, 0.05])


def draw_times(rng, n, now):
    """Node times that keep a table mostly good: heard within 9 minutes of `now`, replied within 110 minutes, 5 %
    expired; every other node is good at `now` and its deadline lies 1 to 10 minutes ahead."""
    time_ns = now - rng.integers(0, 9 * MINUTE, n)
    reply_ns = now - rng.integers(0, 110 * MINUTE, n)
    expired = (rng.random(n) < 0.05).astype(np.uint8)
    return time_ns.astype(np.int64), reply_ns.astype(np.int64), expired


class Model:
    def __init__(self, t, seed=0):
        self.name = t["name"]
        self.ids, self.status = t["ids"].copy(), t["status"].copy()
        self.first, self.off = t["first"].copy(), t["off"].copy()
        self.sorted = bool(t["sorted"])
        self.times = None       # (time_ns, reply_ns, expired) once set_times ran, until a structural apply
        self.addrs = None
        self.now = NOW0
        self.dl_valid = False   # the engine's sorted deadlines stand: the next refresh is an incremental one
        self.from_times = False  # a refresh has run since the last set_times: FLOOR applies from here on
        self.rng = np.random.default_rng(seed)

    def copy(self):
        return copy.deepcopy(self)

    @property
    def n(self):
        return self.ids.shape[0]

    @property
    def B(self):
        return self.first.shape[0]

    def table(self):
        return dict(ids=self.ids, status=self.status, first=self.first, off=self.off, sorted=self.sorted,
                    name=self.name)

    def good_share(self):
        return 1.0 if self.n == 0 else float((self.status & 1).sum()) / self.n

    def pending(self):
        """The deadlines `now` has not passed, ascending (node.cpp:34-40: good while now <= deadline)."""
        time_ns, reply_ns, expired = self.times
        d = np.minimum(time_ns + R.NODE_EXPIRE_NS, reply_ns + R.NODE_GOOD_NS)
        return np.sort(d[(expired == 0) & (d >= self.now)])

    # ---- steps: each returns {"kind", "calls": [(DeviceTable method, args)], ...expectations} ----------------------
    def step(self, kind):
        s = getattr(self, "_" + (kind if not kind.startswith("refresh_") else "refresh"))(kind)
        s["kind"] = kind
        s.setdefault("raises", None)
        return s

    def _structural(self, ops, nid, nst):
        w0 = np.diff(self.off.astype(np.int64))
        F = O.FaithfulTable(self.ids, self.status, self.first, self.off)
        try:
            ids, st, first, off, remap, new = F.apply(ops, nid, nst)
        finally:
            F.close()
        w1 = np.diff(off.astype(np.int64))
        emptied = int(((w0 > 0) & (w1 == 0)).sum()) if w0.shape == w1.shape else 0
        self.ids, self.status, self.first, self.off = ids, st, first, off
        return remap, new, emptied

    def _apply(self, ops, nid, nst):
        assert ops.shape[0] > 0
        n0 = self.n
        remap, new, emptied = self._structural(ops, nid, nst)
        self.sorted, self.times, self.addrs, self.dl_valid, self.from_times = False, None, None, False, False
        return {"calls": [("apply", (ops, nid, nst))], "remap": remap, "new_index": new, "n_old": n0,
                "emptied": emptied, "splits": int((ops[:, 0] == KAD_OP_SPLIT).sum())}

    def _apply_mix(self, kind):
        ops, nid, _ = random_ops(self.table(), self.rng, N_OPS, allow_split=False)
        return self._apply(ops, nid, mostly_good(self.rng, nid.shape[0]))

    def _apply_split(self, kind):
        ops, nid, _ = random_ops(self.table(), self.rng, N_OPS, allow_split=True)
        if not (ops[:, 0] == KAD_OP_SPLIT).any():
            ops = np.concatenate([ops, np.array([[KAD_OP_SPLIT, int(self.rng.integers(0, self.B)), 0]], np.uint32)])
        return self._apply(ops, nid, mostly_good(self.rng, nid.shape[0]))

    def _apply_removals(self, kind):
        """Ascending REMOVE rows only: every node of the narrowest non-empty bucket and a few dozen others."""
        w = np.diff(self.off.astype(np.int64))
        full = np.flatnonzero(w > 0)
        assert full.size, "apply_removals on a table without nodes"
        b = int(full[np.argmin(w[full])])
        gone = np.unique(np.concatenate([np.arange(self.off[b], self.off[b + 1]),
                                         self.rng.choice(self.n, size=min(60, self.n // 10), replace=False)]))
        ops = np.zeros((gone.shape[0], 3), np.uint32)
        ops[:, 0], ops[:, 1] = KAD_OP_REMOVE, gone
        return self._apply(ops, np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8))

    def _expire(self, kind):
        t = self.table()
        want = R.sweep_ref(t)
        n0 = self.n
        gone = want["expired_nodes"]
        out = {"calls": [("expire", ())], "removed": gone, "buckets": want["changed_buckets"], "n_old": n0, "emptied": 0}
        if gone.shape[0] == 0:  # kadgpu.h: the table is untouched, the remap is the identity
            out["remap"] = np.arange(n0, dtype=np.uint32)
            return out
        w0 = np.diff(self.off.astype(np.int64))
        ids, st, first, off, remap, _ = R.expire_ref(t)
        keep = remap != O.NO_NODE

        def carried(a):
            new = np.zeros((ids.shape[0],) + a.shape[1:], a.dtype)
            new[remap[keep]] = a[keep]
            return new

        if self.times is not None:
            self.times = tuple(carried(a) for a in self.times)
        if self.addrs is not None:
            self.addrs = carried(self.addrs)
        self.ids, self.status, self.first, self.off = ids, st, first, off
        self.sorted, self.dl_valid = False, False
        out["remap"] = remap
        out["emptied"] = int(((w0 > 0) & (np.diff(off.astype(np.int64)) == 0)).sum())
        return out

    def _update_status(self, kind):
        nodes = self.rng.choice(self.n, size=self.n // 3, replace=False)
        st = self.status.copy()
        st[nodes] = mostly_good(self.rng, nodes.shape[0])
        self.status, self.dl_valid = st, False
        return {"calls": [("update_status", (st.copy(),))]}

    def _patch(self, m, values):
        nodes = np.sort(self.rng.choice(self.n, size=min(m, self.n), replace=False)).astype(np.uint32)
        vals = values(nodes.shape[0])
        self.status = self.status.copy()
        self.status[nodes] = vals
        self.dl_valid = False
        return {"calls": [("patch_status", (nodes, vals))]}

    def _patch_small(self, kind):
        # GOOD | EXPIRED is no state of a Node (node.cpp:34-40), and the oracle's list table does not keep it
        return self._patch(7, lambda m: self.rng.choice(np.array([0, 1, 1, 2, 1], np.uint8), size=m))

    def _patch_large(self, kind):
        assert self.n > 2500, "patch_large needs more than 2048 nodes"
        return self._patch(2500, lambda m: mostly_good(self.rng, m))

    def _set_times(self, kind):
        self.times = draw_times(self.rng, self.n, self.now)
        self.status = R.status_at(*self.times, self.now)
        self.dl_valid, self.from_times = self.n > 0, True
        return {"calls": [("set_times", self.times), ("refresh_status", (self.now,))]}

    def _refused(self, call):
        return {"calls": [call], "raises": NO_TIMES}

    def _refresh(self, kind):
        if self.times is None:
            return self._refused(("refresh_status", (self.now + 1,)))
        d = self.pending()
        if kind == "refresh_none":  # on the next deadline (that node is still good) or half way to it
            new = self.now if d.size == 0 else int(d[0]) if self.rng.random() < 0.5 else (self.now + int(d[0])) // 2
        else:
            k = int(self.rng.choice([x for x in PASS[kind]]))
            assert d.size >= k, f"{kind}: {d.size} deadlines ahead, {k} wanted"
            new = int(d[k - 1]) + 1
        passed = int((d < new).sum())
        lo, hi = BANDS[kind]
        assert lo <= passed and (hi is None or passed <= hi), f"{kind}: {passed} deadlines passed"
        unchanged = kind == "refresh_none" and self.dl_valid  # returns at once without touching the GPU
        before = self.status
        self.now = new
        self.status = R.status_at(*self.times, new)
        if unchanged:
            assert np.array_equal(before, self.status)
        self.dl_valid, self.from_times = self.n > 0, True
        return {"calls": [("refresh_status", (new,))], "passed": passed, "unchanged": unchanged}

    def _patch_times(self, kind):
        m = min(8, self.n)
        nodes = np.sort(self.rng.choice(self.n, size=m, replace=False)).astype(np.uint32)
        if self.times is None:
            z = np.zeros(m, np.int64)
            return self._refused(("patch_times", (nodes, z, z, np.zeros(m, np.uint8))))
        time_ns, reply_ns, expired = (a.copy() for a in self.times)
        heard, gone = nodes[:m // 2], nodes[m // 2:]
        time_ns[heard] = self.now - np.arange(heard.shape[0])  # heard again: good at the next refresh
        reply_ns[heard] = time_ns[heard]
        expired[heard] = 0
        expired[gone] = 1                                        # setExpired
        self.times = (time_ns, reply_ns, expired)
        self.now += 1
        self.status = R.status_at(*self.times, self.now)
        self.dl_valid, self.from_times = self.n > 0, True
        return {"calls": [("patch_times", (nodes, time_ns[nodes], reply_ns[nodes], expired[nodes])),
                          ("refresh_status", (self.now,))]}

    def _prepare(self, kind):
        return {"calls": [("prepare", ())]}

    def _set_addrs(self, kind):
        alen = self.addrs.shape[1] if self.addrs is not None else int(self.rng.choice([6, 18]))  # v4 or v6 records
        self.addrs = self.rng.integers(0, 256, size=(self.n, alen), dtype=np.uint8)
        return {"calls": [("set_addrs", (self.addrs.copy(),))]}


def checked_step(m, kind, prev=None):
    """One step with what every script must hold asserted: the refresh bands (in the step), the 85 % floor while the
    statuses come from node times, and that an expire removes a node unless it follows another expire directly (then
    it must remove none)."""
    s = m.step(kind)
    if m.from_times and m.n:
        assert m.good_share() >= FLOOR, f"{m.name} {kind}: good share {m.good_share():.3f}"
    if kind == "expire":
        if prev == "expire":
            assert s["removed"].shape[0] == 0
        else:
            assert s["removed"].shape[0] >= 1, f"{m.name}: expire with no expired node"
    return s


def run_script(t, kinds, seed=0):
    """The script on the model alone: (model at the end, the steps, the good share after each step or None where the
    statuses do not come from node times)."""
    m = Model(t, seed)
    steps, shares = [], []
    for j, kind in enumerate(kinds):
        try:
            steps.append(checked_step(m, kind, kinds[j - 1] if j else None))
        except AssertionError as e:
            raise AssertionError(f"{t['name']} step {j}: {e}") from None
        shares.append(m.good_share() if m.from_times else None)
    return m, steps, shares


def pairs_of(kinds):
    return set(zip(kinds[:-1], kinds[1:]))


def random_walk(t, seed, steps=30):
    """A seeded walk over the kinds the table's size allows, drawn against the model itself: a kind whose step would
    break what checked_step asserts is drawn again, a refresh or patch_times on a table without node times is kept
    only directly after the apply that dropped them, and one apply_split and one apply_removals are placed at drawn
    positions so that every walk splits a bucket and empties one."""
    rng = np.random.default_rng(seed)
    kinds = [k for k in KINDS if k not in BIG_ONLY or t["ids"].shape[0] >= 20_000]
    forced = dict(zip(rng.choice(np.arange(1, steps), size=2, replace=False).tolist(), ("apply_split", "apply_removals")))
    m = Model(t, seed)
    out = []
    while len(out) < steps:
        prev = out[-1] if out else None
        for _ in range(64):
            kind = forced.get(len(out)) or kinds[int(rng.integers(0, len(kinds)))]
            trial = m.copy()
            try:
                s = checked_step(trial, kind, prev)
            except AssertionError:
                continue
            if s["raises"] and prev not in ("apply_mix", "apply_split", "apply_removals") and kind not in forced.values():
                continue
            m = trial
            out.append(kind)
            break
        else:
            raise AssertionError(f"{t['name']} walk {seed}: no kind fits at step {len(out)}")
    return tuple(out)
