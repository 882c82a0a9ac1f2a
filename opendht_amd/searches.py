"""Device set of one family's live searches and the batch form of Dht::trySearchInsert.

Dht::trySearchInsert(node) (dht.cpp:816-849) takes lower_bound(node->id) in the family's search map and calls
Search::insertNode forwards and backwards until the first search that refuses. kad_sr_try_insert_batch gives, for a
whole tick of candidates and one snapshot of the searches, which searches would take each candidate and why each
walk stopped; try_search_insert turns those verdicts into the exact sequential result while the host touches only
the searches that accept. try_search_insert_device goes one step further: the accepted inserts
run on the device as well (kad_sr_insert), in rounds planned by plan_insert_round, and no list is uploaded.
try_search_insert_tick is the same scheme with the rounds run by the engine in one call per segment of
the tick (kad_sr_try_insert_tick): the candidates are uploaded once and nothing of the size of the set is read back.
mark_search_nodes carries the node status changes of a tick (timeouts, replies, candidate bits) to
every list that holds the node with one kad_sr_mark_nodes, without the host looking for the holders.
step_searches is Dht::searchStep's decision on every stepped search with one kad_sr_step: which
entries get a get request, which searches are synced and which expire, applied to the device set in place.
step_searches_full is the same with the listen requests and the announce probes of a synced search
(kad_sr_step_full), for the searches that carry a listen() or a put().
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (KAD_NO_NODE, KAD_SEARCH_NODES, KAD_SN_BAD, KAD_SN_REMOVABLE, KAD_SR_INSERT_OVERFLOW,
                   KAD_SR_REFILL_OVERFLOW, KAD_SR_TICK_APPLIED, KAD_SR_TICK_LEFT,
                   KAD_SR_STOP_END, KAD_SR_STOP_FAR, KAD_SR_STOP_FAR_EXPIRED, KAD_SR_STOP_KNOWN, KAD_STEP_APPLY,
                   KAD_STEP_DONE, KAD_STEP_EXHAUSTED, KAD_STEP_EXPIRE, KAD_STEP_NO_EXPIRE, KAD_STEP_PROBE_BLOCKS,
                   KAD_STEP_SHORT, KAD_STEP_SKIPPED, KAD_STEP_SYNCED, STEP_FULL_OUT_DTYPE, STEP_OUT_DTYPE, check, lib, ptr,
                   sr_step_full_stats, sr_step_stats, sr_tick_stats)
from .table import _as_ids, _stream_of

STOP_NAMES = {KAD_SR_STOP_END: "end", KAD_SR_STOP_KNOWN: "known", KAD_SR_STOP_FAR: "far",
              KAD_SR_STOP_FAR_EXPIRED: "far_expired"}


def _lists(m, flags, off, node_ids, node_flags):
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    off = np.ascontiguousarray(off, dtype=np.uint32).reshape(-1)
    node_ids = _as_ids(node_ids)
    node_flags = np.ascontiguousarray(node_flags, dtype=np.uint8).reshape(-1)
    if flags.shape[0] != m or off.shape[0] != m + 1:
        raise ValueError("flags must have one byte and off one offset (plus one) per search")
    if node_ids.shape[0] != node_flags.shape[0] or node_ids.shape[0] < int(off[-1]):
        raise ValueError("node_ids / node_flags shorter than off[-1]")
    return flags, off, node_ids, node_flags


class DeviceSearches:
    """One family's live searches on the device (kad_searches_create).

    ids         (S, 20) uint8, strictly ascending
    flags       (S,) uint8, KAD_SR_EXPIRED
    off         (S + 1,) uint32, CSR offsets of the node lists
    node_ids    (off[-1], 20) uint8, each list strictly ascending in XOR distance to its search's ID
    node_flags  (off[-1],) uint8, KAD_SN_BAD
    cap         slab entries per search (>= KAD_SEARCH_NODES); a longer list raises KAD_ERR_UNSUPPORTED
    """

    def __init__(self, ids, flags, off, node_ids, node_flags, cap: int = 32, device: int = 0):
        ids = _as_ids(ids)
        S = ids.shape[0]
        flags, off, node_ids, node_flags = _lists(S, flags, off, node_ids, node_flags)
        self._h = C.c_void_p()
        self.device, self.S, self.cap, self._ids = device, S, cap, ids
        check(lib().kad_searches_create(C.byref(self._h), device, S, cap, ptr(ids), ptr(flags), ptr(off),
                                        ptr(node_ids), ptr(node_flags)), "kad_searches_create")

    def recreate(self, flags, off, node_ids, node_flags, cap: int) -> None:
        """A new device set of the same search IDs with slabs of `cap` entries (a list outgrew the old ones:
        KAD_ERR_UNSUPPORTED from patch); the old one is freed once the new one stands."""
        flags, off, node_ids, node_flags = _lists(self.S, flags, off, node_ids, node_flags)
        h = C.c_void_p()
        check(lib().kad_searches_create(C.byref(h), self.device, self.S, cap, ptr(self._ids), ptr(flags), ptr(off),
                                        ptr(node_ids), ptr(node_flags)), "kad_searches_create")
        self.close()
        self._h, self.cap = h, cap

    def close(self) -> None:
        if self._h:
            lib().kad_searches_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        b = C.c_uint64()
        check(lib().kad_searches_info(self._h, None, None, C.byref(b)), "kad_searches_info")
        return b.value

    def patch(self, which, flags, off, node_ids, node_flags) -> None:
        """Replace the flags and lists of the searches `which` (strictly ascending indices); lists in CSR form as
        for the constructor (kad_searches_patch). Synchronous."""
        which = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        flags, off, node_ids, node_flags = _lists(which.shape[0], flags, off, node_ids, node_flags)
        check(lib().kad_searches_patch(self._h, which.shape[0], ptr(which), ptr(flags), ptr(off), ptr(node_ids),
                                       ptr(node_flags)), "kad_searches_patch")

    def apply(self, erase=(), ins_ids=(), ins_flags=None, cap=None):
        """Erase the searches `erase` (strictly ascending indices), insert empty searches with the IDs ins_ids
        ((n, 20) uint8, any order; ins_flags (n,) uint8 KAD_SR_EXPIRED or None) and grow the slabs to `cap` entries
        (None or 0 keeps them), on the device (kad_searches_apply): (remap (S,) uint32 with the new index of every old
        search, KAD_NO_NODE if erased; new_index (n,) uint32 of the inserted ones). Synchronous."""
        erase = np.ascontiguousarray(erase, dtype=np.uint32).reshape(-1)
        ins = _as_ids(ins_ids) if len(ins_ids) else np.zeros((0, 20), np.uint8)
        n_ins = ins.shape[0]
        if ins_flags is not None:
            ins_flags = np.ascontiguousarray(ins_flags, dtype=np.uint8).reshape(-1)
            if ins_flags.shape[0] != n_ins:
                raise ValueError("ins_flags must have one byte per inserted search")
        remap, new_index = np.zeros(self.S, np.uint32), np.zeros(n_ins, np.uint32)
        check(lib().kad_searches_apply(self._h, ptr(erase), erase.shape[0], ptr(ins), ptr(ins_flags), n_ins,
                                       cap or 0, ptr(remap), ptr(new_index)), "kad_searches_apply")
        kept = remap != KAD_NO_NODE
        ids = np.zeros((int(kept.sum()) + n_ins, 20), np.uint8)
        ids[remap[kept]] = self._ids[kept]
        ids[new_index] = ins
        self.S, self._ids = ids.shape[0], ids
        if cap:  # None and 0 keep the cap
            self.cap = cap
        return remap, new_index

    def grow(self, cap: int) -> None:
        """Slabs of `cap` entries (>= the current cap) for the same searches: apply with the cap alone."""
        self.apply(cap=cap)

    def export(self, nodes: bool = True) -> dict:
        """The device state as host arrays (kad_searches_export): ids, flags, n, full, t per search and, with
        nodes, the slabs node_ids (S, cap, 20) and node_flags (S, cap)."""
        S, cap = self.S, self.cap
        out = {"ids": np.zeros((S, 20), np.uint8), "flags": np.zeros(S, np.uint8), "n": np.zeros(S, np.uint32),
               "full": np.zeros(S, np.uint8), "t": np.zeros(S, np.uint32)}
        if nodes:
            out["node_ids"] = np.zeros((S, cap, 20), np.uint8)
            out["node_flags"] = np.zeros((S, cap), np.uint8)
        check(lib().kad_searches_export(self._h, ptr(out["ids"]), ptr(out["flags"]), ptr(out["n"]),
                                        ptr(out.get("node_ids")), ptr(out.get("node_flags")), ptr(out["full"]),
                                        ptr(out["t"])), "kad_searches_export")
        return out

    def try_insert(self, ids, want_lb: bool = True, out=None, stream=None):
        """trySearchInsert verdicts (kad_sr_try_insert_batch) over a (q, 20) uint8 device tensor of candidate IDs:
        (lb (q,) int32 or None, fwd (q,) int32, back (q,) int32, stop (q,) uint8 = fstop | bstop << 4). out: the
        same tuple of tensors to write into."""
        import torch

        q = ids.shape[0]
        lb, fwd, back, stop = out if out is not None else (None, None, None, None)
        if lb is None and want_lb:
            lb = torch.empty((q,), dtype=torch.int32, device=ids.device)
        if fwd is None:
            fwd = torch.empty((q,), dtype=torch.int32, device=ids.device)
        if back is None:
            back = torch.empty((q,), dtype=torch.int32, device=ids.device)
        if stop is None:
            stop = torch.empty((q,), dtype=torch.uint8, device=ids.device)
        check(lib().kad_sr_try_insert_batch(self._h, ptr(ids), q, ptr(lb), ptr(fwd), ptr(back), ptr(stop),
                                            _stream_of(self, stream)), "kad_sr_try_insert_batch")
        return lb, fwd, back, stop

    def try_insert_host(self, ids):
        """try_insert over host IDs, synchronous (kad_sr_try_insert_batch_host): (lb, fwd, back uint32, stop
        uint8) host arrays."""
        t = _as_ids(ids)
        q = t.shape[0]
        lb, fwd, back = (np.zeros((q,), dtype=np.uint32) for _ in range(3))
        stop = np.zeros((q,), dtype=np.uint8)
        check(lib().kad_sr_try_insert_batch_host(self._h, ptr(t), q, ptr(lb), ptr(fwd), ptr(back), ptr(stop)),
              "kad_sr_try_insert_batch_host")
        return lb, fwd, back, stop

    def refill(self, nc_table, which):
        """Dht::refill of the searches `which` (strictly ascending indices) from the NodeCache table nc_table, on the
        device (kad_sr_refill): (rows (m, 14) uint32 padded with KAD_NO_NODE, cnt (m,) uint8, inserted (m,) uint16
        with bit j = insertNode(row[j]) returned true, status (m,) uint8 KAD_SR_REFILL_*). Synchronous."""
        which = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        m = which.shape[0]
        rows = np.zeros((m, KAD_SEARCH_NODES), np.uint32)
        cnt, ins, status = np.zeros(m, np.uint8), np.zeros(m, np.uint16), np.zeros(m, np.uint8)
        check(lib().kad_sr_refill(self._h, nc_table.handle, m, ptr(which), ptr(rows), ptr(cnt), ptr(ins), ptr(status)),
              "kad_sr_refill")
        return rows, cnt, ins, status

    def insert(self, which, off, cand_ids, cand_flags=None):
        """Search::insertNode of the candidates cand_ids[off[i]:off[i+1]] ((T, 20) uint8, in list order; cand_flags
        (T,) uint8 KAD_SN_BAD = node->isExpired(), None for all zero) into search which[i] (strictly ascending
        indices), on the device (kad_sr_insert): (inserted (T,) uint8 with 1 where insertNode returned true, status
        (m,) uint8 KAD_SR_INSERT_*). Synchronous."""
        which = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint32).reshape(-1)
        m = which.shape[0]
        if off.shape[0] != m + 1:
            raise ValueError("off must have one offset (plus one) per listed search")
        T = int(off[-1])
        cand = _as_ids(cand_ids) if T else np.zeros((0, 20), np.uint8)
        if cand_flags is not None:
            cand_flags = np.ascontiguousarray(cand_flags, dtype=np.uint8).reshape(-1)
        if cand.shape[0] < T or (cand_flags is not None and cand_flags.shape[0] < T):
            raise ValueError("cand_ids / cand_flags shorter than off[-1]")
        ins, status = np.zeros(T, np.uint8), np.zeros(m, np.uint8)
        check(lib().kad_sr_insert(self._h, m, ptr(which), ptr(off), ptr(cand), ptr(cand_flags), ptr(ins), ptr(status)),
              "kad_sr_insert")
        return ins, status

    def try_insert_tick(self, cand_ids, cand_flags=None, max_rounds: int = 0) -> dict:
        """Dht::trySearchInsert of the candidates cand_ids ((q, 20) uint8, in arrival order; cand_flags (q,) uint8
        KAD_SN_BAD = node->isExpired(), None for all zero) applied to the set in one call (kad_sr_try_insert_tick): the
        rounds of verdicts, plan and inserts run in the engine, for up to max_rounds rounds (0: no limit). Returns kind
        (q,) uint8 KAD_SR_TICK_*, round (q,) uint32 and the deciding round's verdict lb, fwd, back (q,) uint32, stop and
        trim (q,) uint8 for the candidates that are not LEFT, overflow (the searches left untouched because their slab
        is too small, ascending) and stats (kad_sr_tick_stats as a dict). Synchronous."""
        cand = _as_ids(cand_ids) if len(cand_ids) else np.zeros((0, 20), np.uint8)
        q = cand.shape[0]
        if cand_flags is not None:
            cand_flags = np.ascontiguousarray(cand_flags, dtype=np.uint8).reshape(-1)
            if cand_flags.shape[0] != q:
                raise ValueError("cand_flags must have one byte per candidate")
        out = {"kind": np.zeros(q, np.uint8), "round": np.zeros(q, np.uint32), "lb": np.zeros(q, np.uint32),
               "fwd": np.zeros(q, np.uint32), "back": np.zeros(q, np.uint32), "stop": np.zeros(q, np.uint8),
               "trim": np.zeros(q, np.uint8)}
        over, n_over, st = np.zeros(max(self.S, 1), np.uint32), C.c_uint32(), sr_tick_stats()
        check(lib().kad_sr_try_insert_tick(self._h, ptr(cand), ptr(cand_flags), q, max_rounds, ptr(out["kind"]),
                                           ptr(out["round"]), ptr(out["lb"]), ptr(out["fwd"]), ptr(out["back"]),
                                           ptr(out["stop"]), ptr(out["trim"]), ptr(over), C.byref(n_over),
                                           C.byref(st)), "kad_sr_try_insert_tick")
        out["overflow"] = over[:n_over.value].copy()
        out["stats"] = {n: getattr(st, n) for n, _ in sr_tick_stats._fields_}
        return out

    def insert_kernel_ms(self) -> float:
        """The device time of the last insert's insert kernel (kad_sr_insert_kernel_ms)."""
        ms = C.c_float()
        check(lib().kad_sr_insert_kernel_ms(self._h, C.byref(ms)), "kad_sr_insert_kernel_ms")
        return ms.value

    def mark_nodes(self, node_ids, clear_bits=None, set_bits=None, pairs=None) -> dict:
        """Node status changes over the set (kad_sr_mark_nodes): every list entry whose ID is node_ids[j] ((q, 20) uint8,
        distinct, any order) gets the flag byte (f & ~clear_bits[j]) | set_bits[j] ((q,) uint8 of KAD_SN_BAD |
        KAD_SN_REMOVABLE, None for all zero); then every pair of pairs = (which (p,), ids (p, 20), flags (p,)) whose
        search holds the ID gets exactly its flag byte. Returns hits (q,) uint32 (searches that hold node j), pair_found
        (p,) uint8, changed (ascending indices of the searches with a byte that differs from before) and counts
        (len(changed), 4) uint8: n, bad, leading bad, record bits. Synchronous."""
        ids = _as_ids(node_ids) if len(node_ids) else np.zeros((0, 20), np.uint8)
        q = ids.shape[0]
        if clear_bits is not None:
            clear_bits = np.ascontiguousarray(clear_bits, dtype=np.uint8).reshape(-1)
        if set_bits is not None:
            set_bits = np.ascontiguousarray(set_bits, dtype=np.uint8).reshape(-1)
        if any(b is not None and b.shape[0] != q for b in (clear_bits, set_bits)):
            raise ValueError("clear_bits / set_bits must have one byte per node")
        pw, pid, pfl, p = None, None, None, 0
        if pairs is not None and len(pairs[0]):
            pw = np.ascontiguousarray(pairs[0], dtype=np.uint32).reshape(-1)
            pid = _as_ids(pairs[1])
            pfl = np.ascontiguousarray(pairs[2], dtype=np.uint8).reshape(-1)
            p = pw.shape[0]
            if pid.shape[0] != p or pfl.shape[0] != p:
                raise ValueError("pairs must be (which, ids, flags) of one length")
        hits, found = np.zeros(q, np.uint32), np.zeros(p, np.uint8)
        changed, counts, n = np.zeros(self.S, np.uint32), np.zeros((self.S, 4), np.uint8), C.c_uint32()
        check(lib().kad_sr_mark_nodes(self._h, q, ptr(ids), ptr(clear_bits), ptr(set_bits), p, ptr(pw), ptr(pid),
                                      ptr(pfl), ptr(hits), ptr(found), ptr(changed), ptr(counts), C.byref(n)),
              "kad_sr_mark_nodes")
        return {"hits": hits, "pair_found": found, "changed": changed[:n.value].copy(),
                "counts": counts[:n.value].copy()}

    def mark_kernel_ms(self):
        """The device times (scan kernel, fix kernel) of the last mark_nodes (kad_sr_mark_kernel_ms)."""
        a, b = C.c_float(), C.c_float()
        check(lib().kad_sr_mark_kernel_ms(self._h, C.byref(a), C.byref(b)), "kad_sr_mark_kernel_ms")
        return a.value, b.value

    def mark_entries(self, which, ids, clear_bits=None, set_bits=None):
        """Step bits of single entries (kad_sr_mark_entries): for every pair (which[k], ids[k]) whose search holds the ID,
        the flag byte becomes (f & ~clear_bits[k]) | set_bits[k] ((p,) uint8 over KAD_SN_CANDIDATE | KAD_SN_PENDING |
        KAD_SN_SYNCED | KAD_SN_NOGET, None for all zero). Returns found (p,) uint8. Synchronous."""
        return self._mark_bits("kad_sr_mark_entries", which, ids, clear_bits, set_bits)

    def step(self, which=None, modes=None) -> dict:
        """Dht::searchStep's decision on the searches `which` (strictly ascending indices; None: every search) under
        modes ((m,) uint8 of KAD_STEP_APPLY | KAD_STEP_NO_SEND | KAD_STEP_DONE_IF_SYNCED | KAD_STEP_NO_EXPIRE, or one
        int for all, None for 0), on the device (kad_sr_step). Returns picks (m,) uint64 (bit e: entry e gets a
        request), n, bad, lead_bad, solicited (m,) uint8, bits (m,) uint32 of KAD_STEP_SKIPPED .. KAD_STEP_EXPIRE, and
        stats (kad_sr_step_stats as a dict). With KAD_STEP_APPLY the sends and expiries are written to the set.
        Synchronous."""
        return self._step("kad_sr_step", STEP_OUT_DTYPE, sr_step_stats, which, modes)

    def _which_modes(self, which, modes):
        """step's arguments as the call takes them: which (m,) uint32 or None, m, modes (m,) uint8 or None."""
        if which is not None:
            which = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        m = self.S if which is None else which.shape[0]
        if modes is not None:
            modes = (np.full(m, modes, np.uint8) if np.isscalar(modes)
                     else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1))
            if modes.shape[0] != m:
                raise ValueError("modes must have one byte per stepped search")
        return which, m, modes

    def _step(self, call, dtype, stats_cls, which, modes) -> dict:
        which, m, modes = self._which_modes(which, modes)
        out, st = np.zeros(m, dtype), stats_cls()
        check(getattr(lib(), call)(self._h, m, ptr(which), ptr(modes), ptr(out), C.byref(st)), call)
        return _step_fields(out, {n: getattr(st, n) for n, _ in stats_cls._fields_})

    def mark_due(self, which, ids, clear_bits=None, set_bits=None):
        """mark_entries for the two due bits (kad_sr_mark_due): clear_bits and set_bits over KAD_SN_LISTEN_DUE |
        KAD_SN_ANNOUNCE_DUE. Returns found (p,) uint8. Synchronous."""
        return self._mark_bits("kad_sr_mark_due", which, ids, clear_bits, set_bits)

    def _mark_bits(self, call, which, ids, clear_bits, set_bits):
        pw = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
        p = pw.shape[0]
        pid = _as_ids(ids) if p else np.zeros((0, 20), np.uint8)
        if clear_bits is not None:
            clear_bits = np.ascontiguousarray(clear_bits, dtype=np.uint8).reshape(-1)
        if set_bits is not None:
            set_bits = np.ascontiguousarray(set_bits, dtype=np.uint8).reshape(-1)
        if pid.shape[0] != p or any(b is not None and b.shape[0] != p for b in (clear_bits, set_bits)):
            raise ValueError("ids, clear_bits and set_bits must have one entry per pair")
        found = np.zeros(p, np.uint8)
        check(getattr(lib(), call)(self._h, p, ptr(pw), ptr(pid), ptr(clear_bits), ptr(set_bits), ptr(found)), call)
        return found

    def step_full(self, which=None, modes=None) -> dict:
        """step with the listen and announce sends (kad_sr_step_full): modes may also carry KAD_STEP_LISTEN,
        KAD_STEP_ANNOUNCE and KAD_STEP_PROBE_BLOCKS. Returns step's arrays plus listen and announce (m,) uint64 (bit e:
        entry e gets the listen requests due on it / the announce probe); stats is kad_sr_step_full_stats as a dict.
        With KAD_STEP_APPLY the three kinds of sends and the expiries are written to the set. Synchronous."""
        return self._step("kad_sr_step_full", STEP_FULL_OUT_DTYPE, sr_step_full_stats, which, modes)

    @property
    def refill_kernel_ms(self) -> float:
        """The device time of the last refill's refill kernel (kad_sr_refill_kernel_ms)."""
        ms = C.c_float()
        check(lib().kad_sr_refill_kernel_ms(self._h, C.byref(ms)), "kad_sr_refill_kernel_ms")
        return ms.value


def apply_search_verdicts(host, S: int, lb, fwd, back, stop, trims):
    """The host half of try_search_insert: the candidates in order against the verdicts (host arrays) of one
    snapshot, with a dirty mark per search. trims[s]: search s held entries past its trim position in the snapshot
    (full and t < n). Returns the counts and the dirty marks."""
    counts = {"skipped": 0, "direct": 0, "fallback": 0, "inserts": 0}
    dirty = np.zeros(S, dtype=bool)
    far = (KAD_SR_STOP_FAR, KAD_SR_STOP_FAR_EXPIRED)
    for j in range(len(stop)):
        l, f, b = int(lb[j]), int(fwd[j]), int(back[j])
        fs, bs = int(stop[j]) & 15, int(stop[j]) >> 4
        pending = bool((fs in far and trims[l + f]) or (bs in far and trims[l - b - 1]))
        if (f + b == 0 and fs in (KAD_SR_STOP_END, KAD_SR_STOP_FAR) and bs in (KAD_SR_STOP_END, KAD_SR_STOP_FAR)
                and not pending):
            counts["skipped"] += 1
            continue
        if S and not pending and not dirty[max(l - b - 1, 0):min(l + f, S - 1) + 1].any():
            for s in list(range(l, l + f)) + list(range(l - 1, l - b - 1, -1)):
                if not host.insert(s, j):
                    raise RuntimeError(f"try_search_insert: search {s} refused candidate {j} against its verdict")
            dirty[l - b:l + f] = True
            counts["direct"] += 1
            counts["inserts"] += f + b
            continue
        counts["fallback"] += 1
        s = l
        while s < S:  # insert forward (dht.cpp:826-836)
            dirty[s] = True
            if not host.insert(s, j):
                break
            counts["inserts"] += 1
            s += 1
        s = l
        while s > 0:  # insert backward (dht.cpp:837-847)
            s -= 1
            dirty[s] = True
            if not host.insert(s, j):
                break
            counts["inserts"] += 1
    return counts, dirty


def try_search_insert(DS: DeviceSearches, host, cand_ids) -> dict:
    """Dht::trySearchInsert for the candidates cand_ids ((q, 20) uint8, in arrival order) over the searches of DS,
    with one verdict launch. `host` holds the real searches: host.insert(s, j) -> bool is Search::insertNode of
    candidate j into search s, host.state(s) -> (flags, node_ids, node_flags) its state afterwards. The searches end
    exactly as after q sequential trySearchInsert calls, and DS is patched to match.

    A candidate that both neighbours refuse as too far (or that has no neighbour on a side) is skipped without a
    host probe: a FAR refusal by a live search survives every later insert of the tick (inserts only move the
    threshold closer, bad nodes do not count towards it, an insert never makes a live search expired). KNOWN does not
    survive (removeExpiredNode can drop the member), nor does FAR_EXPIRED (an accepted good node resets `expired`,
    dht.cpp:1026-1029). A refusing search that holds entries past its trim position is not a no-op either: the
    reference trims it while refusing (dht.cpp:1010-1011), so such a candidate takes the reference walk.
    Otherwise the verdict is applied directly while no search of [lb-back-1, lb+fwd] was touched earlier in the
    tick, and the reference walk runs on the host if one was.

    Returns {"skipped", "direct", "fallback", "inserts"}."""
    import torch

    cand = _as_ids(cand_ids)
    if cand.shape[0] == 0:
        return {"skipped": 0, "direct": 0, "fallback": 0, "inserts": 0}
    dev = torch.device("cuda", DS.device)
    lb, fwd, back, stop = DS.try_insert(torch.from_numpy(cand).to(dev))
    torch.cuda.synchronize(dev)
    st = DS.export(nodes=False)
    trims = (st["full"] != 0) & (st["t"] < st["n"])  # a refusal by such a search still trims it
    counts, dirty = apply_search_verdicts(host, DS.S, lb.cpu().numpy().view(np.uint32),
                                          fwd.cpu().numpy().view(np.uint32), back.cpu().numpy().view(np.uint32),
                                          stop.cpu().numpy(), trims)
    def states(which):
        flags, off, nid, nfl = [], [0], [np.zeros((0, 20), np.uint8)], [np.zeros(0, np.uint8)]
        for s in which:
            fl, ids_s, nf_s = host.state(int(s))
            flags.append(fl)
            if len(ids_s):
                nid.append(_as_ids(ids_s))
                nfl.append(np.asarray(nf_s, dtype=np.uint8).reshape(-1))
            off.append(off[-1] + len(ids_s))
        return np.array(flags, np.uint8), np.array(off, np.uint32), np.concatenate(nid), np.concatenate(nfl)

    which = np.flatnonzero(dirty)
    if which.size:
        flags, off, nid, nfl = states(which)
        longest = int(np.diff(off).max())
        if longest <= DS.cap:
            DS.patch(which, flags, off, nid, nfl)
        else:  # a list outgrew the slabs (bad nodes do not count towards SEARCH_NODES): a new set
            DS.recreate(*states(range(DS.S)), cap=max(longest, 2 * DS.cap))
    return counts


def plan_insert_round(S: int, lb, fwd, back, stop, trims):
    """One scan over the remaining candidates of a tick, in order, against the verdicts (host arrays) of one snapshot
    (DESIGN.md §7.16). trims[s]: search s held entries past its trim position in the snapshot (full and t < n).
    Returns (skipped, ready, deferred): skipped and deferred are lists of candidate positions, ready a list of
    (position, [(search, expected insertNode result), ...]).

    T_j, the searches candidate j probes, is [lb-back-1, lb+fwd] without the ends whose stop is END.
      skipped   fwd + back == 0, both stops END or FAR, neither stopper trims: final in any order, marks nothing.
      ready     T_j meets no T of an earlier candidate of the scan that was not skipped, and does not lie in the
                open side of an earlier deferred one: a deferred candidate whose forward stop is KNOWN or FAR_EXPIRED
                (stops that do not survive earlier inserts) may walk on, so it blocks every search from its lowest
                probed index upwards; likewise backwards from its highest probed index downwards.
      deferred  everything else; it waits for the next round.
    The pairs of a ready candidate are its accepting searches (expected 1) and every FAR / FAR_EXPIRED stopper that
    trims (expected 0: the refusal still cuts the list). Ready candidates of one round never share a search."""
    far, open_stops = (KAD_SR_STOP_FAR, KAD_SR_STOP_FAR_EXPIRED), (KAD_SR_STOP_KNOWN, KAD_SR_STOP_FAR_EXPIRED)
    marked = np.zeros(S + 1, dtype=bool)
    block_up, block_down = S, -1  # searches >= block_up and <= block_down are blocked
    skipped, ready, deferred = [], [], []
    for j in range(len(stop)):
        l, f, b = int(lb[j]), int(fwd[j]), int(back[j])
        fs, bs = int(stop[j]) & 15, int(stop[j]) >> 4
        ftrim = fs in far and bool(trims[l + f])
        btrim = bs in far and bool(trims[l - b - 1])
        if (f + b == 0 and fs in (KAD_SR_STOP_END, KAD_SR_STOP_FAR) and bs in (KAD_SR_STOP_END, KAD_SR_STOP_FAR)
                and not ftrim and not btrim):
            skipped.append(j)
            continue
        lo = l - b - (0 if bs == KAD_SR_STOP_END else 1)
        hi = l + f - (1 if fs == KAD_SR_STOP_END else 0)
        if lo <= hi and not marked[lo:hi + 1].any() and hi < block_up and lo > block_down:
            pairs = [(s, 1) for s in range(l, l + f)] + [(s, 1) for s in range(l - 1, l - b - 1, -1)]
            if ftrim:
                pairs.append((l + f, 0))
            if btrim:
                pairs.append((l - b - 1, 0))
            ready.append((j, pairs))
        else:
            deferred.append(j)
            if lo <= hi:
                if fs in open_stops:
                    block_up = min(block_up, lo)
                if bs in open_stops:
                    block_down = max(block_down, hi)
        if lo <= hi:
            marked[lo:hi + 1] = True
    return skipped, ready, deferred


def _host_states(host, idx, now):
    flags, off, nid, nfl = [], [0], [np.zeros((0, 20), np.uint8)], [np.zeros(0, np.uint8)]
    for s in idx:
        fl, ids_s, nf_s = host.state(int(s), now)
        flags.append(fl)
        if len(ids_s):
            nid.append(_as_ids(ids_s))
            nfl.append(np.asarray(nf_s, dtype=np.uint8).reshape(-1))
        off.append(off[-1] + len(ids_s))
    return np.array(flags, np.uint8), np.array(off, np.uint32), np.concatenate(nid), np.concatenate(nfl)


def _patch_from_host(DS, host, idx, now) -> None:
    """The searches idx (any order, repeats allowed) from the host's lists; the slabs grow when a list no longer fits."""
    idx = sorted(set(int(s) for s in idx))
    if not idx:
        return
    flags, off, nid, nfl = _host_states(host, idx, now)
    longest = int(np.diff(off).max())
    if longest > DS.cap:
        DS.grow(max(longest, 2 * DS.cap))
    DS.patch(np.array(idx, np.uint32), flags, off, nid, nfl)


def _host_walk(host, S: int, l: int, j: int, touched: list) -> bool:
    """Dht::trySearchInsert's two walks of candidate j from its lower bound l on the host; the probed searches are
    appended to touched. True if any search accepted."""
    inserted = False
    s = l
    while s < S:  # insert forward (dht.cpp:826-836)
        touched.append(s)
        if not host.insert(s, j):
            break
        inserted = True
        s += 1
    s = l
    while s > 0:  # insert backward (dht.cpp:837-847)
        s -= 1
        touched.append(s)
        if not host.insert(s, j):
            break
        inserted = True
    return inserted


def try_search_insert_device(DS, host, cand_ids, now, max_rounds=8) -> dict:
    """Dht::trySearchInsert for the candidates cand_ids ((q, 20) uint8, in arrival order) over the searches of DS,
    with the accepted inserts applied on the device: rounds of one verdict launch for the remaining
    candidates, plan_insert_round, one DS.insert of the ready pairs and the host's replay of the ready candidates
    (host.insert(s, j) forwards, then backwards, until the first refusal; any result that differs from the device's
    byte or from the verdict raises). Deferred candidates wait for the next round; after max_rounds rounds (None: no
    limit) the rest takes the reference walk on the host, in order, followed by one patch. Searches the device
    reports as KAD_SR_INSERT_OVERFLOW are patched from the host's lists, the slabs grown when a list no longer fits.

    `host` holds the real searches: insert(s, j) -> bool, state(s, now) -> (flags, node_ids, node_flags) with
    KAD_SN_REMOVABLE evaluated at `now`, bad(j) -> node->isExpired() of candidate j, old(j) -> its node is removable at
    `now` (expired and time + NODE_EXPIRE_TIME < now), holders(j) -> the searches that hold its node. The device set's
    KAD_SN_REMOVABLE bits must be those of `now` (as for refill_searches). A candidate that is old is a barrier:
    old(j) is asked when the scan reaches j, after every earlier old candidate has been applied; everything before it
    is finished by rounds, then it takes the host walk, and the searches it probed are patched together with, if any
    search accepted it, every search of holders(j) (node.time = now clears its REMOVABLE bit wherever it is a member).

    Returns {"skipped", "device", "host", "rounds", "pairs", "overflowed"}."""
    cand = _as_ids(cand_ids)
    q = cand.shape[0]
    counts = {"skipped": 0, "device": 0, "host": 0, "rounds": 0, "pairs": 0, "overflowed": 0}

    def rounds(rem):
        """Rounds over the candidates rem (ascending positions) until none is left or the budget is spent: what is left."""
        # kad_sr_insert holds a list in one wave: slabs grown past 64 entries leave the rest to the host path
        while rem and DS.cap <= 64 and (max_rounds is None or counts["rounds"] < max_rounds):
            counts["rounds"] += 1
            ids = cand[rem]
            lb, fwd, back, stop = DS.try_insert_host(ids)
            st = DS.export(nodes=False)
            trims = (st["full"] != 0) & (st["t"] < st["n"])
            skipped, ready, deferred = plan_insert_round(DS.S, lb, fwd, back, stop, trims)
            counts["skipped"] += len(skipped)
            counts["device"] += len(ready)
            pairs = sorted((s, rem[k], want) for k, pr in ready for s, want in pr)  # one candidate per search
            got, over = {}, set()
            if pairs:
                which = np.array([p[0] for p in pairs], np.uint32)
                js = [p[1] for p in pairs]
                ins, status = DS.insert(which, np.arange(len(pairs) + 1, dtype=np.uint32), cand[js],
                                        np.array([KAD_SN_BAD if host.bad(j) else 0 for j in js], np.uint8))
                counts["pairs"] += len(pairs)
                over = set(int(s) for s in which[status == KAD_SR_INSERT_OVERFLOW])
                got = {(p[0], p[1]): (int(ins[k]), p[2]) for k, p in enumerate(pairs)}
            for k, _ in ready:  # the replay: the reference's own walk, checked against the device and the verdict
                j, l, f, b = rem[k], int(lb[k]), int(fwd[k]), int(back[k])
                for rng, end in ((range(l, DS.S), l + f), (range(l - 1, -1, -1), l - b - 1)):
                    for s in rng:
                        r = bool(host.insert(s, j))
                        if r != (s != end):
                            raise RuntimeError(f"try_search_insert_device: search {s} answered {r} to candidate {j} "
                                               "against its verdict")
                        if (s, j) in got and s not in over and got[(s, j)][0] != int(r):
                            raise RuntimeError(f"try_search_insert_device: search {s}, candidate {j}: the host "
                                               f"answered {r}, the device {got[(s, j)][0]}")
                        if not r:
                            break
            if over:
                counts["overflowed"] += len(over)
                _patch_from_host(DS, host, over, now)
            rem = [rem[k] for k in deferred]
        return rem

    dirty, pos = [], 0
    left = []  # what the rounds left when the budget ran out, and everything after it: the host path, in order
    while pos < q:
        end = pos
        while end < q and not (host.bad(end) and host.old(end)):
            end += 1
        segment = list(range(pos, end))
        left = left + segment if left else rounds(segment)
        if end < q:  # the barrier
            if left:  # the budget is spent: the old candidate waits its turn on the host path
                left.append(end)
            else:
                counts["host"] += 1
                touched = []
                lb = DS.try_insert_host(cand[end:end + 1])[0]
                if _host_walk(host, DS.S, int(lb[0]), end, touched):
                    touched += [int(s) for s in host.holders(end)]
                _patch_from_host(DS, host, touched, now)
        pos = end + 1
    if left:
        lbs = DS.try_insert_host(cand[left])[0]
        for k, j in enumerate(left):
            counts["host"] += 1
            was_old = bool(host.bad(j) and host.old(j))
            holders = [int(s) for s in host.holders(j)] if was_old else []
            if _host_walk(host, DS.S, int(lbs[k]), j, dirty):
                dirty += holders
        _patch_from_host(DS, host, dirty, now)
    return counts


def plan_round(S: int, lb, fwd, back, stop, trim):
    """plan_insert_round by the engine's planner (kad_sr_plan_round, no device): trim[k] bit 0 = the forward stopper is
    FAR / FAR_EXPIRED and trims, bit 1 = the backward one. Returns (kind (r,) uint8 KAD_SR_PLAN_*, pair_which, pair_cand
    (position in the round) uint32 and pair_want uint8, ascending by search)."""
    lb, fwd, back = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (lb, fwd, back))
    stop, trim = (np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in (stop, trim))
    r = stop.shape[0]
    if any(a.shape[0] != r for a in (lb, fwd, back, trim)):
        raise ValueError("one verdict and one trim byte per candidate")
    kind = np.zeros(r, np.uint8)
    pw, pc, want, n = np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint8), C.c_uint32()
    rc = lib().kad_sr_plan_round(S, r, ptr(lb), ptr(fwd), ptr(back), ptr(stop), ptr(trim), ptr(kind), ptr(pw), ptr(pc),
                                 ptr(want), C.byref(n))
    if rc:
        raise ValueError(f"kad_sr_plan_round: {rc}: verdicts outside the {S} searches")
    return kind, pw[:n.value].copy(), pc[:n.value].copy(), want[:n.value].copy()


def try_search_insert_tick(DS, host, cand_ids, now, max_rounds=8) -> dict:
    """try_search_insert_device with the rounds run by the engine: one DS.try_insert_tick per segment
    of the tick, a segment ending before every old candidate (host.bad(j) and host.old(j), asked when the scan reaches
    j), which is handled as try_search_insert_device handles it. The host replays the APPLIED candidates in (round,
    position) order, every answer checked against the verdict; searches the call lists as overflowed are patched from
    the host's lists, the slabs grown when a list no longer fits, and the call is repeated for what it left while the
    round budget lasts (max_rounds over the whole tick, None: no limit). What is LEFT then takes the reference walk on
    the host, in order, followed by one patch. Same `host`, same preconditions and the same counts as
    try_search_insert_device: {"skipped", "device", "host", "rounds", "pairs", "overflowed"}."""
    cand = _as_ids(cand_ids)
    q = cand.shape[0]
    counts = {"skipped": 0, "device": 0, "host": 0, "rounds": 0, "pairs": 0, "overflowed": 0}

    def replay(rem, r):
        applied = np.flatnonzero(r["kind"] == KAD_SR_TICK_APPLIED)
        for k in applied[np.argsort(r["round"][applied], kind="stable")]:
            j, l, f, b = rem[k], int(r["lb"][k]), int(r["fwd"][k]), int(r["back"][k])
            for rng, end in ((range(l, DS.S), l + f), (range(l - 1, -1, -1), l - b - 1)):
                for s in rng:
                    got = bool(host.insert(s, j))
                    if got != (s != end):
                        raise RuntimeError(f"try_search_insert_tick: search {s} answered {got} to candidate {j} "
                                           "against its verdict")
                    if not got:
                        break

    def rounds(rem):
        """Engine calls over the candidates rem (ascending positions) until none is left or the budget is spent."""
        # the insert kernel holds a list in one wave: slabs grown past 64 entries leave the rest to the host path
        while rem and DS.cap <= 64 and (max_rounds is None or counts["rounds"] < max_rounds):
            flags = np.array([KAD_SN_BAD if host.bad(j) else 0 for j in rem], np.uint8)
            r = DS.try_insert_tick(cand[rem], flags, 0 if max_rounds is None else max_rounds - counts["rounds"])
            st = r["stats"]
            for mine, theirs in (("skipped", "skipped"), ("device", "applied"), ("rounds", "rounds"), ("pairs", "pairs"),
                                 ("overflowed", "overflowed")):
                counts[mine] += st[theirs]
            replay(rem, r)
            if len(r["overflow"]):
                _patch_from_host(DS, host, r["overflow"], now)
            rem = [rem[k] for k in np.flatnonzero(r["kind"] == KAD_SR_TICK_LEFT)]
            if not len(r["overflow"]):
                break
        return rem

    dirty, pos = [], 0
    left = []  # what the calls left when the budget ran out, and everything after it: the host path, in order
    while pos < q:
        end = pos
        while end < q and not (host.bad(end) and host.old(end)):
            end += 1
        segment = list(range(pos, end))
        left = left + segment if left else rounds(segment)
        if end < q:  # the barrier
            if left:  # the budget is spent: the old candidate waits its turn on the host path
                left.append(end)
            else:
                counts["host"] += 1
                touched = []
                lb = DS.try_insert_host(cand[end:end + 1])[0]
                if _host_walk(host, DS.S, int(lb[0]), end, touched):
                    touched += [int(s) for s in host.holders(end)]
                _patch_from_host(DS, host, touched, now)
        pos = end + 1
    if left:
        lbs = DS.try_insert_host(cand[left])[0]
        for k, j in enumerate(left):
            counts["host"] += 1
            was_old = bool(host.bad(j) and host.old(j))
            holders = [int(s) for s in host.holders(j)] if was_old else []
            if _host_walk(host, DS.S, int(lbs[k]), j, dirty):
                dirty += holders
        _patch_from_host(DS, host, dirty, now)
    return counts


SEARCH_MAX_BAD_NODES = 25  # dht.h:324


def mark_search_nodes(DS, host, nodes, pairs, now) -> dict:
    """The status changes of one tick carried to the device set with one DS.mark_nodes. nodes: the
    nodes whose isExpired() or time changed (any handles the host understands, one per ID); pairs: (search index, node)
    for every list entry whose `candidate` changed, or whose node un-expired while `candidate` is set. `host` holds the
    real searches: node_id(x) -> the 20 ID bytes, expired(x) -> node->isExpired(), removable(x, now) -> expired and
    time + NODE_EXPIRE_TIME < now, pair_flag(s, x, now) -> the flag byte of x in search s (KAD_SN_BAD from
    SearchNode::isBad(), KAD_SN_REMOVABLE as above). An expired node gives set BAD plus set or clear REMOVABLE at `now`,
    a live node clears both; an entry that is a candidate of its search needs its pair, as its BAD bit is not the node's.

    Returns the changed searches split by what Dht::searchStep would do with them next, from the counts alone: "expire"
    (leading bad entries >= min(n, SEARCH_MAX_BAD_NODES), dht.cpp:1451), else "short" (n - bad < SEARCH_NODES, the
    refill test of :1354), else "neither"; plus "hits" and "pair_found" as mark_nodes gives them."""
    both = KAD_SN_BAD | KAD_SN_REMOVABLE
    ids = np.zeros((len(nodes), 20), np.uint8)
    clear, setb = np.zeros(len(nodes), np.uint8), np.zeros(len(nodes), np.uint8)
    for j, x in enumerate(nodes):
        ids[j] = np.frombuffer(bytes(host.node_id(x)), np.uint8)
        if host.expired(x):
            setb[j] = both if host.removable(x, now) else KAD_SN_BAD
            clear[j] = both & ~setb[j]
        else:
            clear[j] = both
    pw = np.array([s for s, _ in pairs], np.uint32)
    pid = np.zeros((len(pairs), 20), np.uint8)
    pfl = np.zeros(len(pairs), np.uint8)
    for k, (s, x) in enumerate(pairs):
        pid[k] = np.frombuffer(bytes(host.node_id(x)), np.uint8)
        pfl[k] = host.pair_flag(int(s), x, now)
    r = DS.mark_nodes(ids, clear, setb, (pw, pid, pfl))
    out = {"expire": [], "short": [], "neither": [], "hits": r["hits"], "pair_found": r["pair_found"]}
    for s, (n, bad, lead, _) in zip(r["changed"], r["counts"]):
        if int(lead) >= min(int(n), SEARCH_MAX_BAD_NODES):
            out["expire"].append(int(s))
        elif int(n) - int(bad) < KAD_SEARCH_NODES:
            out["short"].append(int(s))
        else:
            out["neither"].append(int(s))
    return out


def _step_fields(out, stats=None) -> dict:
    """kad_step_out records as separate arrays."""
    c = out["counts"]
    r = {"picks": out["picks"].copy(), "n": (c & 0xFF).astype(np.uint8), "bad": ((c >> 8) & 0xFF).astype(np.uint8),
         "lead_bad": ((c >> 16) & 0xFF).astype(np.uint8), "solicited": (c >> 24).astype(np.uint8),
         "bits": out["bits"].copy()}
    if "listen" in (out.dtype.names or ()):
        r["listen"], r["announce"] = out["listen"].copy(), out["announce"].copy()
    if stats is not None:
        r["stats"] = stats
    return r


def search_step(node_flags, search_flags: int = 0, mode: int = 0) -> dict:
    """Dht::searchStep's decision on one list from its flag bytes, on the host without a device (kad_search_step):
    picks (int mask of list positions), n, bad, lead_bad, solicited and bits (ints)."""
    return _host_step("kad_search_step", STEP_OUT_DTYPE, "an unknown mode bit", node_flags, search_flags, mode)


def _host_step(call, dtype, bad_mode, node_flags, search_flags, mode) -> dict:
    fl = np.ascontiguousarray(node_flags, dtype=np.uint8).reshape(-1)
    out = np.zeros(1, dtype)
    rc = getattr(lib(), call)(fl.shape[0], ptr(fl) if fl.shape[0] else None, search_flags, mode, ptr(out))
    if rc != 0:
        raise ValueError(f"{call}: {rc}: more than 64 entries or {bad_mode}")
    return {k: int(v[0]) for k, v in _step_fields(out).items()}


def _host_step_batch(call, dtype, bad_mode, off, node_flags, search_flags, modes) -> dict:
    off = np.ascontiguousarray(off, dtype=np.uint32).reshape(-1)
    m = off.shape[0] - 1
    fl = np.ascontiguousarray(node_flags, dtype=np.uint8).reshape(-1)
    sf = None if search_flags is None else np.ascontiguousarray(search_flags, dtype=np.uint8).reshape(-1)
    md = None if modes is None else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)
    if m < 0 or fl.shape[0] < int(off[-1]) or any(a is not None and a.shape[0] != m for a in (sf, md)):
        raise ValueError("off needs m + 1 offsets into node_flags, search_flags and modes one byte per list")
    out = np.zeros(m, dtype)
    rc = getattr(lib(), call)(m, ptr(off), ptr(fl) if fl.shape[0] else None, ptr(sf), ptr(md), ptr(out))
    if rc != 0:
        raise ValueError(f"{call}: {rc}: offsets descending, a list of more than 64 entries or {bad_mode}")
    return _step_fields(out)


def search_step_batch(off, node_flags, search_flags=None, modes=None) -> dict:
    """search_step on m lists in CSR form (off (m + 1,) uint32 into node_flags; search_flags and modes (m,) uint8 or
    None), on the host (kad_search_step_batch): the arrays DeviceSearches.step returns, without stats."""
    return _host_step_batch("kad_search_step_batch", STEP_OUT_DTYPE, "an unknown mode bit", off, node_flags, search_flags,
                            modes)


def step_searches(DS, host, which, modes, now) -> dict:
    """Dht::searchStep's sends and expiries for the searches `which` (strictly ascending indices; None: all) of DS under
    modes (as DeviceSearches.step) with one device step, replayed on the host's searches. `host` holds
    the real searches in the same list order: step(s, mode, now) -> (picks, n, bad, lead_bad, solicited, bits), its own
    entry-by-entry searchStep on search s as it stands, changing nothing (picks the list positions it would send to, in
    order); send(s, pos, now) marks the get request to entry pos of search s as sent (getStatus[query] pending);
    expire(s) is Search::expire(). Every search's device answer is checked against host.step before anything is
    replayed; a difference raises. A search whose mode has KAD_STEP_APPLY then gets its sends and, unless the mode has
    KAD_STEP_NO_EXPIRE, its expiry on the host, as the device has applied them to its own copy; nothing is uploaded.

    Returns {"synced", "short", "done", "exhausted", "expire", "skipped"} (lists of searches), "picks" ({search: list
    positions}) and "stats"."""
    return _step_and_replay("step_searches", DS, DS.step, ("picks",), host, which, modes, now)


def _positions(mask) -> list:
    return [e for e in range(64) if (int(mask) >> e) & 1]


def _step_and_replay(name, DS, step, sends, host, which, modes, now) -> dict:
    """step_searches (sends = ("picks",)) and step_searches_full (("picks", "listen", "announce")): host.step's tuple and
    the device's answer both open with one list of positions per name in `sends`, then n, bad, lead_bad, solicited, bits."""
    idx = np.arange(DS.S, dtype=np.uint32) if which is None else np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
    m = idx.shape[0]
    md = np.zeros(m, np.uint8) if modes is None else (np.full(m, modes, np.uint8) if np.isscalar(modes)
                                                      else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1))
    want = [host.step(int(s), int(md[k]), now) for k, s in enumerate(idx)]
    r = step(which, md)
    out = {"synced": [], "short": [], "done": [], "exhausted": [], "expire": [], "skipped": []}
    out.update({f: {} for f in sends}, stats=r["stats"])
    names = ((KAD_STEP_SYNCED, "synced"), (KAD_STEP_SHORT, "short"), (KAD_STEP_DONE, "done"),
             (KAD_STEP_EXHAUSTED, "exhausted"), (KAD_STEP_EXPIRE, "expire"), (KAD_STEP_SKIPPED, "skipped"))
    for k, s in enumerate(idx):
        got = tuple(_positions(r[f][k]) for f in sends) + tuple(
            int(r[f][k]) for f in ("n", "bad", "lead_bad", "solicited", "bits"))
        w = want[k]
        if got != tuple(list(v) for v in w[:len(sends)]) + tuple(int(v) for v in w[len(sends):]):
            raise RuntimeError(f"{name}: search {int(s)} stepped to {w} on the host, {got} on the device")
    for k, s in enumerate(idx):
        s, bits = int(s), int(r["bits"][k])
        pos = dict(zip(sends, want[k]))
        for f in sends:
            if pos[f]:
                out[f][s] = list(pos[f])
        for bit, flag in names:
            if bits & bit:
                out[flag].append(s)
        if md[k] & KAD_STEP_APPLY:  # the reference's order: listens, probes, gets, then the expiry
            for e in pos.get("listen", ()):
                host.listen(s, e, now)
            for e in pos.get("announce", ()):
                host.announce_probe(s, e, now, bool(md[k] & KAD_STEP_PROBE_BLOCKS))
            for e in pos["picks"]:
                host.send(s, e, now)
            if bits & KAD_STEP_EXPIRE and not md[k] & KAD_STEP_NO_EXPIRE:
                host.expire(s)
    return out


def search_step_full(node_flags, search_flags: int = 0, mode: int = 0) -> dict:
    """search_step with the listen and announce sends (kad_search_step_full): also listen and announce (int masks)."""
    return _host_step("kad_search_step_full", STEP_FULL_OUT_DTYPE, "an invalid mode", node_flags, search_flags, mode)


def search_step_full_batch(off, node_flags, search_flags=None, modes=None) -> dict:
    """search_step_full on m lists in CSR form, as search_step_batch (kad_search_step_full_batch): the arrays
    DeviceSearches.step_full returns, without stats."""
    return _host_step_batch("kad_search_step_full_batch", STEP_FULL_OUT_DTYPE, "an invalid mode", off, node_flags,
                            search_flags, modes)


def _positions(mask) -> list:
    return [e for e in range(64) if (int(mask) >> e) & 1]


def step_searches_full(DS, host, which, modes, now) -> dict:
    """step_searches with the listen requests and announce probes, one kad_sr_step_full. `host` is
    step_searches' host whose step(s, mode, now) -> (picks, listen, announce, n, bad, lead_bad, solicited, bits) runs all
    three loops of its own searchStep entry by entry, changing nothing (three lists of positions, in order), and which
    has beside send(s, pos, now) and expire(s): listen(s, pos, now), the listen requests due on entry pos are sent
    (listenStatus[query] pending for every listener), and announce_probe(s, pos, now, blocks), the probe to entry pos is
    sent (getStatus[probe_query] pending; blocks: the mode had KAD_STEP_PROBE_BLOCKS). Every search's device answer is
    checked against host.step before anything is replayed; a difference raises. For a search whose mode has
    KAD_STEP_APPLY the listens, the probes and the gets are then replayed in the reference's order, and the expiry
    unless the mode has KAD_STEP_NO_EXPIRE.

    Returns step_searches' dict plus "listen" and "announce" ({search: list positions})."""
    return _step_and_replay("step_searches_full", DS, DS.step_full, ("picks", "listen", "announce"), host, which, modes,
                            now)


def refill_searches(DS: DeviceSearches, NC, host, which, now) -> dict:
    """Dht::refill (dht.cpp:1647-1668) for the searches `which` (strictly ascending indices) of DS from the NodeCache
    table NC, with one device refill. `host` holds the real searches: host.insert_row(s, row) runs
    sr.insertNode(node, now) on search s for every node index of the row in order and returns the mask of the
    inserts that returned true; host.state(s, now) -> (flags, node_ids, node_flags) is its state afterwards, with
    KAD_SN_REMOVABLE evaluated at `now`. The device has already applied the same walk to its own copy, so the host
    replays the whole row (a refused insert can still trim) and nothing is uploaded, except for the searches the
    device reports as KAD_SR_REFILL_OVERFLOW: those it left untouched, and they are patched from the host's lists,
    or the set is created again with larger slabs when a list no longer fits (as try_search_insert does).

    Returns {"refilled", "overflowed", "inserts", "untouched"}: searches the device refilled, searches it left to the
    host, inserts that returned true, searches whose row was empty."""
    which = np.ascontiguousarray(which, dtype=np.uint32).reshape(-1)
    counts = {"refilled": 0, "overflowed": 0, "inserts": 0, "untouched": 0}
    if which.shape[0] == 0:
        return counts
    rows, cnt, ins, status = DS.refill(NC, which)
    over = []
    for k, s in enumerate(which):
        if cnt[k] == 0:  # dht.cpp:1652-1656
            counts["untouched"] += 1
            continue
        mask = int(host.insert_row(int(s), rows[k, :cnt[k]]))
        counts["inserts"] += bin(mask).count("1")
        if status[k] == KAD_SR_REFILL_OVERFLOW:
            over.append(int(s))
            counts["overflowed"] += 1
        else:
            if mask != int(ins[k]):
                raise RuntimeError(f"refill_searches: search {int(s)} inserted {mask:#x}, the device {int(ins[k]):#x}")
            counts["refilled"] += 1

    def states(idx):
        flags, off, nid, nfl = [], [0], [np.zeros((0, 20), np.uint8)], [np.zeros(0, np.uint8)]
        for s in idx:
            fl, ids_s, nf_s = host.state(int(s), now)
            flags.append(fl)
            if len(ids_s):
                nid.append(_as_ids(ids_s))
                nfl.append(np.asarray(nf_s, dtype=np.uint8).reshape(-1))
            off.append(off[-1] + len(ids_s))
        return np.array(flags, np.uint8), np.array(off, np.uint32), np.concatenate(nid), np.concatenate(nfl)

    if over:
        flags, off, nid, nfl = states(over)
        longest = int(np.diff(off).max())
        if longest <= DS.cap:
            DS.patch(np.array(over, np.uint32), flags, off, nid, nfl)
        else:
            DS.recreate(*states(range(DS.S)), cap=max(longest, 2 * DS.cap))
    return counts


def start_searches(DS: DeviceSearches, NC, host, new_ids, now) -> dict:
    """Dht::search (dht.cpp:1673-1735) for a batch of new search IDs ((n, 20) uint8, distinct, none live): the host
    emplaces the empty searches (host.add(ids); its indices follow the ascending ID order of the map), the device set
    takes them with one DeviceSearches.apply, and refill_searches fills them from the NodeCache table NC (:1728).
    Nothing but the IDs is uploaded. Returns refill_searches' counts plus "new_index", the index of every new search
    in the order of new_ids."""
    ids = _as_ids(new_ids)
    host.add(ids)
    _, new_index = DS.apply(ins_ids=ids)
    counts = refill_searches(DS, NC, host, np.sort(new_index), now)
    counts["new_index"] = new_index
    return counts


def expire_searches(DS: DeviceSearches, host, erase):
    """Dht::expireSearches (dht.cpp:1060-1074) for the searches `erase` (strictly ascending indices): host.erase(erase)
    drops them from the host's map and one DeviceSearches.apply from the device set. Returns remap."""
    erase = np.ascontiguousarray(erase, dtype=np.uint32).reshape(-1)
    host.erase(erase)
    return DS.apply(erase=erase)[0]
