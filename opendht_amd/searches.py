"""Device set of one family's live searches and the batch form of Dht::trySearchInsert.

Dht::trySearchInsert(node) (dht.cpp:816-849) takes lower_bound(node->id) in the family's search map and calls
Search::insertNode forwards and backwards until the first search that refuses. kad_sr_try_insert_batch gives, for a
whole tick of candidates and one snapshot of the searches, which searches would take each candidate and why each
walk stopped; try_search_insert turns those verdicts into the exact sequential result while the host touches only
the searches that accept.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (KAD_NO_NODE, KAD_SEARCH_NODES, KAD_SR_REFILL_OVERFLOW, KAD_SR_STOP_END, KAD_SR_STOP_FAR,
                   KAD_SR_STOP_FAR_EXPIRED, KAD_SR_STOP_KNOWN, check, lib, ptr)
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
