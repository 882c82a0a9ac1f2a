"""DeviceTable: a routing-table / NodeCache snapshot resident in HBM, queried in batches.

Thin Python plumbing over the C ABI (include/kadgpu.h) for tests and bench.py. The drop-in
host interface for OpenDHT's C++ code is include/kadgpu.hpp (RoutingTable::findClosestNodes,
NodeCache::getCachedNodes, Dht-style findClosestNodes(id, af, count)).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KAD_TABLE_EAGER, KAD_TABLE_NO_SLOT_LINES, KAD_TABLE_SORTED, check, lib, ptr


def _as_ids(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1:
        a = a.reshape(-1, 20)
    if a.ndim != 2 or a.shape[1] != 20:
        raise ValueError(f"ids must be (n, 20) uint8, got {a.shape}")
    return a


def _self_id(self_id) -> np.ndarray:
    a = np.ascontiguousarray(np.frombuffer(bytes(self_id), np.uint8) if isinstance(self_id, (bytes, bytearray))
                             else self_id, dtype=np.uint8).reshape(-1)
    if a.shape != (20,):
        raise ValueError(f"self_id must be 20 bytes, got {a.shape}")
    return a


def _stream_of(t, stream):
    if stream is not None:  # a raw hipStream_t handle or a torch.cuda.Stream
        return C.c_void_p(getattr(stream, "cuda_stream", stream))
    import torch

    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class DeviceTable:
    """One address family's RoutingTable and/or NodeCache map, snapshotted at `now`.

    ids            (n, 20) uint8, InfoHash bytes; grouped by bucket in list order
    status         (n,) uint8, bit0 Node::isGood(now), bit1 Node::isExpired()
    bucket_first   (B, 20) uint8 ascending, or None for a NodeCache-only table
    bucket_offset  (B+1,) uint32
    sorted         ids strictly ascending (enables NodeCache queries)
    eager          build every line set now (default: the count <= 8 lines; the others on first use)
    slot_lines     general-line tables: build slot lines (KAD_TABLE_NO_SLOT_LINES when False)
    """

    def __init__(self, ids, status, bucket_first=None, bucket_offset=None, *, device: int = 0,
                 index_base: int = 0, sorted: bool = False, eager: bool = False,
                 slot_lines: bool = True):
        L = lib()
        ids = _as_ids(ids)
        status = np.ascontiguousarray(status, dtype=np.uint8)
        n = ids.shape[0]
        if status.shape != (n,):
            raise ValueError("status must have one byte per node")
        if bucket_first is not None:
            bucket_first = _as_ids(bucket_first)
            bucket_offset = np.ascontiguousarray(bucket_offset, dtype=np.uint32)
            B = bucket_first.shape[0]
            if bucket_offset.shape != (B + 1,):
                raise ValueError("bucket_offset must have B+1 entries")
        else:
            B = 0
        h = C.c_void_p()
        rc = L.kad_table_create(C.byref(h), device, n, ptr(ids), ptr(status), B,
                                ptr(bucket_first) if B else None, ptr(bucket_offset) if B else None,
                                index_base, (KAD_TABLE_SORTED if sorted else 0) | (KAD_TABLE_EAGER if eager else 0)
                                | (0 if slot_lines else KAD_TABLE_NO_SLOT_LINES))
        check(rc, "kad_table_create")
        self._h = h
        self.device = device
        self.n = n
        self.B = B
        self.index_base = index_base

    # -- lifetime ------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().kad_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> dict:
        inf = _lib.table_info()
        check(lib().kad_table_get_info(self._h, C.byref(inf)), "kad_table_get_info")
        out = {f: getattr(inf, f) for f, _ in inf._fields_}
        built = C.c_uint32()
        nb = (C.c_uint64 * 4)()
        ms = (C.c_float * 4)()
        check(lib().kad_table_line_sets(self._h, C.byref(built), nb, ms), "kad_table_line_sets")
        out["line_sets"] = {name: {"built": bool(built.value & (1 << k)), "bytes": int(nb[k]), "build_ms": float(ms[k])}
                            for k, name in enumerate(("rt16", "rt32", "nc16", "nc32"))}
        return out

    def serve(self, idle_us: int = 2000) -> None:
        """Resident query service (kad_table_serve): host batches of up to 64 queries with count <= 64 are answered
        by a workgroup that stays on the GPU, without a launch per call. idle_us = 0 turns it off."""
        check(lib().kad_table_serve(self._h, idle_us), "kad_table_serve")

    def serve_stats(self) -> dict:
        """kad_table_serve_stats: launches, requests, and the last request's header reads and device time."""
        st = _lib.serve_stats()
        check(lib().kad_table_serve_stats(self._h, C.byref(st)), "kad_table_serve_stats")
        return {f: getattr(st, f) for f, _ in st._fields_}

    def prepare(self, sets: int = _lib.KAD_LINES_ALL) -> None:
        """Build the line sets `sets` (KAD_LINES_*) now instead of on first use (e.g. before a graph capture)."""
        check(lib().kad_table_prepare(self._h, sets), "kad_table_prepare")

    # -- status --------------------------------------------------------------------------
    def update_status(self, status) -> None:
        status = np.ascontiguousarray(status, dtype=np.uint8)
        check(lib().kad_table_update_status(self._h, ptr(status)), "kad_table_update_status")

    def set_times(self, time_ns, reply_time_ns, expired) -> None:
        a = np.ascontiguousarray(time_ns, dtype=np.int64)
        b = np.ascontiguousarray(reply_time_ns, dtype=np.int64)
        e = np.ascontiguousarray(expired, dtype=np.uint8)
        check(lib().kad_table_set_times(self._h, ptr(a), ptr(b), ptr(e)), "kad_table_set_times")

    def patch_status(self, nodes, status) -> None:
        """Incremental status update of the listed nodes (kad_table_patch_status)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        status = np.ascontiguousarray(status, dtype=np.uint8)
        if nodes.shape != status.shape:
            raise ValueError("nodes and status must have the same length")
        check(lib().kad_table_patch_status(self._h, nodes.shape[0], ptr(nodes), ptr(status)), "kad_table_patch_status")

    def patch_times(self, nodes, time_ns, reply_time_ns, expired) -> None:
        """New liveness of the listed nodes (kad_table_patch_times); applied at the next refresh_status."""
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        a = np.ascontiguousarray(time_ns, dtype=np.int64)
        b = np.ascontiguousarray(reply_time_ns, dtype=np.int64)
        e = np.ascontiguousarray(expired, dtype=np.uint8)
        if not (nodes.shape == a.shape == b.shape == e.shape):
            raise ValueError("patch arrays must have the same length")
        check(lib().kad_table_patch_times(self._h, nodes.shape[0], ptr(nodes), ptr(a), ptr(b), ptr(e)),
              "kad_table_patch_times")

    def refresh_status(self, now_ns: int, stream=None) -> None:
        check(lib().kad_table_refresh_status(self._h, C.c_int64(now_ns), _stream_of(self, stream)),
              "kad_table_refresh_status")

    def refresh_diag(self) -> dict:
        """kad_table_refresh_diag: the small refresh's spin timeouts, lines its last block built, guard errors."""
        d = _lib.refresh_diag()
        check(lib().kad_table_refresh_diag(self._h, C.byref(d)), "kad_table_refresh_diag")
        return {f: getattr(d, f) for f, _ in d._fields_}

    def apply(self, ops, new_ids=None, new_status=None, remap=None):
        """Incremental mirror (kad_table_apply): ops (m, 3) uint32 rows (kind, a, b). Returns the new
        nodes' indices (host uint32); `remap` (device int32 tensor, old n) receives every old node's
        new index."""
        ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 3)
        nid = _as_ids(new_ids) if new_ids is not None and len(new_ids) else np.zeros((0, 20), np.uint8)
        nst = np.ascontiguousarray(new_status if new_status is not None else np.zeros(0), dtype=np.uint8)
        out = np.zeros(max(nid.shape[0], 1), np.uint32)
        check(lib().kad_table_apply(self._h, ptr(ops), ops.shape[0], ptr(nid), ptr(nst), nid.shape[0], ptr(remap),
                                    ptr(out)), "kad_table_apply")
        inf = self.info()
        self.n, self.B = inf["n_nodes"], inf["n_buckets"]
        return out[:nid.shape[0]]

    def sweep(self, incoming: bool = False, want_nodes: bool = True, want_buckets: bool = True, cap_nodes=None,
              cap_buckets=None, stream=None, out=None):
        """Dht::getNodesStats and the scan of Dht::expireBuckets in one device pass (kad_table_sweep) over the current
        status snapshot. Returns a dict: `totals` (the kad_sweep_totals fields as ints), `expired_nodes` (int32 device
        tensor view of uint32: the EXPIRED nodes ascending, plus index_base) and `changed_buckets` (int32 device tensor:
        the buckets holding one), each cut to min(count, cap), or None when not wanted. cap_* default to n / B. out: a
        (nodes, buckets) pair of int32 device tensors to write into (at least cap entries each). Waits for the
        stream to read the totals."""
        import torch

        dev = torch.device("cuda", self.device)
        s = _stream_of(self, stream)
        cn = (self.n if cap_nodes is None else int(cap_nodes)) if want_nodes else 0
        cb = (self.B if cap_buckets is None else int(cap_buckets)) if want_buckets else 0
        nodes, buckets = out if out is not None else (None, None)
        if nodes is None and cn:
            nodes = torch.empty((cn,), dtype=torch.int32, device=dev)
        if buckets is None and cb:
            buckets = torch.empty((cb,), dtype=torch.int32, device=dev)
        tot = torch.empty((8,), dtype=torch.int32, device=dev)
        check(lib().kad_table_sweep(self._h, _lib.KAD_SWEEP_INCOMING if incoming else 0, ptr(tot),
                                    ptr(nodes) if cn else None, cn, ptr(buckets) if cb else None, cb, s),
              "kad_table_sweep")
        if stream is None:
            torch.cuda.current_stream(dev).synchronize()
        elif hasattr(stream, "synchronize"):
            stream.synchronize()
        else:
            torch.cuda.ExternalStream(int(stream), device=dev).synchronize()
        vals = tot.cpu().numpy().view(np.uint32)
        totals = {f: int(vals[k]) for k, (f, _) in enumerate(_lib.sweep_totals._fields_)}
        empty = torch.empty((0,), dtype=torch.int32, device=dev)
        return {"totals": totals,
                "expired_nodes": (nodes[:min(totals["expired"], cn)] if cn else empty) if want_nodes else None,
                "changed_buckets": (buckets[:min(totals["changed_buckets"], cb)] if cb else empty) if want_buckets
                else None}

    def sweep_host(self, incoming: bool = False, want_nodes: bool = True, want_buckets: bool = True, cap_nodes=None,
                   cap_buckets=None):
        """sweep on host buffers, synchronous (kad_table_sweep_host): the same dict with numpy uint32 arrays."""
        cn = (self.n if cap_nodes is None else int(cap_nodes)) if want_nodes else 0
        cb = (self.B if cap_buckets is None else int(cap_buckets)) if want_buckets else 0
        nodes = np.zeros(max(cn, 1), np.uint32)
        buckets = np.zeros(max(cb, 1), np.uint32)
        tot = _lib.sweep_totals()
        check(lib().kad_table_sweep_host(self._h, _lib.KAD_SWEEP_INCOMING if incoming else 0, C.byref(tot),
                                         ptr(nodes) if cn else None, cn, ptr(buckets) if cb else None, cb),
              "kad_table_sweep_host")
        totals = {f: int(getattr(tot, f)) for f, _ in tot._fields_}
        return {"totals": totals,
                "expired_nodes": nodes[:min(totals["expired"], cn)] if want_nodes else None,
                "changed_buckets": buckets[:min(totals["changed_buckets"], cb)] if want_buckets else None}

    # -- bucket times and Dht::bucketMaintenance's scan -----------------------------------------
    def set_bucket_times(self, time_ns=None) -> None:
        """Upload every Bucket::time (kad_table_set_bucket_times): (B,) int64 ns, INT64_MIN for time_point::min();
        None sets every bucket to INT64_MIN."""
        if time_ns is None:
            check(lib().kad_table_set_bucket_times(self._h, None), "kad_table_set_bucket_times")
            return
        a = np.ascontiguousarray(time_ns, dtype=np.int64)
        if a.shape != (self.B,):
            raise ValueError("one time per bucket")
        check(lib().kad_table_set_bucket_times(self._h, ptr(a)), "kad_table_set_bucket_times")

    def patch_bucket_times(self, buckets, time_ns) -> None:
        """buckets[j] gets time_ns[j] (kad_table_patch_bucket_times); the later entry of a bucket listed twice wins."""
        b = np.ascontiguousarray(buckets, dtype=np.uint32)
        a = np.ascontiguousarray(time_ns, dtype=np.int64)
        if b.shape != a.shape or b.ndim != 1:
            raise ValueError("buckets and time_ns must be lists of the same length")
        check(lib().kad_table_patch_bucket_times(self._h, b.shape[0], ptr(b), ptr(a)), "kad_table_patch_bucket_times")

    def bucket_times(self) -> np.ndarray:
        """The bucket times as a host (B,) int64 array (kad_table_get_bucket_times)."""
        out = np.zeros(max(self.B, 1), np.int64)
        check(lib().kad_table_get_bucket_times(self._h, ptr(out)), "kad_table_get_bucket_times")
        return out[:self.B]

    def touch_buckets(self, ids, now_ns: int, want_bucket: bool = True, stream=None):
        """Dht::onReportedAddr per ID (kad_table_touch_buckets): findBucket(id)->time = now_ns. ids: a (q, 20) uint8
        device tensor (enqueued on the stream; returns the int32 device tensor of buckets, or None), or host IDs
        (synchronous, kad_table_touch_buckets_host; returns a uint32 array, or None)."""
        import torch

        if torch.is_tensor(ids):
            q = ids.shape[0]
            out = torch.empty((q,), dtype=torch.int32, device=ids.device) if want_bucket else None
            check(lib().kad_table_touch_buckets(self._h, ptr(ids), q, C.c_int64(now_ns), ptr(out),
                                                _stream_of(self, stream)), "kad_table_touch_buckets")
            return out
        t = _as_ids(ids)
        out = np.empty((t.shape[0],), dtype=np.uint32) if want_bucket else None
        check(lib().kad_table_touch_buckets_host(self._h, ptr(t), t.shape[0], C.c_int64(now_ns), ptr(out)),
              "kad_table_touch_buckets_host")
        return out

    def maintenance(self, now_ns: int, first_bucket: int = 0, cap=None, stream=None, out=None):
        """Dht::bucketMaintenance's scan (kad_table_maintenance): {"totals": the kad_maint_totals fields as ints,
        "records": a (min(candidates, cap), 2) int32 device tensor of (bucket, kind) rows}. cap defaults to the
        buckets from first_bucket on. out: an int32 device tensor of at least cap rows to write into. Waits for the
        stream to read the totals."""
        import torch

        dev = torch.device("cuda", self.device)
        s = _stream_of(self, stream)
        cap = max(self.B - int(first_bucket), 0) if cap is None else int(cap)
        if out is None and cap:
            out = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        tot = torch.empty((8,), dtype=torch.int32, device=dev)
        check(lib().kad_table_maintenance(self._h, C.c_int64(now_ns), int(first_bucket), ptr(tot),
                                          ptr(out) if cap else None, cap, s), "kad_table_maintenance")
        if stream is None:
            torch.cuda.current_stream(dev).synchronize()
        elif hasattr(stream, "synchronize"):
            stream.synchronize()
        else:
            torch.cuda.ExternalStream(int(stream), device=dev).synchronize()
        vals = tot.cpu().numpy().view(np.uint32)
        totals = {f: int(vals[k]) for k, (f, _) in enumerate(_lib.maint_totals._fields_)}
        m = min(totals["candidates"], cap)
        return {"totals": totals,
                "records": out[:m] if cap else torch.empty((0, 2), dtype=torch.int32, device=dev)}

    def maintenance_host(self, now_ns: int, first_bucket: int = 0, cap=None):
        """maintenance on host buffers, synchronous (kad_table_maintenance_host): records as a numpy record array
        (MAINT_REC_DTYPE)."""
        cap = max(self.B - int(first_bucket), 0) if cap is None else int(cap)
        rec = np.zeros(max(cap, 1), _lib.MAINT_REC_DTYPE)
        tot = _lib.maint_totals()
        check(lib().kad_table_maintenance_host(self._h, C.c_int64(now_ns), int(first_bucket), C.byref(tot),
                                               ptr(rec) if cap else None, cap), "kad_table_maintenance_host")
        totals = {f: int(getattr(tot, f)) for f, _ in tot._fields_}
        return {"totals": totals, "records": rec[:min(totals["candidates"], cap)]}

    def expire(self, remap=None):
        """Dht::expireBuckets on the device copy (kad_table_expire): every KAD_STATUS_EXPIRED node leaves; node times
        and wire records stay attached to the survivors. `remap` (device int32 tensor or host uint32 array, old n)
        receives every old node's new index. Returns (removed, changed_buckets): host uint32 arrays with the old
        indices (plus index_base) of the removed nodes and the buckets that held them."""
        removed = np.empty(max(self.n, 1), np.uint32)  # not zeroed: only the first nr / nb entries are written and returned
        buckets = np.empty(max(self.B, 1), np.uint32)
        nr, nb = C.c_uint32(0), C.c_uint32(0)
        check(lib().kad_table_expire(self._h, ptr(remap), ptr(removed), self.n, C.byref(nr), ptr(buckets), self.B,
                                     C.byref(nb)), "kad_table_expire")
        inf = self.info()
        self.n, self.B = inf["n_nodes"], inf["n_buckets"]
        return removed[:nr.value], buckets[:nb.value]

    def nc_apply(self, erase=None, ins_ids=None, ins_status=None):
        """NodeCache map mutations (kad_nc_apply) on a NodeCache-only table: erase the listed node indices,
        insert new IDs. Returns (remap (old n,) uint32, new_index (n_ins,) uint32), both host arrays."""
        er = np.ascontiguousarray(erase if erase is not None else np.zeros(0), dtype=np.uint32)
        nid = _as_ids(ins_ids) if ins_ids is not None and len(ins_ids) else np.zeros((0, 20), np.uint8)
        nst = np.ascontiguousarray(ins_status if ins_status is not None else np.zeros(0), dtype=np.uint8)
        if nst.shape[0] != nid.shape[0]:
            raise ValueError("one status byte per inserted ID")
        remap = np.zeros(max(self.n, 1), np.uint32)
        new_index = np.zeros(max(nid.shape[0], 1), np.uint32)
        check(lib().kad_nc_apply(self._h, ptr(er), er.shape[0], ptr(nid), ptr(nst), nid.shape[0], ptr(remap),
                                 ptr(new_index)), "kad_nc_apply")
        old_n = self.n
        self.n = self.info()["n_nodes"]
        return remap[:old_n], new_index[:nid.shape[0]]

    def export(self):
        """(ids, status, bucket_first, bucket_offset) host arrays of the device table."""
        inf = self.info()
        n, B = inf["n_nodes"], inf["n_buckets"]
        ids = np.zeros((max(n, 1), 20), np.uint8)
        st = np.zeros(max(n, 1), np.uint8)
        first = np.zeros((max(B, 1), 20), np.uint8)
        off = np.zeros(B + 1, np.uint32)
        check(lib().kad_table_export(self._h, ptr(ids), ptr(st), ptr(first), ptr(off)), "kad_table_export")
        return ids[:n], st[:n], first[:B], off

    def export_lines(self, which: int):
        """A derived array (KAD_LINESET_*) as host bytes (kad_table_export_lines), or None if absent."""
        nb = C.c_uint64(0)
        check(lib().kad_table_export_lines(self._h, which, None, C.byref(nb)), "kad_table_export_lines")
        if nb.value == 0:
            return None
        out = np.empty(nb.value, np.uint8)
        check(lib().kad_table_export_lines(self._h, which, ptr(out), C.byref(nb)), "kad_table_export_lines")
        return out

    def export_status(self):
        """The device's status bytes (n,), e.g. after refresh_status."""
        st = np.zeros(max(self.n, 1), np.uint8)
        check(lib().kad_table_export(self._h, None, ptr(st), None, None), "kad_table_export")
        return st[:self.n]

    def set_addrs(self, addrs) -> None:
        """Node address records (n, 6) for IPv4 (in_addr + port bytes) or (n, 18) for IPv6."""
        addrs = np.ascontiguousarray(addrs, dtype=np.uint8)
        if addrs.ndim != 2 or addrs.shape[0] != self.n or addrs.shape[1] not in (6, 18):
            raise ValueError(f"addrs must be (n, 6) or (n, 18) uint8, got {addrs.shape}")
        check(lib().kad_table_set_addrs(self._h, addrs.shape[1], ptr(addrs)), "kad_table_set_addrs")
        self.addr_len = addrs.shape[1]

    def buffer_nodes(self, targets, idx, cnt=None, stream=None):
        """NetworkEngine::bufferNodes per query (network_engine.cpp:942-974) over device tensors: the
        candidates of row i of idx (the first min(cnt[i], k) entries, or all k without cnt) sorted by XOR
        distance, the first 8 packed as 26- / 38-byte records. Entries equal to KAD_NO_NODE or outside
        [index_base, index_base + n) are skipped wherever they stand, and what follows them still counts;
        equal distances keep row order. Returns (out (q, 8 * rec) uint8, zero beyond the records, n (q,))."""
        import torch

        q, k = idx.shape
        rec = 20 + self.addr_len
        out = torch.zeros((q, 8 * rec), dtype=torch.uint8, device=targets.device)
        n = torch.empty((q,), dtype=torch.uint8, device=targets.device)
        check(lib().kad_buffer_nodes_batch(self._h, ptr(targets), q, ptr(idx), ptr(cnt), k, ptr(out), ptr(n),
                                           _stream_of(self, stream)), "kad_buffer_nodes_batch")
        return out, n

    # -- device-pointer batch queries (torch tensors on this table's device) ---------------
    def rt_closest(self, targets, count: int, out_idx=None, out_cnt=None, stream=None):
        """RoutingTable::findClosestNodes over a (q, 20) uint8 device tensor of targets.
        Returns (idx int32 view of uint32 (q, count), cnt uint8 (q,))."""
        import torch

        q = targets.shape[0]
        if out_idx is None:
            out_idx = torch.empty((q, count), dtype=torch.int32, device=targets.device)
        if out_cnt is None:
            out_cnt = torch.empty((q,), dtype=torch.uint8, device=targets.device)
        check(lib().kad_rt_closest_batch(self._h, ptr(targets), q, count, ptr(out_idx), ptr(out_cnt),
                                         _stream_of(self, stream)), "kad_rt_closest_batch")
        return out_idx, out_cnt

    def nc_closest(self, targets, count: int, out_idx=None, out_cnt=None, stream=None):
        """NodeCache::getCachedNodes over a (q, 20) uint8 device tensor of targets."""
        import torch

        q = targets.shape[0]
        if out_idx is None:
            out_idx = torch.empty((q, count), dtype=torch.int32, device=targets.device)
        if out_cnt is None:
            out_cnt = torch.empty((q,), dtype=torch.uint8, device=targets.device)
        check(lib().kad_nc_closest_batch(self._h, ptr(targets), q, count, ptr(out_idx), ptr(out_cnt),
                                         _stream_of(self, stream)), "kad_nc_closest_batch")
        return out_idx, out_cnt

    def find_bucket(self, targets, out=None, stream=None):
        import torch

        q = targets.shape[0]
        if out is None:
            out = torch.empty((q,), dtype=torch.int32, device=targets.device)
        check(lib().kad_rt_find_bucket_batch(self._h, ptr(targets), q, ptr(out), _stream_of(self, stream)),
              "kad_rt_find_bucket_batch")
        return out

    def rt_responsible(self, targets, self_id, count: int = 8, min_nodes: int = 1, out=None, stream=None):
        """Storage-responsibility verdicts (kad_rt_responsible_batch; Dht::maintainStorage count 8 / min_nodes 1,
        Dht::onAnnounce count 14 / min_nodes 8) over a (q, 20) uint8 device tensor of targets: one uint8 per
        target, KAD_RESP_FAR where the last of its `count` closest good nodes is closer to it than self_id."""
        import torch

        q = targets.shape[0]
        sid = _self_id(self_id)
        if out is None:
            out = torch.empty((q,), dtype=torch.uint8, device=targets.device)
        check(lib().kad_rt_responsible_batch(self._h, ptr(sid), ptr(targets), q, count, min_nodes, ptr(out),
                                             _stream_of(self, stream)), "kad_rt_responsible_batch")
        return out

    def rt_triage(self, ids, self_id=None, bootstrap: bool = False, want_bucket: bool = False, out=None, stream=None):
        """Dht::onNewNode(node, 0) triage verdicts (kad_rt_triage_batch) over a (q, 20) uint8 device tensor of
        candidate IDs, against the current status snapshot: (verdict (q,) uint8 = KAD_NN_* kind | KAD_NN_MYBUCKET,
        node (q,) int32, bucket (q,) int32 or None). self_id None: no bucket is "mine". out: the same tuple of
        tensors to write into."""
        import torch

        q = ids.shape[0]
        sid = None if self_id is None else _self_id(self_id)
        verdict, node, bucket = out if out is not None else (None, None, None)
        if verdict is None:
            verdict = torch.empty((q,), dtype=torch.uint8, device=ids.device)
        if node is None:
            node = torch.empty((q,), dtype=torch.int32, device=ids.device)
        if bucket is None and want_bucket:
            bucket = torch.empty((q,), dtype=torch.int32, device=ids.device)
        check(lib().kad_rt_triage_batch(self._h, ptr(sid), ptr(ids), q, _lib.KAD_NN_BOOTSTRAP if bootstrap else 0,
                                        ptr(verdict), ptr(node), ptr(bucket), _stream_of(self, stream)),
              "kad_rt_triage_batch")
        return verdict, node, bucket

    # -- host-pointer synchronous queries ---------------------------------------------------
    def rt_triage_host(self, ids, self_id=None, bootstrap: bool = False, want_bucket: bool = False):
        """rt_triage over host IDs, synchronous (kad_rt_triage_batch_host): (verdict uint8, node uint32, bucket
        uint32 or None) host arrays."""
        t = _as_ids(ids)
        q = t.shape[0]
        sid = None if self_id is None else _self_id(self_id)
        verdict = np.empty((q,), dtype=np.uint8)
        node = np.empty((q,), dtype=np.uint32)
        bucket = np.empty((q,), dtype=np.uint32) if want_bucket else None
        check(lib().kad_rt_triage_batch_host(self._h, ptr(sid), ptr(t), q, _lib.KAD_NN_BOOTSTRAP if bootstrap else 0,
                                             ptr(verdict), ptr(node), ptr(bucket)), "kad_rt_triage_batch_host")
        return verdict, node, bucket

    def rt_responsible_host(self, targets, self_id, count: int = 8, min_nodes: int = 1):
        """rt_responsible over host targets, synchronous (kad_rt_responsible_batch_host). Returns (q,) uint8."""
        t = _as_ids(targets)
        q = t.shape[0]
        sid = _self_id(self_id)
        out = np.empty((q,), dtype=np.uint8)
        check(lib().kad_rt_responsible_batch_host(self._h, ptr(sid), ptr(t), q, count, min_nodes, ptr(out)),
              "kad_rt_responsible_batch_host")
        return out

    def rt_closest_host(self, targets, count: int):
        t = _as_ids(targets)
        q = t.shape[0]
        idx = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty((q,), dtype=np.uint8)
        check(lib().kad_rt_closest_batch_host(self._h, ptr(t), q, count, ptr(idx), ptr(cnt)),
              "kad_rt_closest_batch_host")
        return idx, cnt

    def nc_closest_host(self, targets, count: int):
        t = _as_ids(targets)
        q = t.shape[0]
        idx = np.empty((q, count), dtype=np.uint32)
        cnt = np.empty((q,), dtype=np.uint8)
        check(lib().kad_nc_closest_batch_host(self._h, ptr(t), q, count, ptr(idx), ptr(cnt)),
              "kad_nc_closest_batch_host")
        return idx, cnt


def maint_scan_host(bucket_offset, bucket_first, time_ns, now_ns: int, first_bucket: int = 0, cap=None):
    """Dht::bucketMaintenance's scan over host arrays, without a GPU (kad_maint_scan_host, the twin of
    DeviceTable.maintenance): bucket_offset (B+1,) uint32, bucket_first (B, 20) uint8, time_ns (B,) int64 or None (every
    bucket at INT64_MIN). The same dict as DeviceTable.maintenance_host."""
    off = np.ascontiguousarray(bucket_offset, dtype=np.uint32)
    B = off.shape[0] - 1
    first = _as_ids(bucket_first) if B else np.zeros((0, 20), np.uint8)
    if first.shape[0] != B:
        raise ValueError("bucket_offset must have B+1 entries")
    tm = None if time_ns is None else np.ascontiguousarray(time_ns, dtype=np.int64)
    if tm is not None and tm.shape != (B,):
        raise ValueError("one time per bucket")
    cap = max(B - int(first_bucket), 0) if cap is None else int(cap)
    rec = np.zeros(max(cap, 1), _lib.MAINT_REC_DTYPE)
    tot = _lib.maint_totals()
    rc = lib().kad_maint_scan_host(B, ptr(off), ptr(first), ptr(tm), C.c_int64(now_ns), int(first_bucket),
                                   C.byref(tot), ptr(rec) if cap else None, cap)
    if rc != 0:
        raise _lib.KadError(rc, "kad_maint_scan_host", "bad argument")
    totals = {f: int(getattr(tot, f)) for f, _ in tot._fields_}
    return {"totals": totals, "records": rec[:min(totals["candidates"], cap)]}


def rt_closest_dual(table4: DeviceTable | None, table6: DeviceTable | None, targets, af, count: int,
                    stream=None):
    """Per-query family select (af 0 -> v4, 1 -> v6), as Dht::onGetValues asks both tables."""
    import torch

    q = targets.shape[0]
    out_idx = torch.empty((q, count), dtype=torch.int32, device=targets.device)
    out_cnt = torch.empty((q,), dtype=torch.uint8, device=targets.device)
    s = C.c_void_p(stream) if stream is not None else C.c_void_p(
        torch.cuda.current_stream(targets.device).cuda_stream)
    check(lib().kad_rt_closest_batch_dual(table4.handle if table4 else None, table6.handle if table6 else None,
                                          ptr(targets), ptr(af), q, count, ptr(out_idx), ptr(out_cnt), s),
          "kad_rt_closest_batch_dual")
    return out_idx, out_cnt


def rt_responsible_dual(table4: DeviceTable | None, table6: DeviceTable | None, targets, self_id, count: int = 8,
                        min_nodes: int = 1, stream=None):
    """Dht::maintainStorage's verdict from both families in one launch (kad_rt_responsible_batch_dual): one uint8
    per target, bit 0 (KAD_RESP_FAR4) far in table4, bit 1 (KAD_RESP_FAR6) far in table6; None = an empty table.
    3 is maintainStorage's "discard"."""
    import torch

    q = targets.shape[0]
    sid = _self_id(self_id)
    out = torch.empty((q,), dtype=torch.uint8, device=targets.device)
    s = C.c_void_p(getattr(stream, "cuda_stream", stream)) if stream is not None else C.c_void_p(
        torch.cuda.current_stream(targets.device).cuda_stream)
    check(lib().kad_rt_responsible_batch_dual(table4.handle if table4 else None, table6.handle if table6 else None,
                                              ptr(sid), ptr(targets), q, count, min_nodes, ptr(out), s),
          "kad_rt_responsible_batch_dual")
    return out


def nc_closest_dual(table4: DeviceTable | None, table6: DeviceTable | None, targets, af, count: int, stream=None):
    """NodeCache::getCachedNodes with a per-query family (af 0 -> cache_4, 1 -> cache_6; node_cache.cpp:36-66)."""
    import torch

    q = targets.shape[0]
    out_idx = torch.empty((q, count), dtype=torch.int32, device=targets.device)
    out_cnt = torch.empty((q,), dtype=torch.uint8, device=targets.device)
    s = C.c_void_p(stream) if stream is not None else C.c_void_p(
        torch.cuda.current_stream(targets.device).cuda_stream)
    check(lib().kad_nc_closest_batch_dual(table4.handle if table4 else None, table6.handle if table6 else None,
                                          ptr(targets), ptr(af), q, count, ptr(out_idx), ptr(out_cnt), s),
          "kad_nc_closest_batch_dual")
    return out_idx, out_cnt
