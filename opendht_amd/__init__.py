"""opendht_amd — MI355X-native batched Kademlia closest-node engine for OpenDHT's lookup path.

The hot path (RoutingTable::findClosestNodes / findBucket, NodeCache::getCachedNodes and the
InfoHash XOR primitives) runs as hand-written HIP kernels for gfx950 in libkadgpu.so, behind
the C ABI of include/kadgpu.h. This package is thin Python plumbing for tests and the bench;
the drop-in host interface for OpenDHT's C++ code is include/kadgpu.hpp.
"""
from ._lib import (KAD_MAX_COUNT, KAD_NO_NODE, KAD_SEARCH_NODES, KAD_STATUS_EXPIRED, KAD_STATUS_GOOD,
                   KAD_TARGET_NODES, KadError, lib)
from .infohash import InfoHash, zeroes
from ._lib import KAD_RESP_FAR, KAD_RESP_FAR4, KAD_RESP_FAR6
from ._lib import (KAD_NN_BOOTSTRAP, KAD_NN_FULL, KAD_NN_INSERT, KAD_NN_KIND_MASK, KAD_NN_KNOWN, KAD_NN_MYBUCKET,
                   KAD_NN_NONE, KAD_NN_REPLACE, KAD_NN_SPLIT)
from ._lib import (KAD_SN_BAD, KAD_SR_EXPIRED, KAD_SR_STOP_END, KAD_SR_STOP_FAR, KAD_SR_STOP_FAR_EXPIRED,
                   KAD_SR_STOP_KNOWN)
from ._lib import KAD_SN_REMOVABLE, KAD_SR_REFILL_OK, KAD_SR_REFILL_OVERFLOW
from ._lib import KAD_SR_INSERT_OK, KAD_SR_INSERT_OVERFLOW
from ._lib import KAD_SR_MARK_MAX_NODES
from ._lib import (KAD_SR_PLAN_DEFERRED, KAD_SR_PLAN_READY, KAD_SR_PLAN_SKIPPED, KAD_SR_TICK_APPLIED, KAD_SR_TICK_LEFT,
                   KAD_SR_TICK_SKIPPED)
from ._lib import KAD_SWEEP_INCOMING
from ._lib import (KAD_MAINT_BIT_SHIFT, KAD_MAINT_CLASS_SHIFT, KAD_MAINT_EMPTY, KAD_MAINT_HAS_NEXT, KAD_MAINT_HAS_PREV,
                   KAD_MAINT_MAYBE, KAD_MAINT_NEVER, KAD_MAINT_NEXT_EMPTY, KAD_MAINT_PREV_EMPTY, KAD_MAINT_STALE,
                   KAD_MAINT_STALE_NS, KAD_MAINT_SURE)
from ._lib import (KAD_SN_CANDIDATE, KAD_SN_NOGET, KAD_SN_PENDING, KAD_SN_SYNCED, KAD_STEP_APPLY, KAD_STEP_DONE,
                   KAD_STEP_DONE_IF_SYNCED, KAD_STEP_EXHAUSTED, KAD_STEP_EXPIRE, KAD_STEP_NO_EXPIRE, KAD_STEP_NO_SEND,
                   KAD_STEP_SHORT, KAD_STEP_SKIPPED, KAD_STEP_SYNCED)
from ._lib import KAD_SN_ANNOUNCE_DUE, KAD_SN_LISTEN_DUE, KAD_STEP_ANNOUNCE, KAD_STEP_LISTEN, KAD_STEP_PROBE_BLOCKS
from .ingest import ingest
from .searches import (DeviceSearches, expire_searches, mark_search_nodes, plan_insert_round, plan_round, refill_searches,
                       search_step, search_step_batch, search_step_full, search_step_full_batch, start_searches,
                       step_searches, step_searches_full, try_search_insert, try_search_insert_device,
                       try_search_insert_tick)
from .table import DeviceTable, maint_scan_host, nc_closest_dual, rt_closest_dual, rt_responsible_dual

__all__ = [
    "DeviceTable", "InfoHash", "KadError", "KAD_MAX_COUNT", "KAD_NO_NODE", "KAD_SEARCH_NODES",
    "KAD_STATUS_EXPIRED", "KAD_STATUS_GOOD", "KAD_TARGET_NODES", "lib", "nc_closest_dual", "rt_closest_dual", "zeroes",
    "KAD_RESP_FAR", "KAD_RESP_FAR4", "KAD_RESP_FAR6", "rt_responsible_dual",
    "KAD_NN_BOOTSTRAP", "KAD_NN_FULL", "KAD_NN_INSERT", "KAD_NN_KIND_MASK", "KAD_NN_KNOWN", "KAD_NN_MYBUCKET",
    "KAD_NN_NONE", "KAD_NN_REPLACE", "KAD_NN_SPLIT", "ingest",
    "KAD_SN_BAD", "KAD_SR_EXPIRED", "KAD_SR_STOP_END", "KAD_SR_STOP_FAR", "KAD_SR_STOP_FAR_EXPIRED",
    "KAD_SR_STOP_KNOWN", "DeviceSearches", "try_search_insert", "KAD_SWEEP_INCOMING",
    "KAD_SN_REMOVABLE", "KAD_SR_REFILL_OK", "KAD_SR_REFILL_OVERFLOW", "refill_searches",
    "start_searches", "expire_searches",
    "KAD_SR_INSERT_OK", "KAD_SR_INSERT_OVERFLOW", "plan_insert_round", "try_search_insert_device",
    "KAD_SR_MARK_MAX_NODES", "mark_search_nodes",
    "KAD_SR_PLAN_DEFERRED", "KAD_SR_PLAN_READY", "KAD_SR_PLAN_SKIPPED", "KAD_SR_TICK_APPLIED", "KAD_SR_TICK_LEFT",
    "KAD_SR_TICK_SKIPPED", "plan_round", "try_search_insert_tick",
    "KAD_SN_CANDIDATE", "KAD_SN_NOGET", "KAD_SN_PENDING", "KAD_SN_SYNCED", "KAD_STEP_APPLY", "KAD_STEP_DONE",
    "KAD_STEP_DONE_IF_SYNCED", "KAD_STEP_EXHAUSTED", "KAD_STEP_EXPIRE", "KAD_STEP_NO_EXPIRE", "KAD_STEP_NO_SEND",
    "KAD_STEP_SHORT", "KAD_STEP_SKIPPED", "KAD_STEP_SYNCED", "search_step", "search_step_batch", "step_searches",
    "KAD_SN_ANNOUNCE_DUE", "KAD_SN_LISTEN_DUE", "KAD_STEP_ANNOUNCE", "KAD_STEP_LISTEN", "KAD_STEP_PROBE_BLOCKS",
    "search_step_full", "search_step_full_batch", "step_searches_full",
    "KAD_MAINT_BIT_SHIFT", "KAD_MAINT_CLASS_SHIFT", "KAD_MAINT_EMPTY", "KAD_MAINT_HAS_NEXT", "KAD_MAINT_HAS_PREV",
    "KAD_MAINT_MAYBE", "KAD_MAINT_NEVER", "KAD_MAINT_NEXT_EMPTY", "KAD_MAINT_PREV_EMPTY", "KAD_MAINT_STALE",
    "KAD_MAINT_STALE_NS", "KAD_MAINT_SURE", "maint_scan_host",
]
