"""ctypes binding of libkadgpu.so (the C ABI in include/kadgpu.h).

The library is built in-tree by ``__graft_entry__.build()`` (opendht_amd/csrc/Makefile).
There is no fallback: if the HIP library is missing, importing the query API raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkadgpu.so")

KAD_HASH_LEN = 20
KAD_TARGET_NODES = 8
KAD_SEARCH_NODES = 14
KAD_MAX_COUNT = 32
KAD_NO_NODE = 0xFFFFFFFF
KAD_STATUS_GOOD = 0x01
KAD_STATUS_EXPIRED = 0x02
KAD_TABLE_SORTED = 0x01
KAD_TABLE_EAGER = 0x02
KAD_TABLE_NO_SLOT_LINES = 0x04
KAD_LINES_RT16, KAD_LINES_RT32, KAD_LINES_NC16, KAD_LINES_NC32, KAD_LINES_ALL = 0x01, 0x02, 0x04, 0x08, 0x0F
# kad_table_export_lines sets
(KAD_LINESET_WL, KAD_LINESET_WS, KAD_LINESET_WL16, KAD_LINESET_WL32, KAD_LINESET_GL, KAD_LINESET_GL16, KAD_LINESET_GL32,
 KAD_LINESET_SL, KAD_LINESET_SL16, KAD_LINESET_NCL, KAD_LINESET_NCL32, KAD_LINESET_GCNT, KAD_LINESET_DIR) = range(13)
KAD_INFO_WINDOW_LINES = 0x100
KAD_INFO_GENERAL_LINES = 0x200
KAD_INFO_GENERAL_LINES32 = 0x400
KAD_INFO_GENERAL_LINES16 = 0x4000
KAD_INFO_SLOT_LINES16 = 0x8000
KAD_INFO_SHORT_LINES = 0x800
KAD_INFO_NODECACHE_LINES32 = 0x1000
KAD_INFO_SLOT_LINES = 0x2000
KAD_SERVE_MAX_Q, KAD_SERVE_MAX_COUNT, KAD_SERVE_MAX_IDLE_US = 64, 64, 1000000
KAD_OP_REMOVE, KAD_OP_REPLACE, KAD_OP_INSERT, KAD_OP_SPLIT = 1, 2, 3, 4
KAD_RESP_FAR, KAD_RESP_FAR4, KAD_RESP_FAR6 = 1, 1, 2
KAD_NN_NONE, KAD_NN_KNOWN, KAD_NN_REPLACE, KAD_NN_INSERT, KAD_NN_SPLIT, KAD_NN_FULL = 0, 1, 2, 3, 4, 5
KAD_NN_KIND_MASK, KAD_NN_MYBUCKET, KAD_NN_BOOTSTRAP = 0x0F, 0x10, 1
KAD_SR_EXPIRED, KAD_SN_BAD = 0x01, 0x01
KAD_SN_REMOVABLE = 0x02
KAD_SR_REFILL_OK, KAD_SR_REFILL_OVERFLOW = 0, 1
KAD_SR_INSERT_OK, KAD_SR_INSERT_OVERFLOW = 0, 1
KAD_SR_MARK_MAX_NODES = 1 << 20
KAD_SR_PLAN_SKIPPED, KAD_SR_PLAN_READY, KAD_SR_PLAN_DEFERRED = 0, 1, 2
KAD_SR_TICK_LEFT, KAD_SR_TICK_SKIPPED, KAD_SR_TICK_APPLIED = 0, 1, 2
KAD_SR_STOP_END, KAD_SR_STOP_KNOWN, KAD_SR_STOP_FAR, KAD_SR_STOP_FAR_EXPIRED = 0, 1, 2, 3
KAD_SN_CANDIDATE, KAD_SN_PENDING, KAD_SN_SYNCED, KAD_SN_NOGET = 0x04, 0x08, 0x10, 0x20
KAD_STEP_APPLY, KAD_STEP_NO_SEND, KAD_STEP_DONE_IF_SYNCED, KAD_STEP_NO_EXPIRE = 0x01, 0x02, 0x04, 0x08
KAD_STEP_SKIPPED, KAD_STEP_SHORT, KAD_STEP_SYNCED, KAD_STEP_DONE, KAD_STEP_EXHAUSTED, KAD_STEP_EXPIRE = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20)
KAD_SN_LISTEN_DUE, KAD_SN_ANNOUNCE_DUE = 0x40, 0x80
KAD_STEP_LISTEN, KAD_STEP_ANNOUNCE, KAD_STEP_PROBE_BLOCKS = 0x10, 0x20, 0x40
KAD_SWEEP_INCOMING = 1
(KAD_MAINT_STALE, KAD_MAINT_EMPTY, KAD_MAINT_HAS_NEXT, KAD_MAINT_NEXT_EMPTY, KAD_MAINT_HAS_PREV,
 KAD_MAINT_PREV_EMPTY) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
KAD_MAINT_CLASS_SHIFT, KAD_MAINT_NEVER, KAD_MAINT_MAYBE, KAD_MAINT_SURE, KAD_MAINT_BIT_SHIFT = 6, 0, 1, 2, 8
KAD_MAINT_STALE_NS = 600_000_000_000
INT64_MIN = -(1 << 63)


def row_words(count: int) -> int:
    """KAD_ROW_WORDS: uint32 words of one complete row of kad_rt_shard_batch."""
    return 4 + ((count + 3) & ~3)


def part_words(count: int) -> int:
    """KAD_PART_WORDS: a row plus the entries' 160-bit XOR distances (5 words each)."""
    return row_words(count) + 5 * count


KAD_SHARD_REGIONS = 8
KAD_SHARD_COUNTERS = 10
KAD_SHARD_COUNTER_STRIDE = 32
KAD_SHARD_MAX_WORLD = 16
KAD_ROUTE_CSTRIDE = 32
KAD_ROUTE_MAX_WORLD = 16
KAD_ROUTE_PACKED_MAX_COUNT = 32
KAD_ROUTE_SUBS = 8
KAD_ROUTE_QPW = 1024


def route_ctr_words(world: int) -> int:
    """KAD_ROUTE_CTR_WORDS(world)"""
    return (world * KAD_ROUTE_SUBS + 1) * KAD_ROUTE_CSTRIDE


def route_overflow_word(world: int) -> int:
    """KAD_ROUTE_OVERFLOW_WORD(world)"""
    return world * KAD_ROUTE_SUBS * KAD_ROUTE_CSTRIDE


def route_packed_words(count: int) -> int:
    """KAD_ROUTE_PACKED_WORDS(count)"""
    return 1 + (count + 3) // 4


def shard_block_words(count: int, row_cap: int, part_cap: int) -> int:
    """KAD_SHARD_BLOCK_WORDS: one rank's send block (regions of rows, parts, counters)."""
    return (KAD_SHARD_REGIONS * row_cap * row_words(count) + part_cap * part_words(count)
            + KAD_SHARD_COUNTERS * KAD_SHARD_COUNTER_STRIDE)


KAD_ERR_INVALID = -1
KAD_ERR_NOMEM = -3
KAD_ERR_UNSUPPORTED = -4
KAD_ERR_NOT_SORTED = -5

ERRORS = {
    -1: "KAD_ERR_INVALID",
    -2: "KAD_ERR_HIP",
    -3: "KAD_ERR_NOMEM",
    -4: "KAD_ERR_UNSUPPORTED",
    -5: "KAD_ERR_NOT_SORTED",
    -6: "KAD_ERR_NO_DEVICE",
}

# Every symbol include/kadgpu.h declares, with its ctypes signature.
_P = C.c_void_p
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_i64p = C.POINTER(C.c_int64)
SIGNATURES = {
    "kad_last_error": (C.c_char_p, []),
    "kad_version": (C.c_int, []),
    "kad_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "kad_table_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint32, _P, _P, C.c_uint32, _P, _P,
                                   C.c_uint32, C.c_uint32]),
    "kad_table_destroy": (C.c_int, [_P]),
    "kad_table_get_info": (C.c_int, [_P, _P]),
    "kad_table_prepare": (C.c_int, [_P, C.c_uint32]),
    "kad_table_line_sets": (C.c_int, [_P, _P, _P, _P]),
    "kad_table_update_status": (C.c_int, [_P, _P]),
    "kad_table_apply": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P]),
    "kad_table_export": (C.c_int, [_P, _P, _P, _P, _P]),
    "kad_table_export_lines": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "kad_table_sweep": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    "kad_table_sweep_host": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint32]),
    "kad_table_set_bucket_times": (C.c_int, [_P, _P]),
    "kad_table_patch_bucket_times": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "kad_table_get_bucket_times": (C.c_int, [_P, _P]),
    "kad_table_touch_buckets": (C.c_int, [_P, _P, C.c_uint32, C.c_int64, _P, _P]),
    "kad_table_touch_buckets_host": (C.c_int, [_P, _P, C.c_uint32, C.c_int64, _P]),
    "kad_table_maintenance": (C.c_int, [_P, C.c_int64, C.c_uint32, _P, _P, C.c_uint32, _P]),
    "kad_table_maintenance_host": (C.c_int, [_P, C.c_int64, C.c_uint32, _P, _P, C.c_uint32]),
    "kad_maint_scan_host": (C.c_int, [C.c_uint32, _P, _P, _P, C.c_int64, C.c_uint32, _P, _P, C.c_uint32]),
    "kad_table_expire": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, _P]),
    "kad_nc_apply": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P]),
    "kad_table_set_times": (C.c_int, [_P, _P, _P, _P]),
    "kad_table_refresh_status": (C.c_int, [_P, C.c_int64, _P]),
    "kad_table_refresh_diag": (C.c_int, [_P, _P]),
    "kad_table_patch_status": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "kad_table_patch_times": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P]),
    "kad_rt_closest_batch": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_rt_closest_batch_host": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "kad_table_serve": (C.c_int, [_P, C.c_uint32]),
    "kad_table_serve_stats": (C.c_int, [_P, _P]),
    "kad_rt_find_bucket_batch": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "kad_nc_closest_batch": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_nc_closest_batch_host": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "kad_rt_closest_batch_dual": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_nc_closest_batch_dual": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_rt_responsible_batch": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "kad_rt_responsible_batch_dual": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "kad_rt_responsible_batch_host": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    "kad_rt_triage_batch": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P]),
    "kad_rt_triage_batch_host": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_search_trim": (C.c_int, [C.c_uint32, _P, C.c_uint32, _P, _P]),
    "kad_searches_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_searches_patch": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_searches_apply": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, _P, _P]),
    "kad_searches_info": (C.c_int, [_P, _P, _P, _P]),
    "kad_searches_export": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "kad_searches_destroy": (C.c_int, [_P]),
    "kad_sr_try_insert_batch": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_sr_try_insert_batch_host": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P]),
    "kad_sr_refill": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_sr_refill_kernel_ms": (C.c_int, [_P, _P]),
    "kad_sr_insert": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "kad_sr_insert_kernel_ms": (C.c_int, [_P, _P]),
    "kad_sr_plan_round": (C.c_int, [C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kad_sr_try_insert_tick": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kad_sr_mark_nodes": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "kad_sr_mark_kernel_ms": (C.c_int, [_P, _P, _P]),
    "kad_sr_mark_entries": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_search_step": (C.c_int, [C.c_uint32, _P, C.c_uint32, C.c_uint32, _P]),
    "kad_search_step_batch": (C.c_int, [C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_sr_step": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P]),
    "kad_sr_mark_due": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_search_step_full": (C.c_int, [C.c_uint32, _P, C.c_uint32, C.c_uint32, _P]),
    "kad_search_step_full_batch": (C.c_int, [C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_sr_step_full": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P]),
    "kad_rt_shard_batch": (C.c_int, [_P, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32,
                                     _P, _P]),
    "kad_rt_scatter_rows": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.c_int,
                                      _P]),
    "kad_rt_merge_parts": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, C.c_int, _P]),
    "kad_rt_gather_finish": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P,
                                       _P, C.c_int, _P]),
    "kad_home_range": (None, [C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "kad_rt_shard_batch_home": (C.c_int, [_P, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P]),
    "kad_rt_home_finish": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P,
                                     _P, _P, _P, C.c_int, _P]),
    "kad_rt_shard_step_home": (C.c_int, [_P, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P]),
    "kad_rt_home_finish_reset": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, _P, _P, _P, _P, C.c_int, _P]),
    "kad_route_pack": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_int, _P]),
    "kad_route_unpack": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_int, _P]),
    "kad_route_compress": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_int, _P]),
    "kad_rt_closest_batch_packed": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_route_unpack_packed": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_int, _P]),
    "kad_route_fold_flags": (C.c_int, [_P, C.c_uint32, _P, C.c_int, _P]),
    "kad_route_pack_keys": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_int, _P]),
    "kad_rt_closest_keys_packed": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P]),
    "kad_route_pack_ex": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint32, C.c_int,
                                    _P]),
    "kad_route_unpack_packed_fold": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, C.c_int,
                                               _P]),
    "kad_comm_unique_id": (C.c_int, [_P]),
    "kad_comm_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint32, C.c_uint32, _P]),
    "kad_comm_destroy": (C.c_int, [_P]),
    "kad_comm_info": (C.c_int, [_P, _P, _P, _P]),
    "kad_comm_all_to_all": (C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    "kad_route_run": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P]),
    "kad_shard_run": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P,
                                _P, _P, _P, _P]),
    "kad_table_set_addrs": (C.c_int, [_P, C.c_uint32, _P]),
    "kad_buffer_nodes_batch": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, _P]),
    "kad_parse_nodes_batch": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, C.c_int, _P]),
    "kad_swarm_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint32, _P]),
    "kad_swarm_destroy": (C.c_int, [_P]),
    "kad_swarm_info": (C.c_int, [_P, _P, _P]),
    "kad_swarm_get_table": (C.c_int, [_P, C.c_uint32, _P, _P, _P]),
    "kad_swarm_closest_batch": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    "kad_search_create": (C.c_int, [C.POINTER(_P), _P, C.c_uint32, _P, _P, C.c_uint32, _P]),
    "kad_search_hop": (C.c_int, [_P, _P]),
    "kad_search_get": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "kad_search_destroy": (C.c_int, [_P]),
    "kad_xor_cmp_batch": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P]),
    "kad_common_bits_batch": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "kad_lowbit_batch": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "kad_infohash_get_batch": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_int, _P]),
    "kad_synth_ids": (C.c_int, [C.c_uint64, C.c_uint32, _P]),
    "kad_synth_status": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    "kad_sort_ids": (C.c_int, [C.c_uint32, _P, _P]),
    "kad_uniform_buckets": (C.c_int, [C.c_uint32, _P, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P]),
    "kad_split_table": (C.c_int, [C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P]),
    "kad_synth_uniform_shard": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_double,
                                          C.c_uint32, C.c_uint32, _P, _P, _P, _P]),
    "kad_synth_recipe_range": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.c_uint64, _P, _P, _P, _P, _P]),
}


class KadError(RuntimeError):
    def __init__(self, code: int, where: str, msg: str):
        super().__init__(f"{where}: {ERRORS.get(code, code)}: {msg}")
        self.code = code


class table_info(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32), ("n_buckets", C.c_uint32), ("index_base", C.c_uint32),
        ("flags", C.c_uint32), ("device", C.c_int32), ("rt_radix_bits", C.c_uint32),
        ("nc_radix_bits", C.c_uint32), ("n_good", C.c_uint32), ("device_bytes", C.c_uint64),
    ]


KAD_COMM_ID_BYTES = 128
KAD_ROUTE_PACKED, KAD_ROUTE_KEYS, KAD_ROUTE_ZEROED = 1, 2, 4


class route_set(C.Structure):
    """kad_route_set: one buffer set of kad_route_run (device pointers)."""
    _fields_ = [(n, C.c_void_p) for n in ("send", "recv", "slot", "ctr", "rows", "cnt", "back_rows", "back_cnt", "prow",
                                          "back_prow")]


class serve_stats(C.Structure):
    _fields_ = [
        ("idle_us", C.c_uint32), ("last_polls", C.c_uint32), ("launches", C.c_uint64), ("requests", C.c_uint64),
        ("last_busy_ns", C.c_uint64),
    ]


class sweep_totals(C.Structure):
    """kad_sweep_totals"""
    _fields_ = [(n, C.c_uint32) for n in ("good", "dubious", "expired", "incoming", "changed_buckets", "empty_buckets",
                                          "flags", "reserved")]


class maint_totals(C.Structure):
    """kad_maint_totals"""
    _fields_ = [(n, C.c_uint32) for n in ("candidates", "stale", "empty", "sure", "maybe", "never", "first_sure",
                                          "reserved")]


MAINT_REC_DTYPE = [("bucket", "<u4"), ("kind", "<u4")]  # kad_maint_rec as a numpy record


class sr_tick_stats(C.Structure):
    """kad_sr_tick_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("rounds", "skipped", "applied", "left", "pairs", "overflowed")] + [
        ("verdict_ms", C.c_float), ("insert_ms", C.c_float)]


class step_out(C.Structure):
    """kad_step_out"""
    _fields_ = [("picks", C.c_uint64), ("counts", C.c_uint32), ("bits", C.c_uint32)]


STEP_OUT_DTYPE = [("picks", "<u8"), ("counts", "<u4"), ("bits", "<u4")]  # kad_step_out as a numpy record


class sr_step_stats(C.Structure):
    """kad_sr_step_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("synced", "expired", "skipped", "picks")] + [("kernel_ms", C.c_float)]


class step_full_out(C.Structure):
    """kad_step_full_out"""
    _fields_ = [("picks", C.c_uint64), ("listen", C.c_uint64), ("announce", C.c_uint64), ("counts", C.c_uint32),
                ("bits", C.c_uint32)]


# kad_step_full_out as a numpy record
STEP_FULL_OUT_DTYPE = [("picks", "<u8"), ("listen", "<u8"), ("announce", "<u8"), ("counts", "<u4"), ("bits", "<u4")]


class sr_step_full_stats(C.Structure):
    """kad_sr_step_full_stats"""
    _fields_ = [(n, C.c_uint32) for n in ("synced", "expired", "skipped", "picks", "listens", "announces")] + [
        ("kernel_ms", C.c_float)]


class refresh_diag(C.Structure):
    _fields_ = [("spin_timeouts", C.c_uint32), ("last_block_lines", C.c_uint32), ("guard_errors", C.c_uint32)]


_lib = None


def use_ablation_build() -> None:
    """Tools only (tools/bench_paths.py, tools/ab_bench.py): load libkadgpu_abl.so, the build with the
    timing-ablation kernels (make -C opendht_amd/csrc ablations), instead of the product library.
    Must run before the first lib() call."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("libkadgpu.so is already loaded")
    LIB_PATH = os.path.join(_HERE, "libkadgpu_abl.so")


def use_library(path: str) -> None:
    """Tools only (tools/nc32_ab.py): load a variant build of the engine (an A/B against the product library).
    Must run before the first lib() call."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("libkadgpu.so is already loaded")
    LIB_PATH = os.path.abspath(path)


def lib() -> C.CDLL:
    """Load libkadgpu.so, raising loudly (no fallback) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP engine first (python -c "
                f"'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, where: str) -> None:
    if rc != 0:
        raise KadError(rc, where, lib().kad_last_error().decode(errors="replace"))


def ptr(a) -> C.c_void_p | None:
    """Raw pointer of a numpy array or a torch tensor (host or device); None for None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)
