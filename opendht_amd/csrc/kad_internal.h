// Shared by the translation units of libkadgpu.so, not installed: what kad_engine.hip exports to the others in
// namespace kadgpu_internal. struct kad_table stays private to the engine; other units see a table only through
// table_ids().
#pragma once

#include <cstdint>

struct kad_table;

namespace kadgpu_internal {

// Sets the thread-local error of kad_last_error() and returns code.
int set_error(int code, const char* msg);
// The device is a gfx950.
bool device_ok(int dev);

// The device view of a table's node IDs: key[i] = the top 64 ID bits as one native u64, tail[3 i ..] = the remaining
// three words as numbers; n nodes, indices reported as index + index_base; the table's device and KAD_TABLE_SORTED.
struct TableIds {
    const uint64_t* key;
    const uint32_t* tail;
    uint32_t n, index_base;
    int device;
    bool sorted;
};
TableIds table_ids(const kad_table* t);

}  // namespace kadgpu_internal
