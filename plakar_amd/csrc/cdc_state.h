// What cdc_state.cpp (the aggregate, its C ABI) and cdc_state.hip (the
// kernels and their launches) share.  DESIGN.md 5.24.  Internal.
#pragma once

#include <stdint.h>

#include "plakar_cdc.h"
#include "state_plan.h"

namespace cst {

constexpr uint64_t kEmpty = ~0ull;         // a free slot of the table
constexpr uint32_t kNoPos = 0xFFFFFFFFu;   // an id with no IdToChecksum record (yet)
constexpr uint32_t kTypeDeleted = splan::kTypes;  // a DeletedSnapshots record's key type in the table
constexpr uint64_t kMinSlots = 1024;

// One state of a merge call, in device memory.  The host fills the first three
// fields, k_state_plan the layout and its status, the host id_base after it.
struct StateDesc {
    uint64_t plain;    // offset of its plaintext
    uint64_t len;
    uint64_t id_base;  // its first entry in the id table
    splan::Layout L;
    int32_t status;
    uint32_t bad;      // set by a kernel that met an id it cannot resolve
};

// A run of records of one section of one state; `first` is the exclusive sum
// of the counts before it, so a grid-stride item finds its run by bisection.
struct Seg {
    uint64_t first, count;
    uint64_t src;      // offset of the section's first record in the plaintext
    uint64_t out;      // k_state_index: unused; k_state_resolve: the first record's number
    uint32_t state;    // index in the StateDesc array
    uint32_t type;     // 0..8, or kTypeDeleted
};

struct Table {
    uint64_t *slots;   // record numbers; kEmpty when free
    uint64_t mask;     // capacity - 1 (a power of two)
    const cdc_state_row *recs;
};

// Launches, all asynchronous on `stream`; CDC_OK or CDC_E_DEVICE.
int launch_plan(int device, StateDesc *d_desc, uint32_t n, const uint8_t *d_plain, void *stream);
int launch_index(int device, StateDesc *d_desc, const Seg *d_segs, uint32_t nsegs, uint64_t items, const uint8_t *d_plain,
                 uint32_t *d_idtab, void *stream);
int launch_resolve(int device, StateDesc *d_desc, const Seg *d_segs, uint32_t nsegs, uint64_t items,
                   const uint8_t *d_plain, const uint32_t *d_idtab, cdc_state_row *d_recs, void *stream);
int launch_insert(int device, const Table &T, uint64_t lo, uint64_t hi, void *stream);
// d_counts: kTypes + 1 u64, zeroed here
int launch_count(int device, const Table &T, uint64_t *d_counts, void *stream);
int launch_lookup(int device, const Table &T, uint32_t type, const uint8_t *d_sums, uint64_t n, cdc_state_row *d_out,
                  void *stream);
// d_n: one u64, zeroed here; rows past cap are counted and not written
int launch_rows(int device, const Table &T, uint32_t type, cdc_state_row *d_out, uint64_t cap, uint64_t *d_n, void *stream);

}  // namespace cst
