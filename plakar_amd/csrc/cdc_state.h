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

// ---- maintenance ----

constexpr uint32_t kRefBytes = 33;   // a reference of cdc_state_mark: the type byte, then the checksum
constexpr uint32_t kSweepTile = 256; // records per tile of the stable compaction: one trip of one workgroup

// The packfile table and what a sweep accumulates beside it, all indexed by
// the table's slot; P.recs is the record store, the key a record's packfile.
struct Packs {
    Table P;
    uint64_t *extent, *live_bytes, *live_rows;
    int32_t *verdict;
};
// Counters of a sweep, in device memory (zeroed by the host before the stage that adds to them).
struct SweepCounts {
    uint64_t packs;                // k_state_packs: slots claimed
    uint64_t seen, live, losers;   // k_state_sweep
    uint64_t listed;               // k_state_verdict: entries of the packfile list written
    uint64_t kept, repack;         // k_sweep_scan: the totals of the two classes
};

// n references (stride 33 with the type in byte 0 when type == kTypeOfRecord,
// else stride 32, all of `type`) -> bits of `marks`, found[i] when found is not null
constexpr uint32_t kTypeOfRecord = 0xFFFFFFFFu;
int launch_mark(int device, const Table &T, uint32_t type, const uint8_t *d_refs, uint64_t n, uint32_t *d_marks,
                uint8_t *d_found, void *stream);
// *d_missing (zeroed here) = the zeros among found[0, n)
int launch_missing(int device, const uint8_t *d_found, uint64_t n, uint64_t *d_missing, void *stream);
// the four stages of a sweep over records [0, nrecs); see cdc_state.hip
int launch_packs(int device, const Table &P, uint64_t nrecs, SweepCounts *d_counts, void *stream);
int launch_sweep(int device, const Table &T, const Packs &K, uint64_t nrecs, const uint32_t *d_marks, uint32_t keep_types,
                 uint64_t *d_live, uint64_t *d_slot, SweepCounts *d_counts, void *stream);
int launch_verdict(int device, const Packs &K, uint32_t permille, cdc_sweep_pack *d_list, uint64_t cap,
                   SweepCounts *d_counts, void *stream);
// d_class: one byte per record; d_tiles: 2 * (ntiles + 1) u64, counts then exclusive sums, kept at [2t], repack at [2t + 1]
int launch_classes(int device, const Packs &K, uint64_t nrecs, const uint64_t *d_live, const uint64_t *d_slot,
                   uint8_t *d_class, uint64_t *d_tiles, SweepCounts *d_counts, void *stream);
int launch_compact(int device, const cdc_state_row *d_recs, uint64_t nrecs, const uint8_t *d_class, const uint64_t *d_tiles,
                   cdc_state_row *d_kept, uint64_t kept_cap, cdc_state_row *d_repack, uint64_t repack_cap, void *stream);

}  // namespace cst
