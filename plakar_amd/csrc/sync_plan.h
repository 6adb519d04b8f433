// Host-only planning of cdc_sync_run, shared by the library (cdc_sync.cpp) and
// the stand-alone sanitizer program tests/c/sync_plan_check.cpp:
//
//   * the row filter of synchronize (cmd/plakar/subcommands/sync/sync.go:
//     182-266): every index row of the registered packfiles, in registration
//     and index order, of every blob type, is taken unless its (type, checksum)
//     is in `known` (the destination's BlobExists), was already taken in this
//     run, or, when `wanted` is given, is not in it.  known and wanted are
//     33-byte records (type, checksum) sorted ascending by memcmp, searched by
//     bisection; the run's taken-set is a hash set;
//   * the batch cut: rows up to `budget` stored bytes; a batch closes before
//     the row that would take it past the budget, a batch always takes its
//     first row (a row larger than the budget goes alone) and a row of 0
//     stored bytes is a row like any other;
//   * the split of a batch's surviving blobs among the packers: contiguous
//     ranges in source order, of about equal bytes.
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <unordered_set>
#include <vector>

#include "plakar_cdc.h"

namespace splan {

constexpr size_t kKeyBytes = 33;              // u8 type, 32-B checksum
constexpr uint64_t kMaxRows = 0x7FFFFFFFull;  // a batch's blobs are numbered in 32 bits

struct Key {
    uint8_t b[kKeyBytes];
    bool operator==(const Key &o) const { return memcmp(b, o.b, kKeyBytes) == 0; }
};
struct KeyHash {  // the checksums are SHA-256: any eight bytes of one are a hash
    size_t operator()(const Key &k) const
    {
        uint64_t v;
        memcpy(&v, k.b + 1, 8);
        return size_t(v * 31 + k.b[0]);
    }
};

static inline Key key_of(const cdc_packfile_row &r)
{
    Key k;
    k.b[0] = r.type;
    memcpy(k.b + 1, r.checksum, 32);
    return k;
}

// n records in non-descending memcmp order (an empty list is sorted).
static inline bool sorted33(const uint8_t *recs, uint64_t n)
{
    for (uint64_t i = 1; i < n; ++i)
        if (memcmp(recs + kKeyBytes * (i - 1), recs + kKeyBytes * i, kKeyBytes) > 0) return false;
    return true;
}

// Whether `key` is one of the n sorted records.
static inline bool contains33(const uint8_t *recs, uint64_t n, const uint8_t *key)
{
    uint64_t lo = 0, hi = n;  // the first record >= key lies in [lo, hi]
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (memcmp(recs + kKeyBytes * mid, key, kKeyBytes) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && memcmp(recs + kKeyBytes * lo, key, kKeyBytes) == 0;
}

struct Pack {  // one registered packfile's index
    const cdc_packfile_row *rows;
    uint64_t n;
};
struct Item {  // a row the run takes
    uint32_t pack, row;
};
struct Batch {  // items [first, first + count)
    uint64_t first, count, bytes;
};
struct Plan {
    std::vector<Item> items;
    std::vector<Batch> batches;
    uint64_t skipped = 0;  // rows in `known` or already taken (a row outside `wanted` is not counted)
    uint64_t bytes = 0;
};

// wanted == NULL: every row is wanted (nwanted is not read).
static inline void plan(const Pack *packs, size_t npacks, const uint8_t *known, uint64_t nknown, const uint8_t *wanted,
                        uint64_t nwanted, uint64_t budget, Plan &out)
{
    out = Plan();
    if (budget == 0) budget = 1;
    std::unordered_set<Key, KeyHash> seen;
    Batch cur{0, 0, 0};
    for (size_t p = 0; p < npacks; ++p)
        for (uint64_t r = 0; r < packs[p].n; ++r) {
            const cdc_packfile_row &R = packs[p].rows[r];
            const Key k = key_of(R);
            if (wanted && !contains33(wanted, nwanted, k.b)) continue;
            if (contains33(known, nknown, k.b) || !seen.insert(k).second) {
                ++out.skipped;
                continue;
            }
            if (cur.count && (cur.bytes + R.length > budget || cur.count >= kMaxRows)) {
                out.batches.push_back(cur);
                cur = Batch{out.items.size(), 0, 0};
            }
            out.items.push_back(Item{uint32_t(p), uint32_t(r)});
            ++cur.count;
            cur.bytes += R.length;
            out.bytes += R.length;
        }
    if (cur.count) out.batches.push_back(cur);
}

// A batch's n blobs lie at off[i] .. off[i + 1] of its output (n + 1 ascending
// offsets; a failed blob has no bytes).  bounds[0 .. parts] ascends from 0 to
// n: packer p takes blobs [bounds[p], bounds[p + 1]), in source order, and
// range p starts at the first blob at or past p / parts of the bytes.
static inline void split(const uint64_t *off, uint32_t n, uint32_t parts, std::vector<uint32_t> &bounds)
{
    if (parts == 0) parts = 1;
    bounds.assign(size_t(parts) + 1, n);
    bounds[0] = 0;
    const uint64_t base = off[0], total = off[n] - off[0];
    uint32_t i = 0;
    for (uint32_t p = 1; p < parts; ++p) {
        // total * p / parts without a 128-bit product
        const uint64_t want = total / parts * p + total % parts * p / parts;
        while (i < n && off[i] - base < want) ++i;
        bounds[p] = i;
    }
}

}  // namespace splan
