// Host-only layout code of a repository state, shared by the library
// (cdc_state.cpp, cdc_state.hip) and the stand-alone sanitizer program
// tests/c/state_plan_check.cpp.
//
// A state is what (*State).SerializeStream writes (repository/state/state.go:
// 132-233), everything little endian:
//
//   u32 version | u64 timestamp (ns) | u8 aggregate | u64 n, n x 32 B extends
//   u64 n, n x 16 B   DeletedSnapshots   id u64, time u64 (ns)
//   u64 n, n x 40 B   IdToChecksum       id u64, checksum 32 B
//   u64 n, n x 24 B   Chunks, Objects, Files, Directories, Children, Datas,
//                     Snapshots, Signatures, Errors:
//                     id u64, packfile id u64, offset u32, length u32
//
// The reader (read) turns `len` bytes into the metadata and the eleven
// sections' ranges; it holds every count against the bytes that remain before
// it multiplies or uses it, so no count can wrap and nothing is sized from one.
// Bytes after the last section are ignored and the version is reported, not
// judged, as DeserializeStream does (state.go:235-348).  The writer (Writer,
// serialize, serialize_deleted) is SerializeStream for a list of rows and of
// deleted snapshots.
//
// No HIP, no library state: everything is a function of its arguments.  The
// reader's functions carry SPLAN_FN, so that cdc_state.hip can compile the same
// checked code for the device (one lane per state reads the twelve counts).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "plakar_cdc.h"

#ifndef SPLAN_FN
#define SPLAN_FN static inline
#endif

namespace splan {

constexpr uint32_t kTypes = 9;                // packfile.TYPE_SNAPSHOT .. TYPE_ERROR (packfile/packfile.go:17-25)
constexpr uint32_t kSections = 2 + kTypes;    // DeletedSnapshots, IdToChecksum, then one per type
constexpr uint32_t kSecDeleted = 0, kSecIds = 1, kSecFirstType = 2;
constexpr uint64_t kHeadBytes = 4 + 8 + 1;    // version, timestamp, aggregate
constexpr uint64_t kMinBytes = kHeadBytes + 8 + 8 * kSections;  // 109: every count zero
constexpr uint64_t kSumBytes = 32, kDeletedBytes = 16, kIdBytes = 40, kLocBytes = 24;
constexpr uint32_t kVersion = 100;            // state.VERSION

// The section a type's locations are written in: SerializeStream's order
// (Chunks first, Snapshots seventh), not the type numbers'.
SPLAN_FN uint32_t section_of_type(uint32_t type)
{
    return type == 0 ? kSecFirstType + 6 : type <= 6 ? kSecFirstType + type - 1 : kSecFirstType + type;
}
SPLAN_FN uint32_t type_of_section(uint32_t sec)  // sec >= kSecFirstType
{
    const uint32_t k = sec - kSecFirstType;
    return k == 6 ? 0 : k < 6 ? k + 1 : k;
}
SPLAN_FN uint64_t record_bytes(uint32_t sec) { return sec == kSecDeleted ? kDeletedBytes : sec == kSecIds ? kIdBytes : kLocBytes; }

SPLAN_FN uint32_t rd32(const uint8_t *p)
{
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}
SPLAN_FN uint64_t rd64(const uint8_t *p) { return uint64_t(rd32(p)) | uint64_t(rd32(p + 4)) << 32; }

struct Section {
    uint64_t off;    // of the first record
    uint64_t count;
};
struct Layout {
    uint32_t version;
    uint32_t aggregate;
    uint64_t timestamp;
    Section extends;
    Section sec[kSections];
    uint64_t end;    // one past the last section
};

// A u64 count at `*pos` and its records of `rec` bytes: CDC_E_CORRUPT when the
// count itself, or count * rec, does not fit in the bytes that remain.
SPLAN_FN int take(const uint8_t *bytes, uint64_t len, uint64_t *pos, uint64_t rec, Section *s)
{
    if (len - *pos < 8) return CDC_E_CORRUPT;  // *pos <= len always
    const uint64_t count = rd64(bytes + *pos);
    *pos += 8;
    if (count > (len - *pos) / rec) return CDC_E_CORRUPT;
    s->off = *pos;
    s->count = count;
    *pos += count * rec;  // <= len
    return CDC_OK;
}

// CDC_OK and *L, or CDC_E_CORRUPT (then *L is zero).  Reads bytes[0, len) only.
SPLAN_FN int read(const uint8_t *bytes, uint64_t len, Layout *L)
{
    memset(L, 0, sizeof(*L));
    if (len < kHeadBytes) return CDC_E_CORRUPT;
    uint64_t pos = kHeadBytes;
    int st = take(bytes, len, &pos, kSumBytes, &L->extends);
    for (uint32_t s = 0; s < kSections && st == CDC_OK; ++s) st = take(bytes, len, &pos, record_bytes(s), &L->sec[s]);
    if (st != CDC_OK) {
        memset(L, 0, sizeof(*L));
        return st;
    }
    L->version = rd32(bytes);
    L->timestamp = rd64(bytes + 4);
    L->aggregate = bytes[12] == 1;
    L->end = pos;
    return CDC_OK;
}

}  // namespace splan

#ifndef SPLAN_NO_WRITER

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

namespace splan {

struct Sum {
    uint8_t b[32];
    bool operator==(const Sum &o) const { return memcmp(b, o.b, 32) == 0; }
};
struct SumHash {  // the checksums are SHA-256: any eight bytes are a hash
    size_t operator()(const Sum &s) const
    {
        uint64_t v;
        memcpy(&v, s.b, 8);
        return size_t(v);
    }
};

static inline void wr32(uint8_t *p, uint32_t v) { p[0] = uint8_t(v), p[1] = uint8_t(v >> 8), p[2] = uint8_t(v >> 16), p[3] = uint8_t(v >> 24); }
static inline void wr64(uint8_t *p, uint64_t v) { wr32(p, uint32_t(v)), wr32(p + 4, uint32_t(v >> 32)); }

// A state under construction: SetPackfileForBlob (state.go:572-626) for each
// row, then SerializeStream with every section in ascending id.
struct Writer {
    struct Loc {
        uint64_t id, pack;
        uint32_t offset, length;
    };
    std::unordered_map<Sum, uint64_t, SumHash> ids;  // checksumToId
    std::vector<Sum> sums;                           // IdToChecksum
    std::vector<Loc> locs[kTypes];
    std::vector<uint8_t> seen[kTypes];               // by id: the type's map has it
    std::unordered_map<uint64_t, int64_t> deleted;   // DeletedSnapshots: id -> time (ns)

    uint64_t id_of(const uint8_t *sum)  // getOrCreateIdForChecksum (state.go:118-130)
    {
        Sum s;
        memcpy(s.b, sum, 32);
        const auto r = ids.emplace(s, uint64_t(sums.size()));
        if (r.second) sums.push_back(s);
        return r.first->second;
    }
    // CDC_OK, or CDC_E_INVALID for a type the reference panics on
    int set_packfile_for_blob(uint32_t type, const uint8_t *pack, const uint8_t *blob, uint32_t offset, uint32_t length)
    {
        if (type >= kTypes) return CDC_E_INVALID;
        const uint64_t p = id_of(pack), b = id_of(blob);  // the packfile's id first
        std::vector<uint8_t> &S = seen[type];
        if (S.size() <= b) S.resize(sums.size(), 0);
        if (S[b]) return CDC_OK;  // a key already present keeps its location (state.go:618-625)
        S[b] = 1;
        locs[type].push_back(Loc{b, p, offset, length});
        return CDC_OK;
    }
    // DeleteSnapshot (state.go:628-647) as a delta records it: the last time given stays
    void delete_snapshot(const uint8_t *sum, int64_t time_ns) { deleted[id_of(sum)] = time_ns; }
    uint64_t rows() const
    {
        uint64_t n = 0;
        for (const auto &v : locs) n += v.size();
        return n;
    }
    uint64_t size(uint64_t nextends) const
    {
        return kMinBytes + kSumBytes * nextends + kDeletedBytes * deleted.size() + kIdBytes * sums.size() + kLocBytes * rows();
    }
    // `out` holds size(nextends) bytes
    void write(int64_t timestamp_ns, int aggregate, const uint8_t *extends, uint64_t nextends, uint8_t *out)
    {
        uint8_t *p = out;
        wr32(p, kVersion), wr64(p + 4, uint64_t(timestamp_ns)), p[12] = aggregate ? 1 : 0;
        p += kHeadBytes;
        wr64(p, nextends), p += 8;
        if (nextends) memcpy(p, extends, size_t(kSumBytes * nextends));
        p += kSumBytes * nextends;
        std::vector<std::pair<uint64_t, int64_t>> gone(deleted.begin(), deleted.end());
        std::sort(gone.begin(), gone.end());
        wr64(p, gone.size()), p += 8;
        for (const auto &g : gone) wr64(p, g.first), wr64(p + 8, uint64_t(g.second)), p += kDeletedBytes;
        wr64(p, sums.size()), p += 8;
        for (uint64_t i = 0; i < sums.size(); ++i, p += kIdBytes) wr64(p, i), memcpy(p + 8, sums[i].b, 32);
        for (uint32_t s = kSecFirstType; s < kSections; ++s) {
            std::vector<Loc> &v = locs[type_of_section(s)];
            std::sort(v.begin(), v.end(), [](const Loc &a, const Loc &b) { return a.id < b.id; });
            wr64(p, v.size()), p += 8;
            for (const Loc &l : v) {
                wr64(p, l.id), wr64(p + 8, l.pack), wr32(p + 16, l.offset), wr32(p + 20, l.length);
                p += kLocBytes;
            }
        }
    }
};

// cdc_state_serialize_deleted without its NULL checks: the rows, then the
// deleted snapshots (their ids come after the rows').
static inline int serialize_deleted(const cdc_state_row *rows, uint64_t n, const uint8_t *deleted, const int64_t *deleted_ns,
                                    uint64_t ndeleted, int64_t timestamp_ns, int aggregate, const uint8_t *extends,
                                    uint64_t nextends, uint8_t *out, uint64_t cap, uint64_t *len)
{
    Writer W;
    for (uint64_t i = 0; i < n; ++i) {
        const int st = W.set_packfile_for_blob(rows[i].type, rows[i].packfile, rows[i].checksum, rows[i].offset, rows[i].length);
        if (st != CDC_OK) return st;
    }
    for (uint64_t i = 0; i < ndeleted; ++i) W.delete_snapshot(deleted + kSumBytes * i, deleted_ns[i]);
    if (nextends > (UINT64_MAX - W.size(0)) / kSumBytes) return CDC_E_INVALID;
    *len = W.size(nextends);
    if (*len > cap || !out) return CDC_E_NOSPACE;
    W.write(timestamp_ns, aggregate, extends, nextends, out);
    return CDC_OK;
}

// cdc_state_serialize without its NULL checks.
static inline int serialize(const cdc_state_row *rows, uint64_t n, int64_t timestamp_ns, int aggregate,
                            const uint8_t *extends, uint64_t nextends, uint8_t *out, uint64_t cap, uint64_t *len)
{
    return serialize_deleted(rows, n, nullptr, nullptr, 0, timestamp_ns, aggregate, extends, nextends, out, cap, len);
}

}  // namespace splan

#endif  // SPLAN_NO_WRITER
