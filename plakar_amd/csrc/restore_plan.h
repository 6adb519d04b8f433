// Host-only pieces of the restore path, shared by the library (cdc_restore.cpp)
// and the stand-alone sanitizer program tests/c/restore_plan_check.cpp:
//
//   * the packfile index reader: packfile.NewFromBytes (packfile/packfile.go:
//     152-239) for the plain Serialize form (packfile.go:241-294);
//   * the batch planner of cdc_restore_files: which blobs a batch decodes
//     (each distinct one once) and where every chunk occurrence lands.
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "plakar_cdc.h"

namespace rplan {

constexpr uint64_t kFooterBytes = 52;  // u32 version, i64 timestamp, u32 count, u32 index offset, 32-B SHA-256
constexpr uint64_t kRowBytes = 41;     // u8 type, 32-B checksum, u32 offset, u32 length
constexpr uint32_t kPackVersion = 100;
constexpr uint8_t kTypeChunk = 1;      // packfile.TYPE_CHUNK

typedef void (*sha256_fn)(const void *data, size_t n, uint8_t out[32]);

static inline uint32_t rd32(const uint8_t *p)
{
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}
static inline uint64_t rd64(const uint8_t *p) { return uint64_t(rd32(p)) | uint64_t(rd32(p + 4)) << 32; }

// The footer: the last 52 bytes of a packfile of total_len bytes.  CDC_OK, or
// CDC_E_CORRUPT: shorter than a footer, a version other than 100, or an index
// that is not exactly 41 * count bytes between the index offset and the footer.
static inline int parse_footer(const uint8_t *last52, uint64_t total_len, cdc_packfile_footer *f)
{
    if (total_len < kFooterBytes) return CDC_E_CORRUPT;
    memset(f, 0, sizeof(*f));
    f->version = rd32(last52);
    f->timestamp = int64_t(rd64(last52 + 4));
    f->count = rd32(last52 + 12);
    f->index_offset = rd32(last52 + 16);
    memcpy(f->index_checksum, last52 + 20, 32);
    if (f->version != kPackVersion) return CDC_E_CORRUPT;
    const uint64_t body = total_len - kFooterBytes;
    if (f->index_offset > body || body - f->index_offset != kRowBytes * uint64_t(f->count)) return CDC_E_CORRUPT;
    return CDC_OK;
}

// The index: 41 * f.count bytes.  Writes at most cap rows (rows may be NULL
// when cap is 0); every row is checked whatever cap is.  CDC_E_CORRUPT: an
// entry that ends past the index offset, or an index whose SHA-256 is not the
// footer's.
static inline int parse_index(const uint8_t *index, const cdc_packfile_footer &f, sha256_fn sha,
                              cdc_packfile_row *rows, uint64_t cap)
{
    for (uint64_t i = 0; i < f.count; ++i) {
        const uint8_t *e = index + kRowBytes * i;
        const uint32_t off = rd32(e + 33), len = rd32(e + 37);
        if (uint64_t(off) + len > f.index_offset) return CDC_E_CORRUPT;
        if (i < cap) {
            cdc_packfile_row &r = rows[i];
            memset(&r, 0, sizeof(r));
            memcpy(r.checksum, e + 1, 32);
            r.offset = off;
            r.length = len;
            r.type = e[0];
        }
    }
    uint8_t got[32];
    sha(index, size_t(kRowBytes * f.count), got);
    return memcmp(got, f.index_checksum, 32) == 0 ? CDC_OK : CDC_E_CORRUPT;
}

// A whole packfile in memory (cdc_packfile_index).
static inline int parse_packfile(const uint8_t *bytes, uint64_t len, sha256_fn sha, cdc_packfile_footer *f,
                                 cdc_packfile_row *rows, uint64_t cap)
{
    if (!bytes || len < kFooterBytes) return CDC_E_CORRUPT;
    const int st = parse_footer(bytes + (len - kFooterBytes), len, f);
    if (st != CDC_OK) return st;
    return parse_index(bytes + f->index_offset, *f, sha, rows, cap);
}

// ---- batch planner -----------------------------------------------------------
// A file is its chunk list: blob[i] names chunk i's blob (any id that is
// equal for equal checksums), len[i] is the recorded Length.  Files are laid
// into batches in order, chunk by chunk; a batch closes before the chunk that
// would take its output past `budget` (a batch always takes its first chunk,
// so it exceeds the budget by less than one chunk), and a file that spans
// batches is cut there, on a chunk boundary, into pieces.
struct File {
    uint64_t nchunks;
    const uint32_t *blob;
    const uint32_t *len;
};
struct Segment {      // one chunk occurrence
    uint64_t src_off; // in the batch's plaintext buffer (distinct blobs back to back)
    uint64_t len;
    uint64_t dst_off; // in the batch's output image (pieces back to back)
    uint32_t blob;    // index into Batch::blobs
};
struct Piece {        // the part of one file that one batch holds
    uint32_t file;
    uint64_t chunk0, nchunks;  // file chunks [chunk0, chunk0 + nchunks)
    uint64_t file_off;         // where the piece starts in the file
    uint64_t len;
    uint64_t dst_off;          // where it starts in the output image
    uint64_t seg0;             // its first segment
    bool first, last;
};
struct Blob {         // a distinct (blob id, recorded length) of one batch, in order of first use
    uint32_t id;
    uint32_t len;
    uint64_t off;     // its place in the plaintext buffer (prefix sum of len)
};
struct Batch {
    std::vector<Blob> blobs;
    std::vector<Segment> segs;
    std::vector<Piece> pieces;
    uint64_t out_bytes = 0;    // the output image
    uint64_t plain_bytes = 0;  // the plaintext buffer: sum of the distinct blobs' lengths
    bool identity = true;      // every segment has src_off == dst_off: the plaintext buffer is the image
};

static inline void plan(const File *files, size_t nfiles, uint64_t budget, std::vector<Batch> &out)
{
    out.clear();
    if (budget == 0) budget = 1;
    Batch cur;
    std::unordered_map<uint64_t, uint32_t> seen;  // (id, recorded length) -> index into cur.blobs
    auto close = [&] {
        out.push_back(std::move(cur));
        cur = Batch();
        seen.clear();
    };
    for (size_t fi = 0; fi < nfiles; ++fi) {
        const File &F = files[fi];
        uint64_t c = 0, file_off = 0;
        bool first = true;
        do {
            Piece P{};
            P.file = uint32_t(fi);
            P.chunk0 = c;
            P.file_off = file_off;
            P.dst_off = cur.out_bytes;
            P.seg0 = cur.segs.size();
            P.first = first;
            while (c < F.nchunks) {
                const uint64_t len = F.len[c];
                if (cur.out_bytes != 0 && cur.out_bytes + len > budget) break;
                const uint64_t key = uint64_t(F.blob[c]) << 32 | len;
                auto it = seen.find(key);
                uint32_t local;
                if (it == seen.end()) {
                    local = uint32_t(cur.blobs.size());
                    seen.emplace(key, local);
                    cur.blobs.push_back(Blob{F.blob[c], uint32_t(len), cur.plain_bytes});
                    cur.plain_bytes += len;
                } else {
                    local = it->second;
                }
                const Segment S{cur.blobs[local].off, len, cur.out_bytes, local};
                if (S.src_off != S.dst_off) cur.identity = false;
                cur.segs.push_back(S);
                cur.out_bytes += len;
                P.len += len;
                ++c;
            }
            P.nchunks = c - P.chunk0;
            P.last = c == F.nchunks;
            file_off += P.len;
            // a piece that could take no chunk (the batch was full) is not recorded
            if (P.nchunks || P.last) {
                cur.pieces.push_back(P);
                first = false;
            }
            if (!P.last) close();
        } while (c < F.nchunks);
    }
    if (!cur.pieces.empty()) close();
}

}  // namespace rplan
