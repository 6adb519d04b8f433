// The range planner of cdc_restore_ranges, shared by the library
// (cdc_restore.cpp) and the stand-alone sanitizer program tests/c/
// read_plan_check.cpp.  No HIP, no library state: everything is a function of
// its arguments.
//
// A range (file, offset, length) means the file's bytes [offset, min(offset +
// length, size)): VFilep.Seek's rule (snapshot/vfs/vfilep.go:168-197).  offset
// == size or length == 0 is an empty range that succeeds; offset > size, or a
// file index out of bounds, is CDC_E_INVALID for that range alone; a range
// that touches a chunk whose blob id is kMissing is CDC_E_NOTFOUND, alone too.
//
// Ranges are laid into batches in the caller's order, one (range, chunk)
// overlap after the other.  A batch holds
//   - its distinct blobs (id, recorded length) in order of first use, each
//     with `upto`: the largest end offset inside the blob over every range of
//     the batch that touches it, which is how much of it the batch decodes,
//     and `off`, its place in the scratch buffer: the exclusive sum of upto;
//   - one Segment per overlap: scratch [src_off, + len) -> image [dst_off, + len);
//   - one RPiece per range, or per part of a range: the ranges lie back to
//     back in the output image in the caller's order, so the destinations are
//     sorted and disjoint and cdc_assemble_device takes the segments as they
//     are.
// A batch closes before the overlap that would take its output past
// out_budget or its decoded bytes (the sum of upto) past dec_budget; it always
// takes its first overlap, so it passes a budget by less than one chunk.  A
// range that spans batches is cut there, on a chunk boundary, into pieces.
// Overlapping ranges, the same range twice and ranges in any file order are
// all legal: a blob is decoded once per batch, as far as the batch needs it.
#pragma once

#include <algorithm>

#include "restore_plan.h"

namespace rplan {

constexpr uint32_t kMissing = 0xFFFFFFFFu;  // File::blob of a chunk that no packfile holds

struct Range {
    uint32_t file;
    uint64_t offset, length;
};
struct RBlob {
    uint32_t id;
    uint32_t len;   // the recorded Length
    uint64_t upto;  // bytes of it this batch decodes (1 .. len)
    uint64_t off;   // its place in the scratch buffer
};
struct RPiece {
    uint32_t range;
    uint32_t piece;      // its number among the range's pieces
    uint64_t range_off;  // where it starts in the range
    uint64_t len;
    uint64_t dst_off;    // where it starts in the output image
    uint64_t seg0, nsegs;
    bool last;
};
struct RBatch {
    std::vector<RBlob> blobs;
    std::vector<Segment> segs;
    std::vector<RPiece> pieces;
    uint64_t out_bytes = 0;      // the output image
    uint64_t scratch_bytes = 0;  // the sum of upto
};
struct RangeInfo {
    int status;        // CDC_OK, CDC_E_INVALID or CDC_E_NOTFOUND (then it has no piece)
    uint64_t size;     // the file's size
    uint64_t length;   // the bytes it delivers: min(length, size - offset)
    uint32_t pieces;
};

static inline void plan_ranges(const File *files, size_t nfiles, const Range *ranges, size_t nranges, uint64_t out_budget,
                               uint64_t dec_budget, std::vector<RBatch> &out, std::vector<RangeInfo> &info)
{
    out.clear();
    info.assign(nranges, RangeInfo{CDC_OK, 0, 0, 0});
    if (out_budget == 0) out_budget = 1;
    if (dec_budget == 0) dec_budget = 1;
    std::vector<std::vector<uint64_t>> starts(nfiles);  // per file in use: chunk c begins at starts[c]; [nchunks] is the size
    RBatch cur;
    uint64_t dec = 0;
    std::unordered_map<uint64_t, uint32_t> seen;  // (id, recorded length) -> index into cur.blobs
    auto close = [&] {
        uint64_t off = 0;
        for (RBlob &b : cur.blobs) {
            b.off = off;
            off += b.upto;
        }
        cur.scratch_bytes = off;
        for (Segment &s : cur.segs) s.src_off += cur.blobs[s.blob].off;  // it held the offset inside the blob
        out.push_back(std::move(cur));
        cur = RBatch();
        seen.clear();
        dec = 0;
    };
    for (size_t r = 0; r < nranges; ++r) {
        const Range &R = ranges[r];
        RangeInfo &I = info[r];
        if (R.file >= nfiles) {
            I.status = CDC_E_INVALID;
            continue;
        }
        const File &F = files[R.file];
        std::vector<uint64_t> &S = starts[R.file];
        if (S.empty()) {
            S.resize(size_t(F.nchunks) + 1);
            uint64_t at = 0;
            for (uint64_t c = 0; c < F.nchunks; ++c) {
                S[size_t(c)] = at;
                at += F.len[c];
            }
            S[size_t(F.nchunks)] = at;
        }
        I.size = S[size_t(F.nchunks)];
        if (R.offset > I.size) {
            I.status = CDC_E_INVALID;
            continue;
        }
        I.length = std::min(R.length, I.size - R.offset);
        const uint64_t end = R.offset + I.length;
        RPiece P{};
        P.range = uint32_t(r);
        P.dst_off = cur.out_bytes;
        P.seg0 = cur.segs.size();
        if (I.length == 0) {  // an empty range: one piece without bytes
            P.last = true;
            cur.pieces.push_back(P);
            I.pieces = 1;
            continue;
        }
        // the chunk that holds `offset`: the last one that begins at or before it (empty chunks are passed over)
        const uint64_t c0 = uint64_t(std::upper_bound(S.begin(), S.end() - 1, R.offset) - S.begin()) - 1;
        bool missing = false;
        for (uint64_t c = c0; c < F.nchunks && S[size_t(c)] < end; ++c)
            missing = missing || (F.len[c] && F.blob[c] == kMissing);
        if (missing) {
            I.status = CDC_E_NOTFOUND;
            continue;
        }
        for (uint64_t c = c0; c < F.nchunks && S[size_t(c)] < end; ++c) {
            const uint64_t lo = std::max(S[size_t(c)], R.offset), hi = std::min(S[size_t(c) + 1], end);
            if (hi <= lo) continue;
            const uint64_t in_lo = lo - S[size_t(c)], in_hi = hi - S[size_t(c)], n = hi - lo;
            const uint64_t key = uint64_t(F.blob[c]) << 32 | F.len[c];
            auto it = seen.find(key);
            uint64_t grow = it == seen.end() ? in_hi : in_hi - std::min(in_hi, cur.blobs[it->second].upto);
            if ((cur.out_bytes || dec) && (cur.out_bytes + n > out_budget || dec + grow > dec_budget)) {
                if (P.nsegs) {  // what the range has so far leaves with this batch
                    cur.pieces.push_back(P);
                    ++I.pieces;
                }
                close();
                const uint64_t done = lo - R.offset;
                P = RPiece{};
                P.range = uint32_t(r);
                P.piece = I.pieces;
                P.range_off = done;
                it = seen.end();
                grow = in_hi;
            }
            uint32_t local;
            if (it == seen.end()) {
                local = uint32_t(cur.blobs.size());
                seen.emplace(key, local);
                cur.blobs.push_back(RBlob{F.blob[c], F.len[c], in_hi, 0});
            } else {
                local = it->second;
                cur.blobs[local].upto = std::max(cur.blobs[local].upto, in_hi);
            }
            dec += grow;
            cur.segs.push_back(Segment{in_lo, n, cur.out_bytes, local});
            cur.out_bytes += n;
            P.len += n;
            ++P.nsegs;
        }
        P.last = true;
        cur.pieces.push_back(P);
        ++I.pieces;
    }
    if (!cur.pieces.empty()) close();
}

}  // namespace rplan
