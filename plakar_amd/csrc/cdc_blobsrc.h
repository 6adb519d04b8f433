// The blob source of the runs that read blobs out of registered packfiles
// (restore, read, archive, check, diff, grep, sync): where a batch's encoded
// blobs lie, their layout in one arena, and the threaded read into it.  Host
// only: no HIP include, the arena is a raw pointer (tests/c/blobsrc_check.cpp).
// cdc_reader.h puts the pinned and device buffers and Decode on top.
#pragma once

#include <stdint.h>

#include <vector>

#include "cdc_locator.h"

namespace cdc {

struct Span {  // an encoded blob: bytes [offset, offset + length) of a registered packfile
    uint32_t pack;
    uint64_t offset, length;
};
inline Span span_of(const Locator &loc, uint32_t blob_id)
{
    const Locator::Loc &L = loc.locs[blob_id];
    return Span{L.pack, L.offset, L.length};
}
inline Span span_of(uint32_t pack, const cdc_packfile_row &row) { return Span{pack, row.offset, row.length}; }

// The spans back to back: eoff[b] and elen[b] of every span; returns the total.
uint64_t lay_out(const Span *spans, size_t n, std::vector<uint64_t> &eoff, std::vector<uint64_t> &elen);

// Span b's bytes to dst + eoff[b], on up to `threads` threads: memcpy from a
// packfile in memory, pread from one registered by path, each such file opened
// once and closed again before the return.  pre[b] = CDC_OK, or CDC_E_IO for a
// span that could not be read; nothing is copied for an empty span.  dst NULL
// (the caller found no room): pre is filled with CDC_OK and nothing is opened.
void read_spans(const Locator &loc, const Span *spans, size_t n, const uint64_t *eoff, uint8_t *dst, int threads,
                int32_t *pre);

// ids[c] = the blob id of checksums[32 c ..), for c < nchunks.  Returns -1, or
// the index of the first checksum in no registered packfile (ids from there on
// are not written).
int64_t resolve(const Locator &loc, const uint8_t *checksums, uint64_t nchunks, uint32_t *ids);

}  // namespace cdc
