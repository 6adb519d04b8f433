// The reader layer of the runs that read blobs out of registered packfiles by
// checksum, on top of the host-only blob source (cdc_blobsrc.h):
//
//   PackSource    what every such context holds: the device, the repository's
//                 codec (compression and a copy of the key), the locator, the
//                 stored-form codec and the lock that serialises runs, with
//                 the bodies of the context's cdc_*_add_packfile* functions;
//   Arena, gather a batch's encoded blobs read into a pinned arena on N threads
//                 and uploaded in one copy;
//   decode_batch  Decode + check over the arena's blobs, each compared with
//                 its recorded Length, with the one-by-one pass for a batch
//                 that holds a blob longer than recorded.
//
// What a run does with the plaintext (assemble, hash, search, deflate) and how
// it answers a failed blob stay with the run.  DESIGN.md 5.27.  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "cdc_blobsrc.h"
#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "cdc_stored.h"

namespace cdc {

struct PackSource {
    int device = 0;
    int compress = CDC_COMPRESS_NONE;
    std::vector<uint8_t> key;  // a copy of the caller's 32 bytes, or empty
    Locator loc;               // the registered packfiles: checksum -> blob id -> (packfile, offset, length)
    std::unique_ptr<StoredCodec> stored;  // made at the first stored source (add_many)
    std::mutex run_mu;         // held by a run, and while a packfile is entered

    void open(int device_, int compress_, const uint8_t *key32)
    {
        device = device_;
        compress = compress_;
        if (key32) key.assign(key32, key32 + 32);
    }
    const uint8_t *key_ptr() const { return key.empty() ? nullptr : key.data(); }

    // The bodies of cdc_*_add_packfile and cdc_*_add_packfile_path: they wait for a run to end.
    int add_memory(const uint8_t *bytes, uint64_t len);
    int add_path(const char *path);
    // cdc_*_add_packfiles: CDC_E_INVALID while a run is in progress.
    int add_many(const cdc_packfile_src *srcs, uint32_t n, int32_t *status);
    // The context's end: its streams drained and destroyed, the key zeroed.
    void release(hipStream_t *streams, int n);
};

// A batch's encoded blobs on their way to the device.  The caller fills
// `spans`; gather_read lays them out and reads them, gather uploads them too.
struct Arena {
    PinBuf h;
    DevBuf d;
    std::vector<Span> spans;
    std::vector<uint64_t> eoff, elen;  // the blobs in the arena
    std::vector<int32_t> pre;          // a blob that could not be read (CDC_E_IO)
    uint64_t total = 0;

    template <class Blob>  // the plan's blobs: .id is the locator's blob id
    void set_blobs(const Locator &loc, const Blob *blobs, size_t n)
    {
        spans.resize(n);
        for (size_t b = 0; b < n; ++b) spans[b] = span_of(loc, blobs[b].id);
    }
};

// Lay out and read A.spans into A.h (`threads` threads), with room for `tail`
// more pinned bytes from the next 16-byte boundary behind the blobs, and room
// for the blobs in A.d.  CDC_OK or CDC_E_NOMEM; the seconds go to *read_s, the
// blobs' bytes to *encoded_bytes (may be NULL).
int gather_read(const Locator &loc, Arena &A, int threads, uint64_t tail, double *read_s, uint64_t *encoded_bytes);
// gather_read, then one copy to A.d on `stream` and a synchronise (*h2d_s).  CDC_OK, CDC_E_NOMEM, CDC_E_DEVICE.
int gather(const Locator &loc, Arena &A, int threads, hipStream_t stream, double *read_s, double *h2d_s,
           uint64_t *encoded_bytes);

// The repository's codec and where Decode runs, for the calls below.
struct DecodeCtx {
    int device;
    int compress;
    const uint8_t *key;
    bool verify;  // compare every blob's SHA-256 with its checksum in the locator
    hipStream_t stream;
};
// The decode step's view of a batch and what it leaves: per blob its status
// (CDC_OK, Decode's or the check's, CDC_E_MISMATCH for a wrong length, the
// read's CDC_E_IO) and its place in the destination, and the destination's
// bytes in use.  Kept across batches, its vectors are reused.
struct Decoded {
    std::vector<int32_t> bst;
    std::vector<uint64_t> pos;
    uint64_t plain_used = 0;
    // the plan's blobs (set_blobs): recorded Length, planned offset, checksum when verify is set
    std::vector<uint32_t> len;
    std::vector<uint64_t> off;
    std::vector<uint8_t> want;
    std::vector<uint64_t> oo;  // scratch: Decode's offsets

    template <class Blob>  // .id, .len, .off
    void set_blobs(bool verify, const Locator &loc, const Blob *blobs, size_t n)
    {
        len.resize(n);
        off.resize(n);
        want.resize(verify ? n * 32 + 1 : 0);
        for (size_t b = 0; b < n; ++b) {
            len[b] = blobs[b].len;
            off[b] = blobs[b].off;
            if (verify) std::memcpy(&want[b * 32], loc.sums[blobs[b].id].b, 32);
        }
    }
};
struct DecodeTally {  // added to, never reset
    uint64_t *decoded_bytes;
    double *decode_s, *verify_s;
};

// The fast half: one Decode + check over the arena's blobs (D.set_blobs names
// them), compacted into dst[0, cap), each blob's length compared with its
// recorded one.  CDC_OK, CDC_E_NOSPACE (some blob decodes to more than its
// recorded Length, by an amount only its own bytes bound: decode_one_by_one
// tells which; D is not valid), or the call's own failure.
int decode_together(const DecodeCtx &C, Arena &A, uint8_t *dst, uint64_t cap, Decoded &D, const DecodeTally &T);
// The slow half, for a batch decode_together answered with CDC_E_NOSPACE: the
// blobs one by one, each into the room its Length gives it at its planned
// offset in dst[0, plain_bytes): the ones that fit come out, the others are
// CDC_E_MISMATCH.
int decode_one_by_one(const DecodeCtx &C, Arena &A, uint8_t *dst, uint64_t plain_bytes, Decoded &D, const DecodeTally &T);
// Both halves into one destination of plain_bytes (the plan's sum of lengths).
inline int decode_batch(const DecodeCtx &C, Arena &A, uint8_t *dst, uint64_t plain_bytes, Decoded &D, const DecodeTally &T)
{
    const int st = decode_together(C, A, dst, plain_bytes, D, T);
    return st == CDC_E_NOSPACE ? decode_one_by_one(C, A, dst, plain_bytes, D, T) : st;
}

}  // namespace cdc
