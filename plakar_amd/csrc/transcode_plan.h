// Host-only planning of cdc_transcode_device, shared by the library
// (cdc_transcode.hip) and the stand-alone sanitizer program
// tests/c/transcode_plan_check.cpp:
//
//   * which path a call takes, from the two codecs alone;
//   * per blob, from its stored length: whether a writer can have produced it,
//     its GCM records, and the exact stored length after a transcode that keeps
//     the compression (the envelope changes, the bytes inside it do not);
//   * per batch: the running record base, the output offsets with failed blobs
//     contributing 0 bytes, and the spreading of a sub-batch's results (the
//     blobs that survived a check) back over the whole batch.
//
// The GCM stream is encryption.EncryptStream's (encryption/symmetric.go:72-163):
// subkey nonce (12) || Seal(key, nonce, subkey) (48), then per piece of at most
// 65,536 bytes: nonce (12) || ciphertext || tag (16).  Record boundaries follow
// from the length alone, min(remaining, 65,564) bytes each, as DecryptStream
// reads them (symmetric.go:165-243).
//
// No HIP, no library state: everything is a function of its arguments, and all
// sums are in 64 bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "plakar_cdc.h"

namespace tplan {

constexpr uint64_t kHdr = 60;               // subkey nonce || sealed subkey
constexpr uint64_t kPiece = 65536;          // EncryptStream's chunkSize
constexpr uint64_t kRecMin = 28;            // a nonce and a tag around nothing
constexpr uint64_t kRecMax = kPiece + kRecMin;
constexpr uint64_t kMaxRecords = 0x7FFFFFFFull;  // a batch's records are numbered in 32 bits, as Decode's

enum Path {
    kPathCopy = 0,      // same compression, no key on either side
    kPathRekey = 1,     // same compression, both keys: k_rekey
    kPathOpen = 2,      // same compression, only the source key: Decode with compressed = 0
    kPathSeal = 3,      // same compression, only the destination key: Encode with compress = 0
    kPathReencode = 4,  // different compression: Decode, then Encode, through a device workspace
};

// The selector as Decode and Encode read it: 0 none, 2 GZIP, every other value LZ4.
static inline int selector(int compress) { return compress == CDC_COMPRESS_GZIP ? 2 : compress ? 1 : 0; }

static inline Path choose_path(int src_compress, bool src_key, int dst_compress, bool dst_key)
{
    if (selector(src_compress) != selector(dst_compress)) return kPathReencode;
    if (src_key) return dst_key ? kPathRekey : kPathOpen;
    return dst_key ? kPathSeal : kPathCopy;
}

struct BlobPlan {
    int32_t status;    // CDC_OK, or CDC_E_CORRUPT: a length no writer produces
    uint64_t nrec;     // GCM records the envelope kernels walk: the source's when it is encrypted, else the destination's
    uint64_t payload;  // bytes inside the source's envelope (the stored length when it has none)
    uint64_t out_len;  // stored bytes after the transcode; 0 when status != CDC_OK
};

// A blob of `len` stored bytes whose compression both sides share.
static inline BlobPlan plan_blob(uint64_t len, bool src_encrypted, bool dst_encrypted)
{
    BlobPlan P{CDC_OK, 0, len, 0};
    if (src_encrypted) {
        P.payload = 0;
        if (len < kHdr) {
            P.status = CDC_E_CORRUPT;
            return P;
        }
        const uint64_t rem = len - kHdr;
        P.nrec = rem / kRecMax + (rem % kRecMax ? 1 : 0);
        // a trailing record too short for a nonce and a tag (the reference
        // accepts exactly 12 trailing bytes; no writer produces them)
        if (P.nrec && rem - (P.nrec - 1) * kRecMax < kRecMin) {
            P.status = CDC_E_CORRUPT;
            return P;
        }
        P.payload = rem - kRecMin * P.nrec;
        // both keys: every record keeps its place and its length
        P.out_len = dst_encrypted ? len : P.payload;
        return P;
    }
    if (dst_encrypted) {
        P.nrec = len / kPiece + (len % kPiece ? 1 : 0);
        P.out_len = kHdr + len + kRecMin * P.nrec;
        return P;
    }
    P.out_len = len;
    return P;
}

struct BatchPlan {
    std::vector<BlobPlan> blobs;     // n
    std::vector<uint64_t> rec0;      // n: the running record base (a failed blob has no records)
    std::vector<uint64_t> out_off;   // n + 1: a failed blob contributes 0 bytes
    uint64_t nrecs = 0, total = 0;
};

// CDC_OK, or CDC_E_INVALID when the batch's records cannot be numbered.
static inline int plan_batch(const uint64_t *lens, size_t n, bool src_encrypted, bool dst_encrypted, BatchPlan &B)
{
    B.blobs.resize(n);
    B.rec0.resize(n);
    B.out_off.resize(n + 1);
    uint64_t rec = 0, off = 0;
    for (size_t i = 0; i < n; ++i) {
        BlobPlan P = plan_blob(lens[i], src_encrypted, dst_encrypted);
        if (P.status != CDC_OK) P.nrec = 0;
        B.blobs[i] = P;
        B.rec0[i] = rec;
        B.out_off[i] = off;
        if (P.nrec > kMaxRecords || rec + P.nrec > kMaxRecords) return CDC_E_INVALID;
        rec += P.nrec;
        off += P.out_len;  // cannot wrap: out_len <= len + 60 + 28 nrec and the lengths are those of one device buffer
    }
    B.out_off[n] = off;
    B.nrecs = rec;
    B.total = off;
    return CDC_OK;
}

// A path ran over the sub-batch live[0, m) (ascending indices into the batch
// of n): its offsets sub_off[0, m] and statuses sub_status[0, m) spread over
// the whole batch.  A blob that is not live keeps its status and gets the
// offset of the next live blob (it contributes 0 bytes).
static inline void spread_results(const uint32_t *live, size_t m, const uint64_t *sub_off, const int32_t *sub_status,
                                  size_t n, uint64_t *out_off, int32_t *status)
{
    size_t j = 0;
    for (size_t i = 0; i < n; ++i) {
        out_off[i] = sub_off[j];
        if (j < m && live[j] == i) {
            if (sub_status) status[i] = sub_status[j];
            ++j;
        }
    }
    out_off[n] = sub_off[m];
}

}  // namespace tplan
