// What a GZIP-mode batch of Encode is made of, for the translation units that
// plan one and launch its kernels: cdc_encode.hip (Encode, the streamed gzip
// member) and cdc_zip.hip (many raw DEFLATE streams in one call).  The
// kernels declared at the end are defined in cdc_encode.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdc_crypto_dev.h"
#include "deflate_enc.h"
#include "plakar_cdc.h"  // CDC_LEVEL_*

namespace enc {

using namespace devc;

constexpr uint32_t kSegLZ = 8192;             // LZ4 match-search segment
constexpr uint64_t kBlockLZ = 4ull << 20;     // LZ4 block (pierrec Block4Mb)
constexpr uint32_t kPiece = 65536;            // EncryptStream chunkSize
constexpr uint32_t kHashBits = 11;
constexpr uint32_t kRecCap = kSegLZ / 4 + 2;  // records per segment (a match per 4 bytes at most)

struct Seg {             // an 8-KiB LZ4 search segment
    uint64_t src;        // byte offset in the input base
    uint16_t len;
    uint16_t hist;       // bytes before it a match may copy from: 0 at CDC_LEVEL_FAST, at CDC_LEVEL_WIDE
                         // min(kWideHist, its offset in its LZ4 block): never before the block, blob or piece
    uint32_t rem;        // bytes from the segment's start to its LZ4 block's end
};
static_assert(sizeof(Seg) == 16 && kSegLZ <= 0xFFFFu, "len and hist share the word len alone had");

constexpr uint32_t kWideHist = 32768;  // CDC_LEVEL_WIDE's window before a segment (DEFLATE's; half of LZ4's reach)

// A segment's hist at `level`: seg_off is its offset in its 4-MiB block.
inline uint16_t seg_hist(int level, uint32_t seg_off) { return level ? uint16_t(seg_off < kWideHist ? seg_off : kWideHist) : uint16_t(0); }

struct Blk {             // a 4-MiB LZ4 block
    uint64_t src;
    uint32_t len, blob;
    uint32_t seg0, nseg;
    uint32_t k;          // block index in its blob
    uint32_t pad;
};

struct BlobDesc {
    uint64_t src;        // byte offset in the input base
    uint64_t len;
    uint64_t slot;       // frame slot in the frame buffer (16-B aligned)
    uint32_t blk0, nblk;
};

struct Span {            // a DEFLATE span: up to dfl::kSpanSegs segments of one blob
    uint64_t src;
    uint32_t len, blob;
    uint32_t seg0, nseg;
    uint32_t k;          // span index in its blob
    uint32_t last;       // the blob's last span: its block carries BFINAL
};

struct SpanOut {         // what the DEFLATE stages hand on, per span
    uint32_t fixed_bits, dyn_bits;  // the whole block coded either way (k_dfl_size)
    uint32_t hdr_bits;              // the dynamic header
    uint32_t crc;                   // CRC-32 register over the span's bytes from 0, no final inversion
    uint32_t type, nbits;           // the choice and the block's bits (k_enc_plan)
    uint64_t bit;                   // where the block starts, in bits from the member's start
    uint32_t edge_lo, edge_hi;      // its bits in the bytes it shares with its neighbours (k_dfl_emit)
};

constexpr uint32_t kSpanLens = dfl::kLitSlots + dfl::kDistSlots;  // code lengths kept per span

struct Batch {
    const uint8_t *base;
    uint32_t nblobs, nsegs, nblks, npieces_max;
    uint32_t compress, encrypt;
    const BlobDesc *blobs;
    const Seg *segs;
    const Blk *blks;
    const uint8_t *rnd;       // per blob: subkey 32, subkey nonce 12, data nonce 12
    const uint8_t *key;       // repository key (32 B, device)
    uint8_t *frames;          // frame buffer
    uint8_t *out;
    uint64_t out_cap;
    // workspace
    uint2 *recs;              // kRecCap per segment
    uint32_t *nrec;           // per segment
    uint32_t *trail;          // per segment: literals after its last match (from its start when none)
    uint32_t *seg_out;        // per segment: bytes of its sequences in the block (k_lz4_size)
    uint32_t *blk_size;       // per block: encoded size, bit 31 = stored raw
    uint64_t *blk_foff;       // per block: offset of its header in the frame
    uint32_t *xxh;            // per blob
    uint64_t *frame_len;      // per blob
    uint64_t *out_off;        // nblobs + 1
    uint32_t *piece_base;     // nblobs + 1
    BlobKey *keys;            // per blob
    uint64_t *status;         // [0]: CDC_E_NOSPACE when out_cap is too small
    const uint32_t *xx_ids;   // XXH32 order of the blobs
    // GZIP (compress == 2)
    uint32_t nspans;
    const Span *spans;
    const uint32_t *blob_span0;  // nblobs + 1
    SpanOut *sp;
    uint8_t *sp_lens;         // kSpanLens per span: literal/length then distance code lengths
    uint32_t *sp_hdr;         // dfl::kHdrWords per span: the dynamic header's bits
};

constexpr uint32_t kSeqWaves = 2;  // 12 KiB of LDS per wave (the segment and the hash table)
constexpr uint32_t kDflThreads = dfl::kStretches;
static_assert(kDflThreads == 256 && dfl::kSeg == kSegLZ && kBlockLZ % dfl::kSpan == 0, "a span is four segments of one block");

// Defined in cdc_encode.hip; another translation unit launches them through
// their host stubs (the device code stays in cdc_encode.hip's code object).
__global__ __launch_bounds__(kSeqWaves * 64) void k_lz4_seq(const Batch B);
__global__ __launch_bounds__(64) void k_lz_seq_wide(const Batch B);  // a wave per segment and workgroup
__global__ __launch_bounds__(64) void k_lz_seq_deep(const Batch B);  // the same, four candidates per bucket and a lazy look
__global__ __launch_bounds__(kDflThreads) void k_dfl_size(const Batch B);
__global__ __launch_bounds__(kDflThreads) void k_dfl_emit(const Batch B);

// The match search of a batch's ng segments at `level` (the plan filled Seg.hist with seg_hist at the same level).
inline void launch_seq(const Batch &Bt, int level, size_t ng, hipStream_t s)
{
    if (!ng) return;
    if (level == CDC_LEVEL_BEST) hipLaunchKernelGGL(k_lz_seq_deep, dim3(uint32_t(ng)), dim3(64), 0, s, Bt);
    else if (level) hipLaunchKernelGGL(k_lz_seq_wide, dim3(uint32_t(ng)), dim3(64), 0, s, Bt);
    else hipLaunchKernelGGL(k_lz4_seq, dim3(uint32_t((ng + kSeqWaves - 1) / kSeqWaves)), dim3(kSeqWaves * 64), 0, s, Bt);
}

}  // namespace enc
