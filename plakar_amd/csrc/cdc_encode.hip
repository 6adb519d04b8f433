// Encode on the device: plakar's (*Repository).Encode
// (repository/repository.go:212-236) of a batch of blobs: the LZ4 frame of
// compression.DeflateLZ4Stream (compression/compression.go:94-106,
// github.com/pierrec/lz4/v4 v4.1.18 NewWriter defaults: independent blocks of
// at most 4 MiB, content checksum on), then the AES-256-GCM stream of
// encryption.EncryptStream (encryption/symmetric.go:72-163): a random subkey
// sealed under the repository key, then every 64-KiB piece of the
// compressed stream sealed under the subkey with its own nonce.
//
// Kernels, in launch order (one batch = the blobs of one call):
//   k_xxh32       XXH32 of every blob (the frame's content checksum), on a
//                 side stream: one blob per wave, a lane quad's four chains
//   k_lz4_seq     one wave per 8-KiB segment: greedy LZ4 match search, 64
//                 positions per step at LZ4's accelerating stride (hash table
//                 of 2,048 u16 in LDS, matches found by ballot, extended 64
//                 bytes per step both ways); sequences out as (match start,
//                 offset, length) records
//   k_lz4_size    one workgroup per 4-MiB LZ4 block: literal runs across
//                 segment boundaries, encoded size (raw when not smaller)
//   k_enc_plan    one workgroup: frame sizes, block offsets in the frame,
//                 GCM pieces and output offsets of every blob (scans)
//   k_lz4_emit    a workgroup per block (16 per stored block): its bytes
//   k_frame_fin   one wave per blob: frame header, end mark, checksum
//   k_blob_keys   one thread per blob: the subkey's round keys, H and its
//                 4-bit table, and the sealed subkey (header)
//   k_blob_pows   one wave per blob: H^1..H^64 (a doubling ladder over the
//                 lanes) and the 8-bit table of H^64
//   k_gcm         one wave per 64-KiB piece: AES-256-CTR (two rotated
//                 T-tables in LDS, 32 bank-conflict-free copies each; rounds
//                 1-2 partly once per piece) and GHASH (lane l hashes blocks
//                 l, l+64, ... by Horner in H^64 with an 8-bit table, reduced
//                 once per block, then multiplies by its own H^e), tag
//
// Matches stay inside their 8-KiB segment, so compression ratios are those
// of LZ4 with an 8-KiB window; any LZ4 decoder reads the frames (the tests
// decode them with the system's liblz4).  At CDC_LEVEL_WIDE
// (cdc_encode_device_level) k_lz_seq_wide runs in k_lz4_seq's place: the same
// records, from a window that starts up to 32 KiB before the segment (Seg.hist)
// and never before its 4-MiB block or its blob; every later kernel is the same.  Nonces and subkeys come from the
// caller (the host fills them from the OS CSPRNG), as crypto/rand does in
// the reference; piece k of a blob uses the blob's data nonce with its last
// four bytes XOR k (big-endian), unique per subkey.
//
// compress == CDC_COMPRESS_GZIP writes the gzip member of
// compression.DeflateGzipStream (compression/compression.go:78-92) instead of
// the LZ4 frame: k_lz4_seq's records feed a DEFLATE writer (deflate_enc.h),
//   k_dfl_size    one workgroup per 32-KiB span (four segments): histograms,
//                 code lengths, the dynamic header, the block's size as fixed
//                 and as dynamic Huffman, and the span's CRC-32
//   k_enc_plan    also walks each blob's spans: stored, fixed or dynamic by
//                 exact bit count at the running bit position
//   k_dfl_emit    one workgroup per span: its block, packed in LDS
//   k_gz_fin      one wave per blob: header, the bytes two spans share, the
//                 CRC-32 combined from the spans', ISIZE
// in the place of k_xxh32, k_lz4_size, k_lz4_emit and k_frame_fin.
//
// cdc_gzip_stream_piece writes one gzip member piece by piece (archive's
// tarball): a piece is one blob of such a batch with no final block, and
//   k_gzs_plan    one wave: each span's form at its bit, the joiner, the
//                 piece's length against out_cap
//   k_gzs_fin     one wave: header (first piece), shared bytes, the joiner,
//                 the piece's CRC-32; final block and trailer (last piece)
// stand in the place of k_enc_plan and k_gz_fin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "cdc_internal.h"
#include "cdc_crypto_dev.h"
#include "cdc_hostmem.h"
#include "cdc_encode_dev.h"  // Seg, Blk, BlobDesc, Span, SpanOut, Batch and the sizes they are planned with
#include "deflate_enc.h"
#include "inflate_walk.h"

namespace enc {

using namespace devc;

// ---------------------------------------------------------------------------
// AES tables, built on the host (FIPS-197: S-box = affine(inverse in GF(2^8))).
// ---------------------------------------------------------------------------
__device__ uint32_t g_te0[256];
__device__ uint8_t g_sbox[256];

void build_tables(uint32_t te0[256], uint8_t sbox[256])  // cdc_decode.hip uploads its own copies
{
    auto mul = [](uint8_t a, uint8_t b) {
        uint8_t p = 0;
        for (int i = 0; i < 8; ++i) {
            if (b & 1) p ^= a;
            const uint8_t hi = a & 0x80;
            a = uint8_t(a << 1);
            if (hi) a ^= 0x1B;
            b >>= 1;
        }
        return p;
    };
    for (int x = 0; x < 256; ++x) {
        uint8_t inv = 0;
        if (x)
            for (int y = 1; y < 256; ++y)
                if (mul(uint8_t(x), uint8_t(y)) == 1) {
                    inv = uint8_t(y);
                    break;
                }
        uint8_t s = inv;
        for (int i = 1; i <= 4; ++i) s ^= uint8_t((inv << i) | (inv >> (8 - i)));
        sbox[x] = uint8_t(s ^ 0x63);
    }
    for (int x = 0; x < 256; ++x) {
        const uint8_t s = sbox[x];
        te0[x] = uint32_t(mul(s, 2)) << 24 | uint32_t(s) << 16 | uint32_t(s) << 8 | mul(s, 3);
    }
}

// ---------------------------------------------------------------------------
// XXH32 (the frame's content checksum): lanes 0-3 run accumulators v1..v4 over
// the 16-byte stripes, lane 0 the tail.
// ---------------------------------------------------------------------------

// A wave hashes kXxPerWave blobs (sorted longest first on the host: the
// longest chains start first).  Their stripes stream through LDS, a region of
// kXxRegion / kXxPerWave bytes per blob at a time, regions r + 1 and r + 2 in
// flight while lane quad g runs blob g's four accumulator chains (lane a:
// accumulator a) over region r.  The loading lanes store each word already
// multiplied by PRIME32_2, so a chain step is add, rotate, multiply.  A batch
// takes as long as its longest blob's chain (a 4-MiB blob: 262,144 steps);
// more blobs per wave (less idle VALU work) measured slower, because the chain
// latency, not VALU throughput, bounds it.
constexpr uint32_t kXxWaves = 4;
constexpr uint32_t kXxRegion = 4096;                 // bytes per wave per stage
constexpr uint32_t kXxPerWave = 1;                   // blobs per wave
constexpr uint32_t kXxBlobRegion = kXxRegion / kXxPerWave;
constexpr uint32_t kXxLoadLanes = 64 / kXxPerWave;  // lanes loading one blob's region
static_assert(kXxBlobRegion == 16 * 4 * kXxLoadLanes, "16 words per loading lane");

__global__ __launch_bounds__(kXxWaves * 64) void k_xxh32(const Batch B)
{
    __shared__ uint32_t s_buf[kXxWaves][2][kXxRegion / 4];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t i0 = (blockIdx.x * kXxWaves + wv) * kXxPerWave;  // the wave's first blob (sorted order)
    if (i0 >= B.nblobs) return;
    // the blob this lane loads for (lg) and, for lanes < 4 kXxPerWave, chains (cg)
    const uint32_t lg = lane / kXxLoadLanes, sub = lane % kXxLoadLanes, cg = lane >> 2, a = lane & 3u;
    auto blob = [&](uint32_t g, const uint8_t *&p, uint64_t &n, uint32_t &w) {
        const bool ok = i0 + g < B.nblobs;
        w = ok ? B.xx_ids[i0 + g] : 0u;
        p = B.base + (ok ? B.blobs[w].src : 0);
        n = ok ? B.blobs[w].len : 0;
    };
    const uint8_t *lp, *cp;
    uint64_t ln, cn;
    uint32_t lw, cw;
    blob(lg, lp, ln, lw);
    blob(cg < kXxPerWave ? cg : 0u, cp, cn, cw);
    const uint64_t cstripes = cg < kXxPerWave ? cn / 16 : 0;
    // a global-address-space pointer: flat loads would also count in
    // lgkmcnt, so every LDS wait of the chains would wait for the prefetch too
    const gu32 *A = reinterpret_cast<const gu32 *>(reinterpret_cast<uintptr_t>(lp) & ~uintptr_t(3));
    const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(lp) & 3u) * 8u;
    // regions: the wave's longest blob (its first: sorted)
    uint64_t n0;
    {
        const uint8_t *p0;
        uint32_t w0;
        blob(0, p0, n0, w0);
    }
    const uint64_t R = (n0 / 16 * 16 + kXxBlobRegion - 1) / kXxBlobRegion;
    // regions r + 1 and r + 2 are in flight (register sets X and Y, taking
    // turns) while the chains run over region r in LDS
    uint32_t X[16], Y[16];
    // Branch-free loads (a load under a lane condition makes the compiler wait
    // for it before the branch joins, serialising the prefetch): indices are
    // clamped to the blob's last aligned word.
    // A misaligned word takes its last bytes from the next aligned word, which
    // holds some of the blob's bytes; an aligned one ignores it (shift 0).
    const uint64_t klast = ln ? ((reinterpret_cast<uintptr_t>(lp) & 3u) + ln - 1) / 4 : 0;
    auto prefetch = [&](uint32_t (&pw)[16], uint64_t r) {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const uint64_t k = r * (kXxBlobRegion / 4) + 16 * sub + i;  // blob word
            const uint64_t k0 = min(k, klast), k1 = min(k + 1, klast);
            // the round's input product, off the chain (words past the stripes
            // are loaded from the clamped index and never consumed)
            pw[i] = __builtin_amdgcn_alignbit(A[k1], A[k0], sh) * P2;
        }
    };
    auto store = [&](const uint32_t (&pw)[16], uint64_t r) {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) s_buf[wv][r & 1][16 * lane + i] = pw[i];
    };
    uint32_t v = a == 0 ? P1 + P2 : a == 1 ? P2 : a == 2 ? 0u : 0u - P1;
    auto chains = [&](uint64_t r) {
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): region r is in LDS
        __builtin_amdgcn_wave_barrier();
        const uint64_t done = r * (kXxBlobRegion / 16);
        if (cstripes > done) {
            const uint32_t *bw = s_buf[wv][r & 1] + cg * (kXxBlobRegion / 4);
            const uint32_t ns = uint32_t(min<uint64_t>(kXxBlobRegion / 16, cstripes - done));
            uint32_t s = 0;
            for (; s + 8 <= ns; s += 8) {
                uint32_t in[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) in[j] = bw[4 * (s + j) + a];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) v = rol32(v + in[j], 13) * P1;
            }
            for (; s < ns; ++s) v = rol32(v + bw[4 * s + a], 13) * P1;
        }
        __builtin_amdgcn_wave_barrier();
    };
    if (R) {
        prefetch(X, 0);
        store(X, 0);
        prefetch(X, 1);
        prefetch(Y, 2);
    }
    // step r: chains over r; region r + 1 (set of parity r) into LDS; its set loads r + 3
    for (uint64_t r = 0; r < R; r += 2) {
        chains(r);
        if (r + 1 < R) {
            store(X, r + 1);
            prefetch(X, r + 3);
            chains(r + 1);
            if (r + 2 < R) {
                store(Y, r + 2);
                prefetch(Y, r + 4);
            }
        }
    }
    const uint32_t qb = lane & ~3u;
    const uint32_t v1 = __shfl(v, int(qb)), v2 = __shfl(v, int(qb + 1)), v3 = __shfl(v, int(qb + 2)),
                   v4 = __shfl(v, int(qb + 3));
    if (a == 0 && cg < kXxPerWave && i0 + cg < B.nblobs) B.xxh[cw] = xxh_finish(v1, v2, v3, v4, cp, cn);
}

// ---------------------------------------------------------------------------
// k_lz4_seq: one wave per segment.  Record = (match start | offset << 16,
// match length), segment-relative; the literals before a match are the bytes
// since the previous match's end.
// ---------------------------------------------------------------------------
constexpr uint32_t kSkipShift = 6;  // LZ4's skip trigger

struct alignas(16) SeqLds {
    uint32_t data[kSegLZ / 4 + 4];
    uint16_t tab[1u << kHashBits];
};

__device__ __forceinline__ uint32_t lds_rd32(const SeqLds &L, uint32_t p)  // bytes p..p+3 (any p)
{
    const uint32_t w0 = L.data[p >> 2], w1 = L.data[(p >> 2) + 1];
    return __builtin_amdgcn_alignbit(w1, w0, (p & 3u) * 8u);
}

__device__ __forceinline__ uint32_t lds_rd8(const SeqLds &L, uint32_t p)
{
    return (L.data[p >> 2] >> ((p & 3u) * 8u)) & 255u;
}

__global__ __launch_bounds__(kSeqWaves * 64) void k_lz4_seq(const Batch B)
{
    __shared__ SeqLds s_l[kSeqWaves];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * kSeqWaves + wv;
    if (g >= B.nsegs) return;
    SeqLds &L = s_l[wv];
    const Seg S = B.segs[g];
    const uint8_t *src = B.base + S.src;
    const uint32_t n = S.len;
    // the segment into LDS, 16 bytes per lane and load (unaligned global
    // loads, all issued before the first store); a short segment's tail is
    // zero-filled from byte loads
    if (n == kSegLZ) {
        uint4 v[kSegLZ / 1024];
#pragma unroll
        for (uint32_t j = 0; j < kSegLZ / 1024; ++j) __builtin_memcpy(&v[j], src + 1024 * j + 16 * lane, 16);
#pragma unroll
        for (uint32_t j = 0; j < kSegLZ / 1024; ++j) *reinterpret_cast<uint4 *>(&L.data[256 * j + 4 * lane]) = v[j];
    } else for (uint32_t i = lane; i < kSegLZ / 16; i += 64) {
        const uint32_t p = 16 * i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p + 16 <= n) {
            __builtin_memcpy(&v, src + p, 16);
        } else if (p < n) {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; p + b < n; ++b) w[b >> 2] |= uint32_t(src[p + b]) << (8 * (b & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(&L.data[4 * i]) = v;
    }
    if (lane < 4) L.data[kSegLZ / 4 + lane] = 0;
    for (uint32_t i = lane; i < (1u << kHashBits); i += 64) L.tab[i] = 0;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // LZ4 block rules: a match starts >= 12 bytes before the block's end and
    // the block's last 5 bytes are literals (segments near the end of a block
    // are limited by the block's end, not their own); and a match's first 4
    // bytes lie inside the segment.
    const uint32_t start_lim = min(n >= 4 ? n - 3 : 0u, S.rem > 12 ? S.rem - 12 : 0u);
    const uint32_t end_lim = min(n, S.rem > 5 ? S.rem - 5 : 0u);
    uint2 *rec = B.recs + uint64_t(g) * kRecCap;
    uint32_t cursor = 0, anchor = 0, nrec = 0;
    while (cursor < start_lim) {
        // LZ4's acceleration: the further from the last match, the sparser the
        // positions tried (stride 1 + distance / 64), so incompressible data
        // costs a few steps per segment
        const uint32_t stride = 1u + ((cursor - anchor) >> kSkipShift);
        const uint32_t p = cursor + lane * stride;
        const bool valid = p < start_lim;
        const uint32_t v = valid ? lds_rd32(L, p) : 0u;
        const uint32_t h = (v * 2654435761u) >> (32 - kHashBits);
        const uint32_t cand = valid ? L.tab[h] : 0u;
        const uint32_t c = cand ? cand - 1 : 0u;
        const bool ok = valid && cand != 0u && c < p && lds_rd32(L, c) == v;
        const uint64_t m = __ballot(ok);
        __builtin_amdgcn_wave_barrier();
        if (!m) {
            if (valid) L.tab[h] = uint16_t(p + 1);
            cursor += 64 * stride;
            continue;
        }
        const uint32_t f = uint32_t(__ffsll((unsigned long long)m) - 1);
        uint32_t q = cursor + f * stride;
        uint32_t cq = uint32_t(__builtin_amdgcn_readlane(int(c), int(f)));
        uint32_t len = 4;
        // extend backwards over the positions the stride skipped (not past the
        // last match's end nor the candidate's segment start)
        for (;;) {
            const uint32_t room = min(q - anchor, cq);
            if (!room) break;
            const uint32_t k = lane + 1;
            const bool eq = k <= room && lds_rd8(L, q - k) == lds_rd8(L, cq - k);
            const uint64_t mm = __ballot(!eq);
            const uint32_t run = mm ? uint32_t(__ffsll((unsigned long long)mm) - 1) : 64u;
            const uint32_t back = min(run, room);
            q -= back;
            cq -= back;
            len += back;
            if (back < 64) break;
        }
        for (;;) {
            const uint32_t i = q + len + lane;
            const bool eq = i < end_lim && lds_rd8(L, i) == lds_rd8(L, cq + len + lane);
            const uint64_t mm = __ballot(!eq);
            if (!mm) {
                len += 64;
                continue;
            }
            len += uint32_t(__ffsll((unsigned long long)mm) - 1);
            break;
        }
        if (lane == 0) rec[nrec] = make_uint2(q | ((q - cq) << 16), len);
        ++nrec;
        // the window's positions before the next cursor enter the table (later
        // ones are looked up again from there and would only shadow older
        // candidates)
        if (valid && p < q + len) L.tab[h] = uint16_t(p + 1);
        __builtin_amdgcn_wave_barrier();
        anchor = cursor = q + len;
    }
    if (lane == 0) {
        B.nrec[g] = nrec;
        B.trail[g] = n - anchor;
    }
}

__device__ __forceinline__ uint32_t ext_len(uint32_t x) { return x >= 15 ? (x - 15) / 255 + 1 : 0; }

// ---------------------------------------------------------------------------
// k_lz4_size / k_lz4_emit: one workgroup per LZ4 block.  A sequence's literal
// run starts at the previous match's end (or the block start), across segment
// boundaries; the block ends with a literal-only sequence.
// ---------------------------------------------------------------------------
constexpr uint32_t kBlkThreads = 256;
constexpr uint32_t kMaxSegsPerBlk = uint32_t(kBlockLZ / kSegLZ);

struct BlkLds {
    uint32_t rbase[kMaxSegsPerBlk + 1];  // first record index (block-relative) of each segment
    uint32_t prev_end[kMaxSegsPerBlk];   // block-relative end of the last match before each segment
    uint32_t obase[kMaxSegsPerBlk + 1];  // output offset of each segment's first sequence (emit)
    uint32_t acc[kMaxSegsPerBlk];        // per-segment sequence bytes (size)
    uint32_t wsum[3][kBlkThreads / 64];
    uint64_t total;
};

// Block-relative literal start and size of record r of segment s.
__device__ __forceinline__ void rec_geom(const Batch &B, const Blk &K, const BlkLds &L, uint32_t s, uint32_t r,
                                         uint32_t &lit_start, uint32_t &lit_len, uint32_t &mpos, uint32_t &off,
                                         uint32_t &mlen)
{
    const uint2 *rec = B.recs + uint64_t(K.seg0 + s) * kRecCap;
    const uint2 x = rec[r];
    mpos = s * kSegLZ + (x.x & 0xFFFFu);
    off = x.x >> 16;
    mlen = x.y;
    if (r == 0) {
        lit_start = L.prev_end[s];
    } else {
        const uint2 y = rec[r - 1];
        lit_start = s * kSegLZ + (y.x & 0xFFFFu) + y.y;
    }
    lit_len = mpos - lit_start;
}

__device__ __forceinline__ uint32_t seq_size(uint32_t lit_len, uint32_t mlen)
{
    return 1 + ext_len(lit_len) + lit_len + 2 + ext_len(mlen - 4);
}

// Shared prologue: per-segment record bases, the match end before each
// segment and (emit) each segment's output offset: a thread per kPerThr
// consecutive segments, exclusive sum / max scans over the workgroup.
constexpr uint32_t kPerThr = (kMaxSegsPerBlk + kBlkThreads - 1) / kBlkThreads;

__device__ void blk_prologue(const Batch &B, const Blk &K, BlkLds &L, bool with_out)
{
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t nr[kPerThr], en[kPerThr], ob[kPerThr];
    uint32_t c = 0, m = 0, o = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPerThr; ++k) {
        const uint32_t sg = t * kPerThr + k;
        nr[k] = en[k] = ob[k] = 0;
        if (sg < K.nseg) {
            nr[k] = B.nrec[K.seg0 + sg];
            if (nr[k]) {
                const uint2 y = B.recs[uint64_t(K.seg0 + sg) * kRecCap + nr[k] - 1];
                en[k] = sg * kSegLZ + (y.x & 0xFFFFu) + y.y;
            }
            if (with_out) ob[k] = B.seg_out[K.seg0 + sg];
        }
        c += nr[k];
        m = max(m, en[k]);
        o += ob[k];
    }
    // inclusive scans over the wave, then over the waves
    uint32_t ic = c, im = m, io = o;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t yc = __shfl_up(ic, d), ym = __shfl_up(im, d), yo = __shfl_up(io, d);
        if (lane >= d) {
            ic += yc;
            im = max(im, ym);
            io += yo;
        }
    }
    if (lane == 63) {
        L.wsum[0][wv] = ic;
        L.wsum[1][wv] = im;
        L.wsum[2][wv] = io;
    }
    __syncthreads();
    uint32_t bc = 0, bm = 0, bo = 0;
    for (uint32_t i = 0; i < wv; ++i) {
        bc += L.wsum[0][i];
        bm = max(bm, L.wsum[1][i]);
        bo += L.wsum[2][i];
    }
    uint32_t xc = bc + ic - c, xm = max(bm, __shfl_up(im, 1) * (lane ? 1u : 0u)), xo = bo + io - o;  // exclusive
#pragma unroll
    for (uint32_t k = 0; k < kPerThr; ++k) {
        const uint32_t sg = t * kPerThr + k;
        if (sg < K.nseg) {
            L.rbase[sg] = xc;
            L.prev_end[sg] = xm;
            L.obase[sg] = xo;
        }
        xc += nr[k];
        xm = max(xm, en[k]);
        xo += ob[k];
    }
    if (t == kBlkThreads - 1) {
        L.rbase[K.nseg] = xc;
        L.total = xm;  // the last match's end: the final literal run starts here
        L.obase[K.nseg] = xo;
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t seg_of(const BlkLds &L, uint32_t nseg, uint32_t r)
{
    uint32_t lo = 0, hi = nseg;  // last s with rbase[s] <= r
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (L.rbase[mid] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlkThreads) void k_lz4_size(const Batch B)
{
    __shared__ BlkLds L;
    const Blk K = B.blks[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < K.nseg; i += kBlkThreads) L.acc[i] = 0;
    blk_prologue(B, K, L, false);
    const uint32_t nr = L.rbase[K.nseg];
    const uint32_t last_end = uint32_t(L.total);
    for (uint32_t r = threadIdx.x; r < nr; r += kBlkThreads) {
        const uint32_t sg = seg_of(L, K.nseg, r);
        uint32_t ls, ll, mp, off, ml;
        rec_geom(B, K, L, sg, r - L.rbase[sg], ls, ll, mp, off, ml);
        atomicAdd(&L.acc[sg], seq_size(ll, ml));
    }
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t i = threadIdx.x; i < K.nseg; i += kBlkThreads) {
        B.seg_out[K.seg0 + i] = L.acc[i];
        sum += L.acc[i];
    }
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) L.wsum[0][threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (uint32_t i = 0; i < kBlkThreads / 64; ++i) t += L.wsum[0][i];
        const uint32_t fl = K.len - last_end;
        t += 1 + ext_len(fl) + fl;
        B.blk_size[blockIdx.x] = t < K.len ? uint32_t(t) : (K.len | 0x80000000u);
    }
}

// ---------------------------------------------------------------------------
// k_enc_plan: one workgroup of 1,024 threads: per blob its frame size (and the
// offsets of its blocks in the frame), GCM pieces and output size; then
// exclusive scans over the blobs, tile by tile.
// ---------------------------------------------------------------------------
constexpr uint32_t kPlanThreads = 1024;

__global__ __launch_bounds__(kPlanThreads) void k_enc_plan(const Batch B)
{
    __shared__ uint64_t s_o[kPlanThreads / 64];
    __shared__ uint32_t s_p[kPlanThreads / 64];
    __shared__ uint64_t s_carry_o;
    __shared__ uint32_t s_carry_p;
    if (threadIdx.x == 0) B.status[1] = 0;  // k_gcm's piece counter
    if (threadIdx.x == 0) {
        s_carry_o = 0;
        s_carry_p = 0;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t t0 = 0; t0 < B.nblobs; t0 += kPlanThreads) {
        const uint32_t b = t0 + threadIdx.x;
        uint64_t O = 0;
        uint32_t P = 0;
        if (b < B.nblobs) {
            const BlobDesc D = B.blobs[b];
            uint64_t F;
            if (B.compress && D.len == 0) {
                F = 0;  // DeflateStream of empty input is an empty stream (compression/compression.go:58-62)
            } else if (B.compress == 2u) {
                // the member's blocks in order: each span's form is chosen at
                // the bit where the block before it ends (a stored block's
                // padding depends on it)
                uint64_t P = 80;  // after the ten header bytes
                for (uint32_t sp = B.blob_span0[b]; sp < B.blob_span0[b + 1]; ++sp) {
                    SpanOut &o = B.sp[sp];
                    uint64_t bits;
                    o.type = dfl::choose_block(P, B.spans[sp].len, o.fixed_bits, o.dyn_bits, bits);
                    o.bit = P;
                    o.nbits = uint32_t(bits);
                    P += bits;
                }
                F = (P + 7) / 8 + 8;  // CRC-32, ISIZE
            } else if (B.compress) {
                uint64_t off = 7;
                for (uint32_t k = 0; k < D.nblk; ++k) {
                    B.blk_foff[D.blk0 + k] = off;
                    off += 4 + (B.blk_size[D.blk0 + k] & 0x7FFFFFFFu);
                }
                F = off + 4 + 4;  // end mark, content checksum
            } else {
                F = D.len;
            }
            B.frame_len[b] = F;
            P = B.encrypt ? uint32_t((F + kPiece - 1) / kPiece) : 0u;
            O = B.encrypt ? 12 + 48 + F + 28ull * P : F;
        }
        uint64_t xo = O;
        uint32_t xp = P;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t yo = __shfl_up(xo, d);
            const uint32_t yp = __shfl_up(xp, d);
            if (lane >= d) {
                xo += yo;
                xp += yp;
            }
        }
        if (lane == 63) {
            s_o[wv] = xo;
            s_p[wv] = xp;
        }
        __syncthreads();
        uint64_t bo = s_carry_o;
        uint32_t bp = s_carry_p;
        for (uint32_t i = 0; i < wv; ++i) {
            bo += s_o[i];
            bp += s_p[i];
        }
        if (b < B.nblobs) {
            B.out_off[b] = bo + xo - O;
            B.piece_base[b] = bp + xp - P;
        }
        __syncthreads();
        if (threadIdx.x == kPlanThreads - 1) {
            uint64_t to = 0;
            uint32_t tp = 0;
            for (uint32_t i = 0; i < kPlanThreads / 64; ++i) {
                to += s_o[i];
                tp += s_p[i];
            }
            s_carry_o += to;
            s_carry_p += tp;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        B.out_off[B.nblobs] = s_carry_o;
        B.piece_base[B.nblobs] = s_carry_p;
        B.status[0] = s_carry_o > B.out_cap ? uint64_t(uint32_t(CDC_E_NOSPACE)) : 0ull;
    }
}

// Where the LZ4 stages write blob b's frame: the frame buffer when it is
// encrypted next, else its place in the output.
__device__ __forceinline__ uint8_t *frame_ptr(const Batch &B, uint32_t b)
{
    return B.encrypt ? B.frames + B.blobs[b].slot : B.out + B.out_off[b];
}

// The plaintext the GCM stage seals: the frame, or the blob itself uncompressed.
__device__ __forceinline__ const uint8_t *plain_ptr(const Batch &B, uint32_t b)
{
    return B.compress ? B.frames + B.blobs[b].slot : B.base + B.blobs[b].src;
}

// Neither compressed nor encrypted: the output is the blob (Encode with no
// compression and no key configured).
__global__ __launch_bounds__(256) void k_copy(const Batch B)
{
    const uint32_t b = blockIdx.x;
    if (b >= B.nblobs || B.status[0]) return;
    copy_span(B.out + B.out_off[b], B.base + B.blobs[b].src, B.blobs[b].len, threadIdx.x, blockDim.x);
}

// Grid (blocks, kEmitSplit): a stored block is copied by all its kEmitSplit
// workgroups, a compressed one written by segment ranges, one per workgroup
// (its output offset from k_lz4_size's per-segment sizes).
constexpr uint32_t kEmitSplit = 16;

__global__ __launch_bounds__(kBlkThreads) void k_lz4_emit(const Batch B)
{
    __shared__ BlkLds L;
    if (B.status[0]) return;
    const Blk K = B.blks[blockIdx.x];
    uint8_t *dst = frame_ptr(B, K.blob) + B.blk_foff[blockIdx.x];
    const uint8_t *src = B.base + K.src;
    const uint32_t bs = B.blk_size[blockIdx.x];
    if (threadIdx.x == 0 && blockIdx.y == 0) {
        dst[0] = uint8_t(bs);
        dst[1] = uint8_t(bs >> 8);
        dst[2] = uint8_t(bs >> 16);
        dst[3] = uint8_t(bs >> 24);
    }
    dst += 4;
    if (bs & 0x80000000u) {  // stored: the raw bytes, a slice per workgroup
        const uint32_t a = uint32_t(uint64_t(K.len) * blockIdx.y / kEmitSplit);
        const uint32_t e = uint32_t(uint64_t(K.len) * (blockIdx.y + 1) / kEmitSplit);
        copy_span(dst + a, src + a, e - a, threadIdx.x, kBlkThreads);
        return;
    }
    // compressed: workgroup y writes the sequences of segments [sa, sb)
    blk_prologue(B, K, L, true);
    const uint32_t sa = K.nseg * blockIdx.y / kEmitSplit, sb = K.nseg * (blockIdx.y + 1) / kEmitSplit;
    const uint32_t r0 = L.rbase[sa], r1 = L.rbase[sb];
    const uint32_t last_end = uint32_t(L.total);
    // tiles of kBlkThreads records: sizes, workgroup-wide exclusive scan, write
    __shared__ uint32_t s_part[kBlkThreads / 64];
    uint32_t carry = L.obase[sa];
    for (uint32_t t0 = r0; t0 < r1; t0 += kBlkThreads) {
        const uint32_t r = t0 + threadIdx.x;
        uint32_t ls = 0, ll = 0, mp = 0, off = 0, ml = 0, sz = 0;
        if (r < r1) {
            const uint32_t sg = seg_of(L, K.nseg, r);
            rec_geom(B, K, L, sg, r - L.rbase[sg], ls, ll, mp, off, ml);
            sz = seq_size(ll, ml);
        }
        uint32_t x = sz;
        const uint32_t lane = threadIdx.x & 63u;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_part[threadIdx.x >> 6] = x;
        __syncthreads();
        uint32_t wbase = 0;
        for (uint32_t i = 0; i < (threadIdx.x >> 6); ++i) wbase += s_part[i];
        uint32_t tile_total = 0;
        for (uint32_t i = 0; i < kBlkThreads / 64; ++i) tile_total += s_part[i];
        __syncthreads();
        if (r < r1) {
            uint8_t *o = dst + carry + wbase + x - sz;
            const uint32_t lt = ll >= 15 ? 15 : ll, mt = ml - 4 >= 15 ? 15 : ml - 4;
            *o++ = uint8_t(lt << 4 | mt);
            if (ll >= 15) {
                uint32_t e = ll - 15;
                for (; e >= 255; e -= 255) *o++ = 255;
                *o++ = uint8_t(e);
            }
            for (uint32_t i = 0; i < ll; ++i) o[i] = src[ls + i];
            o += ll;
            *o++ = uint8_t(off);
            *o++ = uint8_t(off >> 8);
            if (ml - 4 >= 15) {
                uint32_t e = ml - 4 - 15;
                for (; e >= 255; e -= 255) *o++ = 255;
                *o++ = uint8_t(e);
            }
        }
        carry += tile_total;
    }
    if (threadIdx.x == 0 && sb == K.nseg) {  // the final literal-only sequence
        uint8_t *o = dst + L.obase[K.nseg];
        const uint32_t ll = K.len - last_end;
        *o++ = uint8_t((ll >= 15 ? 15 : ll) << 4);
        if (ll >= 15) {
            uint32_t e = ll - 15;
            for (; e >= 255; e -= 255) *o++ = 255;
            *o++ = uint8_t(e);
        }
        for (uint32_t i = 0; i < ll; ++i) o[i] = src[last_end + i];
    }
}

// Frame header (pierrec/lz4 v4 defaults: version 1, independent blocks,
// content checksum, 4-MiB blocks), end mark and checksum.
__device__ uint32_t xxh32_small(const uint8_t *p, uint32_t n)
{
    uint32_t h = P5 + n;
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4) h = rol32(h + ld32u(p + i) * P3, 17) * P4;
    for (; i < n; ++i) h = rol32(h + p[i] * P5, 11) * P1;
    h ^= h >> 15;
    h *= P2;
    h ^= h >> 13;
    h *= P3;
    h ^= h >> 16;
    return h;
}

__global__ __launch_bounds__(64) void k_frame_fin(const Batch B)
{
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B.nblobs || B.status[0] || B.frame_len[b] == 0) return;  // empty blob: no frame at all
    uint8_t *f = frame_ptr(B, b);
    const uint8_t hdr[6] = {0x04, 0x22, 0x4D, 0x18, 0x64, 0x70};
    for (int i = 0; i < 6; ++i) f[i] = hdr[i];
    f[6] = uint8_t(xxh32_small(hdr + 4, 2) >> 8);
    const uint64_t F = B.frame_len[b];
    uint8_t *e = f + F - 8;
    e[0] = e[1] = e[2] = e[3] = 0;
    const uint32_t x = B.xxh[b];
    e[4] = uint8_t(x);
    e[5] = uint8_t(x >> 8);
    e[6] = uint8_t(x >> 16);
    e[7] = uint8_t(x >> 24);
}

// ---------------------------------------------------------------------------
// GCM
// ---------------------------------------------------------------------------
// Key setup, in two kernels.  k_blob_keys: one thread per blob (the AES
// tables and the repository key's schedule, H and 4-bit table in LDS, shared
// by the workgroup): the subkey's round keys, H = AES_K(0) and its 4-bit
// table, and the stream header (subkey nonce || Seal(repository key, subkey
// nonce, subkey)).  k_blob_pows: one wave per blob: H^1..H^64 by a doubling
// ladder (round k: lanes [2^k, 2^(k+1)) multiply H^(lane + 1 - 2^k) by H^(2^k)
// with its 4-bit table, built by 16 lanes), then four entries per lane of the
// 8-bit table of H^64 from its eight halvings.
constexpr uint32_t kKeyThreads = 256;
constexpr uint32_t kPowWaves = 4;

__global__ __launch_bounds__(kKeyThreads) void k_blob_keys(const Batch B)
{
    __shared__ uint32_t s_te[256];
    __shared__ uint8_t s_sb[256];
    __shared__ uint32_t s_mrk[60];
    __shared__ G128 s_mth[16];
    const uint32_t t = threadIdx.x;
    s_te[t] = g_te0[t];
    s_sb[t] = g_sbox[t];
    __syncthreads();
    if (t == 0) {  // the repository key: schedule, H and its table
        uint8_t key[32];
        for (int i = 0; i < 32; ++i) key[i] = B.key[i];
        uint32_t mk[60];
        aes256_expand(key, mk, s_sb);
        for (int i = 0; i < 60; ++i) s_mrk[i] = mk[i];
        uint32_t z[4] = {0, 0, 0, 0};
        aes256_block(mk, s_te, s_sb, z);
        G128 th[16];
        gtable(g_from_words(z), th);
        for (int i = 0; i < 16; ++i) s_mth[i] = th[i];
    }
    __syncthreads();
    const uint32_t b = blockIdx.x * kKeyThreads + t;
    if (b >= B.nblobs || B.status[0]) return;
    const uint8_t *r = B.rnd + 56ull * b;  // subkey 32, subkey nonce 12, data nonce 12
    BlobKey &K = B.keys[b];
    {
        uint32_t rk[60];
        aes256_expand(r, rk, s_sb);
        for (int i = 0; i < 60; ++i) K.rk[i] = rk[i];
        uint32_t z[4] = {0, 0, 0, 0};
        aes256_block(rk, s_te, s_sb, z);
        const G128 H = g_from_words(z);
        K.hpow[0] = H;
        G128 th[16];
        gtable(H, th);
        for (int i = 0; i < 16; ++i) K.th[i] = th[i];
    }
    // header: subkey nonce || Seal(repository key, subkey nonce, subkey)
    uint8_t *o = B.out + B.out_off[b];
    for (int i = 0; i < 12; ++i) o[i] = r[32 + i];
    const uint8_t *nonce = r + 32;
    uint32_t j0[3];
    j0[0] = uint32_t(nonce[0]) << 24 | uint32_t(nonce[1]) << 16 | uint32_t(nonce[2]) << 8 | nonce[3];
    j0[1] = uint32_t(nonce[4]) << 24 | uint32_t(nonce[5]) << 16 | uint32_t(nonce[6]) << 8 | nonce[7];
    j0[2] = uint32_t(nonce[8]) << 24 | uint32_t(nonce[9]) << 16 | uint32_t(nonce[10]) << 8 | nonce[11];
    G128 S = {0, 0};
    for (uint32_t i = 0; i < 2; ++i) {
        uint32_t c[4] = {j0[0], j0[1], j0[2], 2 + i};
        aes256_block(s_mrk, s_te, s_sb, c);
        uint32_t p[4];
        gcm_block_words(r + 16 * i, p);
        for (int k = 0; k < 4; ++k) {
            c[k] ^= p[k];
            o[12 + 16 * i + 4 * k] = uint8_t(c[k] >> 24);
            o[12 + 16 * i + 4 * k + 1] = uint8_t(c[k] >> 16);
            o[12 + 16 * i + 4 * k + 2] = uint8_t(c[k] >> 8);
            o[12 + 16 * i + 4 * k + 3] = uint8_t(c[k]);
        }
        S = gmul4(gx(S, g_from_words(c)), s_mth);
    }
    S = gmul4(gx(S, G128{0, 256}), s_mth);  // len(A) = 0, len(C) = 256 bits
    uint32_t tg[4] = {j0[0], j0[1], j0[2], 1};
    aes256_block(s_mrk, s_te, s_sb, tg);
    const uint64_t hi = S.hi ^ (uint64_t(tg[0]) << 32 | tg[1]), lo = S.lo ^ (uint64_t(tg[2]) << 32 | tg[3]);
    for (int k = 0; k < 8; ++k) {
        o[44 + k] = uint8_t(hi >> (56 - 8 * k));
        o[52 + k] = uint8_t(lo >> (56 - 8 * k));
    }
}

__global__ __launch_bounds__(kPowWaves * 64) void k_blob_pows(const Batch B)
{
    __shared__ PowLds S[kPowWaves];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPowWaves + wv;
    if (b >= B.nblobs || B.status[0]) return;
    hpow_ladder(B.keys[b], S[wv], lane);
}

__global__ __launch_bounds__(kGcmWaves * 64) void k_gcm(const Batch B)
{
    __shared__ GcmLds L;
    for (uint32_t i = threadIdx.x; i < 256 * 64; i += blockDim.x)
        L.te[i] = (i & 32u) ? ror32(g_te0[i >> 6], 8) : g_te0[i >> 6];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, laneoff = (lane & 31u) << 2;
    const char *te = reinterpret_cast<const char *>(L.te);
    __syncthreads();
    // Persistent: one workgroup per CU; each wave takes pieces from a counter
    // (B.status[1], zeroed by k_enc_plan) until none is left, so the last
    // round of pieces does not leave most CUs idle.
    const uint32_t total = B.piece_base[B.nblobs];
    if (B.status[0]) return;
    for (;;) {
    // every lane in the atomic (lane 0 adds 1): no lane-0 branch before the
    // readfirstlane, which the compiler could thread apart (cdc_kernels.hip wave_ticket)
    uint32_t pc = atomicAdd(reinterpret_cast<uint32_t *>(&B.status[1]), lane == 0 ? 1u : 0u);
    pc = uint32_t(__builtin_amdgcn_readfirstlane(int(pc)));
    if (pc >= total) break;
    uint32_t b;
    {
        uint32_t lo = 0, hi = B.nblobs;  // last blob with piece_base <= pc
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (B.piece_base[mid] <= pc) lo = mid;
            else hi = mid;
        }
        b = lo;
        const BlobKey &K = B.keys[b];
        // this wave's tables (the previous piece's reads of them are done: the
        // wave barrier at the end of its loop body)
        for (uint32_t i = lane; i < 60; i += 64) L.w[wv].rk[i] = K.rk[i];
        for (uint32_t i = lane; i < 60; i += 64) L.w[wv].rk16[i] = ror32(K.rk[i], 16);
        if (lane < 16) L.w[wv].th[lane] = K.th[lane];
        for (uint32_t i = lane; i < 256; i += 64) L.w[wv].t64[i] = K.t64[i];
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
    }
    const BlobKey &K = B.keys[b];
    const uint32_t k = pc - B.piece_base[b];
    const uint64_t F = B.frame_len[b];
    const uint64_t p0 = uint64_t(k) * kPiece;
    const uint32_t m = uint32_t(min<uint64_t>(kPiece, F - p0));  // piece bytes
    const uint32_t nb = (m + 15) / 16;
    const gu8 *pt = reinterpret_cast<const gu8 *>(reinterpret_cast<uintptr_t>(plain_ptr(B, b) + p0));
    const uint32_t pt_sh = uint32_t(reinterpret_cast<uintptr_t>(pt) & 3u);
    uint8_t *o = B.out + B.out_off[b] + 60 + uint64_t(k) * (kPiece + 28);
    const uint8_t *dn = B.rnd + 56ull * b + 44;  // data nonce
    uint32_t j0[3];
    j0[0] = uint32_t(dn[0]) << 24 | uint32_t(dn[1]) << 16 | uint32_t(dn[2]) << 8 | dn[3];
    j0[1] = uint32_t(dn[4]) << 24 | uint32_t(dn[5]) << 16 | uint32_t(dn[6]) << 8 | dn[7];
    j0[2] = (uint32_t(dn[8]) << 24 | uint32_t(dn[9]) << 16 | uint32_t(dn[10]) << 8 | dn[11]) ^ k;
    if (lane < 12) o[lane] = uint8_t(j0[lane >> 2] >> (24 - 8 * (lane & 3)));
    uint8_t *ct = o + 12;
    const CtrPre cpre = ctr_pre(L.w[wv], te, laneoff, j0);
    const G128 *t64 = L.w[wv].t64;
    uint8_t *stage = reinterpret_cast<uint8_t *>(L.w[wv].stage);
    // The piece's plaintext as dwords from its aligned-down start (block i:
    // dwords 4 i .. 4 i + 4, funnel-shifted by its offset in a dword).  A raw
    // buffer returns 0 past its last dword, so every lane loads without a
    // lane condition and a step's loads go out before its AES, which hides
    // their latency (loads under a lane condition were waited for at once).
    const uint32_t lastq = (pt_sh + m - 1) >> 2;
    const __amdgpu_buffer_rsrc_t prs = gcm_rsrc(reinterpret_cast<uintptr_t>(pt) - pt_sh, uint64_t(lastq + 1) * 4);
    const bool pt_fast = pt_sh == 0 && (m & 15u) == 0;  // whole aligned blocks: one 16-byte load each
    // row j: blocks 64 j + lane (1 KiB of the piece), two rows per step (their
    // AES interleaved); lane: Horner in H^64 over its blocks, in order
    G128 Z = {0, 0};
    uint32_t cnt = 0;
    const uint32_t rows = (nb + 63) / 64;
    for (uint32_t j = 0; j < rows; j += kGcmRows) {
        uint32_t c[kGcmRows][4];
#pragma unroll
        for (int u = 0; u < int(kGcmRows); ++u) {
            c[u][0] = j0[0];
            c[u][1] = j0[1];
            c[u][2] = j0[2];
            c[u][3] = 2 + 64 * (j + u) + lane;
        }
        uint32_t px[kGcmRows][5];
#pragma unroll
        for (int u = 0; u < int(kGcmRows); ++u) {
            const int32_t i = int32_t(64 * (j + u) + lane);
            if (pt_fast) {
                const uint4 v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(prs, 16 * i, 0, 0));
                px[u][0] = v.x;
                px[u][1] = v.y;
                px[u][2] = v.z;
                px[u][3] = v.w;
                px[u][4] = 0;
            } else {
                // dword by dword, clamped to the last one (a wide load that
                // straddles the buffer's end may read as wholly out of range)
#pragma unroll
                for (int q = 0; q < 5; ++q)
                    px[u][q] = __builtin_amdgcn_raw_buffer_load_b32(prs, int32_t(4 * min(uint32_t(4 * i + q), lastq)), 0, 0);
            }
        }
#ifndef GCM_DIAG_NO_AES  // build-time diagnostic only: no keystream (timing only)
        {
            uint32_t ctr[kGcmRows];
#pragma unroll
            for (uint32_t u = 0; u < kGcmRows; ++u) ctr[u] = c[u][3];
            aes256_ctr_lds<kGcmRows>(L.w[wv], te, laneoff, cpre, ctr, c);
        }
#endif
#pragma unroll
        for (int u = 0; u < int(kGcmRows); ++u) {
            const uint32_t i = 64 * (j + u) + lane;
            uint4 cw = make_uint4(0, 0, 0, 0);
            if (i < nb) {
                const uint32_t bytes = min(16u, m - 16 * i);
                uint32_t pw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) pw[q] = be32(__builtin_amdgcn_alignbit(px[u][q + 1], px[u][q], 8 * pt_sh));
                uint32_t w[4];
                for (int q = 0; q < 4; ++q) w[q] = c[u][q] ^ pw[q];
                if (bytes < 16) {  // the keystream past the piece's end is not ciphertext (nor hashed)
                    for (int q = 0; q < 4; ++q) {
                        const int keep = int(bytes) - 4 * q;
                        w[q] = keep >= 4 ? w[q] : keep <= 0 ? 0u : (w[q] & ~(0xFFFFFFFFu >> (8 * keep)));
                    }
                }
                cw = make_uint4(be32(w[0]), be32(w[1]), be32(w[2]), be32(w[3]));
#ifdef GCM_DIAG_NO_GHASH  // build-time diagnostic only: no multiply by H^64 (timing only)
                Z = gx(Z, G128{uint64_t(w[0]) << 32 | w[1], uint64_t(w[2]) << 32 | w[3]});
#else
                Z = gx(gmul8(Z, t64), G128{uint64_t(w[0]) << 32 | w[1], uint64_t(w[2]) << 32 | w[3]});
#endif
                ++cnt;
            }
            L.w[wv].stage[64 * u + lane] = cw;
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t row_bytes = min(1024u * kGcmRows, m - 1024 * j);
        // the rows' ciphertext through LDS: the bytes up to the first aligned
        // dword of the destination, then 8 coalesced dword stores (each dword
        // funnel-shifted from two of the stage's), then the last 0-3 bytes
        {
            uint8_t *dst = ct + 1024 * j;
            const uint32_t hb = min((4u - uint32_t(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u, row_bytes);
            const uint32_t nd = (row_bytes - hb) >> 2, tb = row_bytes - hb - 4 * nd;
            const uint32_t *sw = reinterpret_cast<const uint32_t *>(stage);
            uint32_t *dw = reinterpret_cast<uint32_t *>(dst + hb);
#pragma unroll
            for (uint32_t q = 0; q < 4 * kGcmRows; ++q) {
                const uint32_t d = 64 * q + lane;
                if (d < nd) dw[d] = __builtin_amdgcn_alignbit(sw[min(d + 1, 256u * kGcmRows - 1)], sw[d], 8 * hb);
            }
            if (lane < hb) dst[lane] = stage[lane];
            if (lane < tb) dst[hb + 4 * nd + lane] = stage[hb + 4 * nd + lane];
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (cnt) {
        const uint32_t e = nb - lane - 64 * (cnt - 1);  // 1..64
        Z = gmul_bits(Z, K.hpow[e - 1]);
    }
    for (int off = 32; off; off >>= 1) {
        Z.hi ^= __shfl_xor(Z.hi, off);
        Z.lo ^= __shfl_xor(Z.lo, off);
    }
    if (lane == 0) {
        G128 S = gmul4(gx(Z, G128{0, uint64_t(m) * 8}), L.w[wv].th);
        uint32_t t[1][4] = {{j0[0], j0[1], j0[2], 1}};
        aes256_blocks_lds<1>(L.w[wv], te, laneoff, t);
        const uint64_t hi = S.hi ^ (uint64_t(t[0][0]) << 32 | t[0][1]), lo = S.lo ^ (uint64_t(t[0][2]) << 32 | t[0][3]);
        uint8_t *tag = ct + m;
        for (int q = 0; q < 8; ++q) {
            tag[q] = uint8_t(hi >> (56 - 8 * q));
            tag[8 + q] = uint8_t(lo >> (56 - 8 * q));
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// GZIP: DEFLATE over k_lz4_seq's records (deflate_enc.h has every rule), one
// workgroup per span, lane t the span's stretch t.  These kernels stand after
// the GCM kernels on purpose: in front of them they moved k_gcm's code in the
// code object and its time on C3 went from 224 to 259 us, the same
// instructions.
// ---------------------------------------------------------------------------

struct WgPar {
    uint32_t lane;
    static constexpr uint32_t nl = kDflThreads;
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    __device__ __forceinline__ void bor(uint32_t *p, uint32_t v) { atomicOr(p, v); }
};

struct LdsRd {  // the span's bytes in LDS
    const uint32_t *w;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (w[i >> 2] >> ((i & 3u) * 8u)) & 255u; }
};

// The span into LDS, 16 bytes per lane and load (unaligned global loads); the
// last partial 16 bytes from byte loads, zero-filled.  Nothing past src + n is read.
__device__ void load_span(uint32_t *data, const uint8_t *src, uint32_t n)
{
    for (uint32_t i = threadIdx.x; i < (n + 15) / 16; i += kDflThreads) {
        const uint32_t p = 16 * i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p + 16 <= n) {
            __builtin_memcpy(&v, src + p, 16);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t b = 0; p + b < n; ++b) w[b >> 2] |= uint32_t(src[p + b]) << (8 * (b & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(&data[4 * i]) = v;
    }
}

__device__ __forceinline__ dfl::SpanView span_view(const Batch &B, const Span &S)
{
    dfl::SpanView V;
    for (uint32_t g = 0; g < dfl::kSpanSegs; ++g) {
        const bool in = g < S.nseg;
        V.rec[g] = reinterpret_cast<const dfl::Rec *>(B.recs + uint64_t(S.seg0 + (in ? g : 0u)) * kRecCap);
        V.nrec[g] = in ? B.nrec[S.seg0 + g] : 0u;
        V.hist[g] = in ? uint32_t(B.segs[S.seg0 + g].hist) : 0u;
    }
    V.len = S.len;
    return V;
}

struct alignas(16) DflSizeLds {
    uint32_t data[dfl::kSpan / 4];
    uint32_t lfreq[dfl::kLitSlots], dfreq[dfl::kDistSlots];
    uint32_t xbits;
    uint32_t crc[kDflThreads / 64];
    uint32_t hdr[dfl::kHdrWords];
    uint8_t llen[dfl::kLitSlots], dlen[dfl::kDistSlots];
    dfl::CodeWork W;
    dfl::HdrWork H;
};

__global__ __launch_bounds__(kDflThreads) void k_dfl_size(const Batch B)
{
    __shared__ DflSizeLds L;
    const uint32_t t = threadIdx.x, sid = blockIdx.x;
    const Span S = B.spans[sid];
    WgPar par{t};
    for (uint32_t i = t; i < dfl::kLitSlots; i += kDflThreads) {
        L.lfreq[i] = 0;
        L.llen[i] = 0;
    }
    if (t < dfl::kDistSlots) {
        L.dfreq[t] = 0;
        L.dlen[t] = 0;
    }
    if (t < dfl::kHdrWords) L.hdr[t] = 0;
    if (t == 0) L.xbits = 0;
    load_span(L.data, B.base + S.src, S.len);
    __syncthreads();
    const dfl::SpanView V = span_view(B, S);
    LdsRd rd{L.data};
    dfl::span_hist(par, V, rd, L.lfreq, L.dfreq, &L.xbits);
    // CRC-32: each lane its stretch from a zero register, moved to the span's
    // end by x^(8 * bytes after it); the span's register is their sum
    {
        const uint32_t a = min(t * dfl::kStretch, S.len), e = min(a + dfl::kStretch, S.len);
        uint32_t r = 0;
        for (uint32_t i = a; i < e; ++i) r = infw::crc_bits(r, rd(i));
        if (r) r = infw::crc_mul(r, infw::crc_shift(S.len - e));
        for (int o = 32; o; o >>= 1) r ^= __shfl_xor(r, o);
        if ((t & 63u) == 0) L.crc[t >> 6] = r;
    }
    dfl::build_lengths(par, L.lfreq, dfl::kNLit, 15, L.llen, L.W);
    dfl::build_lengths(par, L.dfreq, dfl::kNDist, 15, L.dlen, L.W);
    if (t == 0) dfl::header_tokens(L.llen, L.dlen, L.H);
    dfl::build_lengths(par, L.H.clfreq, dfl::kNCl, 7, L.H.cllen, L.W);
    dfl::assign_codes(par, L.H.cllen, dfl::kNCl, L.H.clcode);
    if (t == 0) {
        SpanOut o{};
        o.hdr_bits = dfl::write_header(L.H, L.hdr);
        o.dyn_bits = 3 + o.hdr_bits + dfl::body_bits(L.lfreq, L.dfreq, L.llen, L.dlen, L.xbits);
        o.fixed_bits = 3 + dfl::body_bits(L.lfreq, L.dfreq, nullptr, nullptr, L.xbits);
        uint32_t c = 0;
        for (uint32_t i = 0; i < kDflThreads / 64; ++i) c ^= L.crc[i];
        o.crc = c;
        B.sp[sid] = o;
    }
    __syncthreads();
    uint8_t *lens = B.sp_lens + uint64_t(sid) * kSpanLens;
    for (uint32_t i = t; i < dfl::kLitSlots; i += kDflThreads) lens[i] = L.llen[i];
    if (t < dfl::kDistSlots) lens[dfl::kLitSlots + t] = L.dlen[t];
    if (t < dfl::kHdrWords) B.sp_hdr[uint64_t(sid) * dfl::kHdrWords + t] = L.hdr[t];
}

struct alignas(16) DflEmitLds {
    uint32_t data[dfl::kSpan / 4];
    uint32_t out[dfl::kSpan / 4 + 8];  // the block from bit (start & 7): at most 8 * len + 42 + 7 bits, and a word to look ahead
    uint32_t sbits[dfl::kStretches];
    uint32_t hdr[dfl::kHdrWords];
    uint8_t lens[kSpanLens];
    dfl::Codes C;
};

__global__ __launch_bounds__(kDflThreads) void k_dfl_emit(const Batch B)
{
    __shared__ DflEmitLds L;
    if (B.status[0]) return;
    const uint32_t t = threadIdx.x, sid = blockIdx.x;
    const Span S = B.spans[sid];
    const SpanOut O = B.sp[sid];
    uint8_t *dst = frame_ptr(B, S.blob);
    const uint32_t sh = uint32_t(O.bit & 7u);
    const uint64_t g = O.bit >> 3;  // the member's byte that holds the block's first bit
    if (O.type == dfl::kStored) {
        // 3 header bits at the running position, zeros to the byte boundary, LEN, NLEN, the bytes
        const uint64_t A = (O.bit + 3 + 7) >> 3;
        if (t == 0) {
            const uint32_t h = S.last ? 1u : 0u;
            if (sh == 0) dst[g] = uint8_t(h);
            if (sh > 5) dst[g + 1] = uint8_t(h >> (8 - sh));
            B.sp[sid].edge_lo = sh ? (h << sh) & 255u : 0u;
            B.sp[sid].edge_hi = 0;
            dst[A] = uint8_t(S.len);
            dst[A + 1] = uint8_t(S.len >> 8);
            dst[A + 2] = uint8_t(~S.len);
            dst[A + 3] = uint8_t(~S.len >> 8);
        }
        copy_span(dst + A + 4, B.base + S.src, S.len, t, kDflThreads);
        return;
    }
    WgPar par{t};
    const bool dyn = O.type == dfl::kDynamic;
    for (uint32_t i = t; i < dfl::kSpan / 4 + 8; i += kDflThreads) L.out[i] = 0;
    load_span(L.data, B.base + S.src, S.len);
    if (dyn) {
        for (uint32_t i = t; i < kSpanLens; i += kDflThreads) L.lens[i] = B.sp_lens[uint64_t(sid) * kSpanLens + i];
        if (t < dfl::kHdrWords) L.hdr[t] = B.sp_hdr[uint64_t(sid) * dfl::kHdrWords + t];
    }
    dfl::load_codes(par, L.C, dyn ? L.lens : nullptr, dyn ? L.lens + dfl::kLitSlots : nullptr);
    const dfl::SpanView V = span_view(B, S);
    LdsRd rd{L.data};
    dfl::span_count(par, V, rd, L.C, L.sbits);
    const uint64_t end = dfl::span_pack(par, V, rd, L.C, L.sbits, O.type, S.last != 0, L.hdr, O.hdr_bits, L.out, sh);
    // whole bytes out; the first and the last byte, where a neighbour's bits
    // share them, go to k_gz_fin as edges
    const uint32_t eb = uint32_t(end), j0 = sh ? 1u : 0u, j1 = eb >> 3;
    if (t == 0) {
        B.sp[sid].edge_lo = sh ? L.out[0] & 255u : 0u;
        B.sp[sid].edge_hi = (eb & 7u) ? (L.out[j1 >> 2] >> ((j1 & 3u) * 8u)) & 255u : 0u;
    }
    if (eb != sh + O.nbits || j1 <= j0) return;  // the plan and the packing disagree (a bug): the CRC-32 will say so
    {
        uint8_t *o = dst + g + j0;
        const uint32_t n = j1 - j0;
        const uint32_t head = min((4u - uint32_t(reinterpret_cast<uintptr_t>(o) & 3u)) & 3u, n);
        const uint32_t nd = (n - head) >> 2, tail = n - head - 4 * nd;
        if (t < head) o[t] = uint8_t((L.out[(j0 + t) >> 2] >> (((j0 + t) & 3u) * 8u)) & 255u);
        uint32_t *ow = reinterpret_cast<uint32_t *>(o + head);
        for (uint32_t d = t; d < nd; d += kDflThreads) {
            const uint32_t so = j0 + head + 4 * d;
            ow[d] = __builtin_amdgcn_alignbit(L.out[(so >> 2) + 1], L.out[so >> 2], (so & 3u) * 8u);
        }
        if (t < tail) {
            const uint32_t so = j0 + head + 4 * nd + t;
            o[head + 4 * nd + t] = uint8_t((L.out[so >> 2] >> ((so & 3u) * 8u)) & 255u);
        }
    }
}

// One wave per blob: the ten header bytes of Go's gzip.NewWriter (no flags,
// MTIME 0, XFL 0, OS 255), the bytes that two spans' blocks share, CRC-32 and ISIZE.
__global__ __launch_bounds__(64) void k_gz_fin(const Batch B)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (B.status[0] || B.frame_len[b] == 0) return;  // empty blob: an empty stream
    uint8_t *f = frame_ptr(B, b);
    const uint64_t len = B.blobs[b].len;
    const uint32_t s0 = B.blob_span0[b], n = B.blob_span0[b + 1] - s0;
    if (lane < 10) f[lane] = lane == 0 ? 0x1F : lane == 1 ? 0x8B : lane == 2 ? 8 : lane == 9 ? 0xFF : 0;
    uint32_t acc = 0;
    for (uint32_t k = lane; k < n; k += 64) {
        const SpanOut &o = B.sp[s0 + k];
        const uint64_t done = min<uint64_t>(len, uint64_t(k + 1) * dfl::kSpan);
        acc ^= infw::crc_mul(o.crc, infw::crc_shift(len - done));
        if (k && (o.bit & 7u)) f[o.bit >> 3] = uint8_t(B.sp[s0 + k - 1].edge_hi | o.edge_lo);
    }
    for (int o = 32; o; o >>= 1) acc ^= __shfl_xor(acc, o);
    if (lane == 0) {
        // the register started from 0xFFFFFFFF, not 0: that start moved past len bytes
        const uint32_t crc = ~(acc ^ infw::crc_mul(0xFFFFFFFFu, infw::crc_shift(len)));
        const SpanOut &o = B.sp[s0 + n - 1];
        const uint64_t E = o.bit + o.nbits;
        if (E & 7u) f[E >> 3] = uint8_t(o.edge_hi);
        uint8_t *e = f + ((E + 7) >> 3);
        for (int i = 0; i < 4; ++i) {
            e[i] = uint8_t(crc >> (8 * i));
            e[4 + i] = uint8_t(uint32_t(len) >> (8 * i));
        }
    }
}

// ---------------------------------------------------------------------------
// The stream form (cdc_gzip_stream_piece): one member out of many pieces.  A
// piece is planned as one blob of a GZIP batch (k_lz4_seq, k_dfl_size and
// k_dfl_emit run unchanged, no span marked last), with these two kernels in
// the place of k_enc_plan and k_gz_fin.  They stand behind the GCM kernels
// like the other DEFLATE kernels.
// ---------------------------------------------------------------------------
struct StreamArgs {
    uint32_t first, last;  // the member's first piece (header), its last (final block, CRC-32, ISIZE)
    uint32_t reg;          // CRC-32 register over the stream before this piece, from 0xFFFFFFFF
    uint32_t isize;        // the stream's length with this piece, mod 2^32
    uint64_t *res;         // [0]: the piece's output bytes; [1]: its CRC-32 register from 0
};

// One wave: each span's form at the bit where the block before it ended.  The
// lanes load 64 spans' sizes at a time; the chain over them runs in registers,
// alike in every lane, and lane j keeps span j's result.
__global__ __launch_bounds__(64) void k_gzs_plan(const Batch B, const StreamArgs A)
{
    const uint32_t lane = threadIdx.x;
    uint64_t P = A.first ? 80 : 0;
    for (uint32_t s0 = 0; s0 < B.nspans; s0 += 64) {
        const uint32_t sp = s0 + lane;
        const bool in = sp < B.nspans;
        const uint32_t len = in ? B.spans[sp].len : 0u;
        const uint32_t fb = in ? B.sp[sp].fixed_bits : 0u, db = in ? B.sp[sp].dyn_bits : 0u;
        uint32_t ty = 0, nb = 0;
        uint64_t at = 0;
        const uint32_t cnt = min(64u, B.nspans - s0);
        for (uint32_t j = 0; j < cnt; ++j) {
            uint64_t bits;
            const uint32_t t = dfl::choose_block(P, uint32_t(__shfl(int(len), int(j))), uint32_t(__shfl(int(fb), int(j))),
                                                 uint32_t(__shfl(int(db), int(j))), bits);
            if (lane == j) {
                ty = t;
                nb = uint32_t(bits);
                at = P;
            }
            P += bits;
        }
        if (in) {
            SpanOut &o = B.sp[sp];
            o.type = ty;
            o.nbits = nb;
            o.bit = at;
        }
    }
    if (lane == 0) {
        P += dfl::joiner_bits(P);
        const uint64_t F = P / 8 + (A.last ? dfl::kFinalBytes + 8 : 0);
        B.frame_len[0] = F;
        B.out_off[0] = 0;
        B.out_off[1] = F;
        B.status[0] = F > B.out_cap ? uint64_t(uint32_t(CDC_E_NOSPACE)) : 0ull;
        B.status[1] = 0;
        A.res[0] = F;
        A.res[1] = 0;
    }
}

// One wave: the header (first piece), the bytes two spans' blocks share, the
// joiner, the piece's CRC-32 register for the host's running one and, on the
// last piece, the final block, the stream's CRC-32 and ISIZE.
__global__ __launch_bounds__(64) void k_gzs_fin(const Batch B, const StreamArgs A)
{
    const uint32_t lane = threadIdx.x;
    if (B.status[0]) return;
    uint8_t *f = B.out;
    const uint64_t len = B.blobs[0].len;
    const uint32_t n = B.nspans;  // >= 1: an empty piece never comes here
    if (A.first && lane < 10) f[lane] = lane == 0 ? 0x1F : lane == 1 ? 0x8B : lane == 2 ? 8 : lane == 9 ? 0xFF : 0;
    uint32_t acc = 0;
    for (uint32_t k = lane; k < n; k += 64) {
        const SpanOut &o = B.sp[k];
        const uint64_t done = min<uint64_t>(len, uint64_t(k + 1) * dfl::kSpan);
        acc ^= infw::crc_mul(o.crc, infw::crc_shift(len - done));
        if (k && (o.bit & 7u)) f[o.bit >> 3] = uint8_t(B.sp[k - 1].edge_hi | o.edge_lo);
    }
    for (int o = 32; o; o >>= 1) acc ^= __shfl_xor(acc, o);
    if (lane == 0) {
        const SpanOut &o = B.sp[n - 1];
        const uint64_t E = o.bit + o.nbits;
        uint8_t *e = f + (E >> 3);
        e += dfl::stream_end(e, o.edge_hi, uint32_t(E & 7u), A.last != 0);
        if (A.last) {
            const uint32_t crc = ~(acc ^ infw::crc_mul(A.reg, infw::crc_shift(len)));
            for (int i = 0; i < 4; ++i) {
                e[i] = uint8_t(crc >> (8 * i));
                e[4 + i] = uint8_t(A.isize >> (8 * i));
            }
        }
        A.res[1] = acc;
    }
}

// ---------------------------------------------------------------------------
// k_lz_seq_wide (CDC_LEVEL_WIDE): k_lz4_seq's search with a window that starts
// up to kWideHist bytes before the segment.  One wave per segment, one wave per
// workgroup: the window (S.hist bytes of history, then the segment) and a hash
// table of 16,384 u16 window positions in LDS, 72 KiB, two workgroups per CU.
// Every history position enters the table before the first lookup (four per
// lane and step from two words), so a repeat that starts anywhere in the
// segment has its twin there whatever the stride.  A candidate more than
// kWideHist back is refused by a compare; records, nrec and trail are
// k_lz4_seq's, with offsets of up to hist + start.  It stands behind the GCM
// kernels like the DEFLATE kernels.
// ---------------------------------------------------------------------------
constexpr uint32_t kWideWin = kWideHist + kSegLZ;  // 40,960: the longest window
constexpr uint32_t kWideHashBits = 14;

struct alignas(16) WideLds {
    uint32_t data[kWideWin / 4 + 4];  // the window and 16 zero bytes after it
    uint16_t tab[1u << kWideHashBits];  // window position + 1 (0: empty)
};
static_assert(sizeof(WideLds) <= 160u * 1024u, "a workgroup's LDS");
static_assert(kWideWin + 1 <= 0xFFFFu, "window positions fit u16");
static_assert(kWideHist <= 0xFFFFu && kWideHist == dfl::kMaxDist, "the record's 16 offset bits; DEFLATE's distances");

__device__ __forceinline__ uint32_t wide_rd32(const uint32_t *d, uint32_t p)  // bytes p..p+3 (any p)
{
    return __builtin_amdgcn_alignbit(d[(p >> 2) + 1], d[p >> 2], (p & 3u) * 8u);
}

__device__ __forceinline__ uint32_t wide_rd8(const uint32_t *d, uint32_t p) { return (d[p >> 2] >> ((p & 3u) * 8u)) & 255u; }

__device__ __forceinline__ uint32_t wide_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kWideHashBits); }

__global__ __launch_bounds__(64) void k_lz_seq_wide(const Batch B)
{
    __shared__ WideLds L;
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    if (g >= B.nsegs) return;
    const Seg S = B.segs[g];
    const uint32_t n = S.len, hist = min(uint32_t(S.hist), kWideHist), W = hist + n;  // W <= kWideWin
    const uint8_t *win = B.base + S.src - hist;  // the plan keeps this inside the segment's block
    // the window into LDS: whole 16-byte pieces by unaligned global loads, eight
    // in flight per lane; the last partial piece byte by byte over zeros.
    // Nothing before win or from win + W on is read.
    const uint32_t nfull = W >> 4;
    const uint32_t nbulk = nfull & ~511u;  // 8 KiB at a time, no lane left out: nothing between the loads and the stores
    for (uint32_t i0 = 0; i0 < nbulk; i0 += 64 * 8) {
        uint4 v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) __builtin_memcpy(&v[j], win + 16 * (i0 + 64 * j + lane), 16);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) *reinterpret_cast<uint4 *>(&L.data[4 * (i0 + 64 * j + lane)]) = v[j];
    }
    for (uint32_t i = nbulk + lane; i < nfull; i += 64) {  // a blob's last, short segment
        uint4 v;
        __builtin_memcpy(&v, win + 16 * i, 16);
        *reinterpret_cast<uint4 *>(&L.data[4 * i]) = v;
    }
    const uint32_t tail = W & 15u;
    if (lane < (tail ? 8u : 4u)) L.data[4 * nfull + lane] = 0;  // at most kWideWin / 4 + 4 words: a tail means W < kWideWin
    for (uint32_t i = lane; i < (1u << kWideHashBits) / 8; i += 64) reinterpret_cast<uint4 *>(L.tab)[i] = make_uint4(0, 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane < tail) reinterpret_cast<uint8_t *>(L.data)[16 * nfull + lane] = win[16 * nfull + lane];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // every position of the history into the table, ascending, so a bucket
    // keeps the latest (within one step of 256 positions whichever lane's
    // write lands last: a candidate is verified, so any of them is sound).
    // hist is a multiple of the segment size, so whole words cover it.
    for (uint32_t j = lane; j < hist / 4; j += 64) {
        const uint32_t w0 = L.data[j], w1 = L.data[j + 1];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t v = k ? __builtin_amdgcn_alignbit(w1, w0, 8 * k) : w0;
            L.tab[wide_hash(v)] = uint16_t(4 * j + k + 1);
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // LZ4's block rules as k_lz4_seq computes them, here in window positions
    const uint32_t start_lim = hist + min(n >= 4 ? n - 3 : 0u, S.rem > 12 ? S.rem - 12 : 0u);
    const uint32_t end_lim = hist + min(n, S.rem > 5 ? S.rem - 5 : 0u);
    uint2 *rec = B.recs + uint64_t(g) * kRecCap;
    uint32_t cursor = hist, anchor = hist, nrec = 0;
    while (cursor < start_lim) {  // the cursor moves forward every turn: at most n turns
        const uint32_t stride = 1u + ((cursor - anchor) >> kSkipShift);
        const uint32_t p = cursor + lane * stride;
        const bool valid = p < start_lim;
        const uint32_t v = valid ? wide_rd32(L.data, p) : 0u;
        const uint32_t h = wide_hash(v);
        const uint32_t cand = valid ? L.tab[h] : 0u;
        const uint32_t c = cand ? cand - 1 : 0u;
        const bool ok = valid && cand != 0u && c < p && p - c <= kWideHist && wide_rd32(L.data, c) == v;
        const uint64_t m = __ballot(ok);
        __builtin_amdgcn_wave_barrier();
        if (!m) {
            if (valid) L.tab[h] = uint16_t(p + 1);
            cursor += 64 * stride;
            continue;
        }
        const uint32_t f = uint32_t(__ffsll((unsigned long long)m) - 1);
        uint32_t q = cursor + f * stride;
        uint32_t cq = uint32_t(__builtin_amdgcn_readlane(int(c), int(f)));
        uint32_t len = 4;
        // backwards over what the stride skipped: the destination not past the
        // last match's end, the source not past the window's start (the
        // distance stays what the compare allowed)
        for (;;) {
            const uint32_t room = min(q - anchor, cq);
            if (!room) break;
            const uint32_t k = lane + 1;
            const bool eq = k <= room && wide_rd8(L.data, q - k) == wide_rd8(L.data, cq - k);
            const uint64_t mm = __ballot(!eq);
            const uint32_t run = mm ? uint32_t(__ffsll((unsigned long long)mm) - 1) : 64u;
            const uint32_t back = min(run, room);
            q -= back;
            cq -= back;
            len += back;
            if (back < 64) break;
        }
        for (;;) {  // forwards to end_lim at most (cq < q: the source stays in the window)
            const uint32_t i = q + len + lane;
            const bool eq = i < end_lim && wide_rd8(L.data, i) == wide_rd8(L.data, cq + len + lane);
            const uint64_t mm = __ballot(!eq);
            if (!mm) {
                len += 64;
                continue;
            }
            len += uint32_t(__ffsll((unsigned long long)mm) - 1);
            break;
        }
        if (lane == 0) rec[nrec] = make_uint2((q - hist) | ((q - cq) << 16), len);
        ++nrec;
        if (valid && p < q + len) L.tab[h] = uint16_t(p + 1);
        __builtin_amdgcn_wave_barrier();
        anchor = cursor = q + len;
    }
    if (lane == 0) {
        B.nrec[g] = nrec;
        B.trail[g] = W - anchor;
    }
}

// ---------------------------------------------------------------------------
// k_lz_seq_deep (CDC_LEVEL_BEST): k_lz_seq_wide's window, records and loop, with
// a table of 4,096 buckets of four u16 window positions (the same 32 KiB: two
// workgroups per CU) and a one-position lazy look.  A bucket is one 8-byte
// word, the newest position in its low 16 bits; an insert shifts it by one way.
// Lanes of one step that insert into one bucket lose each other's entries:
// every candidate is verified, so any of them is sound.  A probe verifies all
// four ways; the ways of the chosen position are measured side by side,
// sixteen lanes and 64 bytes per way and turn, and the longest is taken, the
// nearest among equals.  Before a match at q is taken, the best at q + 1 is
// measured the same way, and again from there while it is strictly longer
// (DESIGN.md 5.18).
// ---------------------------------------------------------------------------
constexpr uint32_t kDeepBucketBits = 12;
constexpr uint32_t kDeepLazyMax = 128;  // a match this long is taken without the look (zlib's max_lazy)

struct alignas(16) DeepLds {
    uint32_t data[kWideWin / 4 + 4];          // the window and 16 zero bytes after it
    uint64_t tab[1u << kDeepBucketBits];      // four ways of window position + 1 (0: empty), the newest lowest
};
static_assert(sizeof(DeepLds) <= 160u * 1024u && 2 * sizeof(DeepLds) <= 160u * 1024u, "two workgroups' LDS on a CU");
static_assert(offsetof(DeepLds, tab) % 8 == 0, "a bucket is one 8-byte read");

__device__ __forceinline__ uint32_t deep_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kDeepBucketBits); }

struct DeepHit {
    uint32_t len, c;  // the longest match of the ways at a position (0: none) and its source
};

// The four ways of `bucket` against position P, alike in every lane: way
// lane / 16 compares the four bytes at P + 4 * (lane % 16).  A way that is
// empty, not before P or more than kWideHist back counts as no match, and
// nothing from end_lim on is compared.  A way that holds for all 64 bytes goes
// on with the whole wave.
__device__ __forceinline__ DeepHit deep_measure(const uint32_t *d, uint32_t P, uint32_t blo, uint32_t bhi, uint32_t end_lim,
                                                uint32_t lane)
{
    const uint32_t way = lane >> 4, k4 = (lane & 15u) * 4u;
    const uint32_t pair = (way & 2u) ? bhi : blo;
    const uint32_t cand = (way & 1u) ? pair >> 16 : pair & 0xFFFFu;
    const uint32_t c = cand - 1;
    const uint32_t i = P + k4;
    const bool wok = cand != 0u && c < P && P - c <= kWideHist && i < end_lim;
    uint32_t nb = 0;
    if (wok) {
        const uint32_t x = wide_rd32(d, i) ^ wide_rd32(d, c + k4);  // c + k4 < i < end_lim: inside the window
        nb = min(x ? uint32_t(__builtin_ctz(x)) >> 3 : 4u, end_lim - i);
    }
    const uint64_t b1 = __ballot(nb >= 1), b2 = __ballot(nb >= 2), b3 = __ballot(nb >= 3), b4 = __ballot(nb >= 4);
    DeepHit best{0, 0};
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t wp = w & 2u ? bhi : blo;
        const uint32_t wc = (w & 1u ? wp >> 16 : wp & 0xFFFFu) - 1;  // read only where the way matched
        const uint32_t open = ~uint32_t(b4 >> (16 * w)) & 0xFFFFu;   // its lanes short of four bytes
        uint32_t len;
        if (open) {
            const uint32_t at = 16 * w + uint32_t(__builtin_ctz(open));
            len = 4 * (at & 15u) + uint32_t((b1 >> at) & 1u) + uint32_t((b2 >> at) & 1u) + uint32_t((b3 >> at) & 1u);
        } else {
            len = 64;
            for (;;) {  // forwards to end_lim at most (wc < P: the source stays in the window)
                const uint32_t j = P + len + lane;
                const bool eq = j < end_lim && wide_rd8(d, j) == wide_rd8(d, wc + len + lane);
                const uint64_t mm = __ballot(!eq);
                if (!mm) {
                    len += 64;
                    continue;
                }
                len += uint32_t(__ffsll((unsigned long long)mm) - 1);
                break;
            }
        }
        if (len > best.len || (len == best.len && len && wc > best.c)) best = DeepHit{len, wc};
    }
    return best;
}

__global__ __launch_bounds__(64) void k_lz_seq_deep(const Batch B)
{
    __shared__ DeepLds L;
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    if (g >= B.nsegs) return;
    const Seg S = B.segs[g];
    const uint32_t n = S.len, hist = min(uint32_t(S.hist), kWideHist), W = hist + n;  // W <= kWideWin
    const uint8_t *win = B.base + S.src - hist;  // the plan keeps this inside the segment's block
    // the window into LDS as k_lz_seq_wide stages it: nothing before win or from win + W on is read
    const uint32_t nfull = W >> 4;
    const uint32_t nbulk = nfull & ~511u;
    for (uint32_t i0 = 0; i0 < nbulk; i0 += 64 * 8) {
        uint4 v[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) __builtin_memcpy(&v[j], win + 16 * (i0 + 64 * j + lane), 16);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) *reinterpret_cast<uint4 *>(&L.data[4 * (i0 + 64 * j + lane)]) = v[j];
    }
    for (uint32_t i = nbulk + lane; i < nfull; i += 64) {
        uint4 v;
        __builtin_memcpy(&v, win + 16 * i, 16);
        *reinterpret_cast<uint4 *>(&L.data[4 * i]) = v;
    }
    const uint32_t tail = W & 15u;
    if (lane < (tail ? 8u : 4u)) L.data[4 * nfull + lane] = 0;  // at most kWideWin / 4 + 4 words: a tail means W < kWideWin
    for (uint32_t i = lane; i < (1u << kDeepBucketBits) / 2; i += 64) reinterpret_cast<uint4 *>(L.tab)[i] = make_uint4(0, 0, 0, 0);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane < tail) reinterpret_cast<uint8_t *>(L.data)[16 * nfull + lane] = win[16 * nfull + lane];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    // every position of the history into the table, ascending by steps of 64
    // positions, so a bucket's ways are its latest (short of what one step's
    // lanes lose to each other).  hist is a multiple of the segment size.
    for (uint32_t j0 = 0; j0 < hist; j0 += 64) {
        const uint32_t pos = j0 + lane;
        const uint32_t h = deep_hash(wide_rd32(L.data, pos));
        const uint64_t old = L.tab[h];
        __builtin_amdgcn_wave_barrier();
        L.tab[h] = old << 16 | (pos + 1);
        __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const uint32_t start_lim = hist + min(n >= 4 ? n - 3 : 0u, S.rem > 12 ? S.rem - 12 : 0u);
    const uint32_t end_lim = hist + min(n, S.rem > 5 ? S.rem - 5 : 0u);
    uint2 *rec = B.recs + uint64_t(g) * kRecCap;
    uint32_t cursor = hist, anchor = hist, nrec = 0;
    while (cursor < start_lim) {  // the cursor moves forward every turn: at most n turns
        const uint32_t stride = 1u + ((cursor - anchor) >> kSkipShift);
        const uint32_t p = cursor + lane * stride;
        const bool valid = p < start_lim;
        const uint32_t v = valid ? wide_rd32(L.data, p) : 0u;
        const uint32_t h = deep_hash(v);
        const uint64_t old = valid ? L.tab[h] : 0ull;
        bool ok = false;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t cand = uint32_t(old >> (16 * w)) & 0xFFFFu, c = cand - 1;
            ok = ok || (cand != 0u && c < p && p - c <= kWideHist && wide_rd32(L.data, c) == v);
        }
        const uint64_t m = __ballot(ok);
        __builtin_amdgcn_wave_barrier();
        if (!m) {
            if (valid) L.tab[h] = old << 16 | (p + 1);
            cursor += 64 * stride;
            continue;
        }
        const uint32_t f = uint32_t(__ffsll((unsigned long long)m) - 1);
        uint32_t q = cursor + f * stride;
        DeepHit hit = deep_measure(L.data, q, uint32_t(__builtin_amdgcn_readlane(int(uint32_t(old)), int(f))),
                                   uint32_t(__builtin_amdgcn_readlane(int(uint32_t(old >> 32)), int(f))), end_lim, lane);
        uint32_t cq = hit.c, len = hit.len;  // len >= 4: lane f verified a way, and q + 4 <= end_lim
        for (bool looked = false;; looked = true) {
            // backwards over what the stride skipped (or, after a look, over
            // the byte it left): the destination not past the last match's
            // end, the source not past the window's start
            uint32_t moved = 0;
            for (;;) {
                const uint32_t room = min(q - anchor, cq);
                if (!room) break;
                const uint32_t k = lane + 1;
                const bool eq = k <= room && wide_rd8(L.data, q - k) == wide_rd8(L.data, cq - k);
                const uint64_t mm = __ballot(!eq);
                const uint32_t run = mm ? uint32_t(__ffsll((unsigned long long)mm) - 1) : 64u;
                const uint32_t back = min(run, room);
                q -= back;
                cq -= back;
                len += back;
                moved += back;
                if (back < 64) break;
            }
            if (moved || looked) break;
            // the lazy look: while the position after q has a strictly longer
            // match, q's byte stays a literal
            bool took = false;
            while (len < kDeepLazyMax && q + 1 < start_lim) {
                // q did not move back: at stride 1 q + 1 is the position lane fl probed, and that lane
                // holds its bucket (read before this step's inserts, as a read from the table here is)
                const uint32_t fl = q + 1 - cursor;
                uint32_t lo1, hi1;
                if (stride == 1 && fl < 64) {
                    lo1 = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(old)), int(fl)));
                    hi1 = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(old >> 32)), int(fl)));
                } else {
                    const uint32_t h1 = deep_hash(wide_rd32(L.data, q + 1));
                    const uint64_t b1 = L.tab[uint32_t(__builtin_amdgcn_readfirstlane(int(h1)))];
                    lo1 = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(b1))));
                    hi1 = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(b1 >> 32))));
                }
                const DeepHit nx = deep_measure(L.data, q + 1, lo1, hi1, end_lim, lane);
                if (nx.len <= len) break;
                q += 1;
                cq = nx.c;
                len = nx.len;
                took = true;
            }
            if (!took) break;
        }
        if (lane == 0) rec[nrec] = make_uint2((q - hist) | ((q - cq) << 16), len);
        ++nrec;
        if (valid && p < q + len) L.tab[h] = old << 16 | (p + 1);
        __builtin_amdgcn_wave_barrier();
        anchor = cursor = q + len;
    }
    if (lane == 0) {
        B.nrec[g] = nrec;
        B.trail[g] = W - anchor;
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static cdc::AesTables g_tab;

// The most a blob of len bytes (nblk LZ4 blocks) takes before encryption.
static uint64_t frame_max(uint64_t len, uint64_t nblk, int compress)
{
    return compress == CDC_COMPRESS_GZIP ? dfl::member_bound(len) : compress ? 7 + 4 * nblk + len + 8 : len;
}

// Workspace kept per device between calls (grow-only); a call holds its
// device's lock while it runs (the entry point is synchronous).
struct WsCache {
    std::mutex mu;
    cdc::DevBuf ws;
    cdc::PinBuf stage;  // pinned staging of the host plan (one DMA instead of pageable copies)
    hipStream_t aux = nullptr;  // k_xxh32 runs here, beside the LZ4 and GCM kernels
    hipEvent_t fork = nullptr, join = nullptr;
};
// Two per device: a caller that runs two Encode calls at once (the backup
// pipeline's two encoder threads) picks the second with cdc::t_encode_ws = 1,
// so one call's kernels run beside the other's copy-back.  Never destroyed
// (DevBuf).
static WsCache (*const g_ws)[2] = new WsCache[cdc::kMaxDevices][2];

}  // namespace enc

namespace cdc {
thread_local int t_encode_ws = 0;
}

using namespace enc;

// Device-resident encode of n blobs (see include/plakar_cdc.h).
extern "C" int cdc_encode_device(int device, const void *d_base, const uint64_t *offsets, const uint64_t *lens,
                                 uint32_t n, int compress, const uint8_t *key, const uint8_t *random, uint8_t *d_out,
                                 uint64_t out_cap, uint64_t *out_offsets, void *stream)
{
    return cdc_encode_device_level(device, d_base, offsets, lens, n, compress, key, random, d_out, out_cap, out_offsets,
                                   CDC_LEVEL_FAST, stream);
}

extern "C" int cdc_encode_device_level(int device, const void *d_base, const uint64_t *offsets, const uint64_t *lens,
                                       uint32_t n, int compress, const uint8_t *key, const uint8_t *random,
                                       uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets, int level, void *stream)
{
    if ((n && (!d_base || !offsets || !lens || !out_offsets)) || (key && !random) || !d_out) return CDC_E_INVALID;
    if (device < 0 || device >= cdc::kMaxDevices) return CDC_E_INVALID;
    if (!cdc::level_ok(level)) return CDC_E_INVALID;
    // the selector: 0 none, 2 GZIP, every other value LZ4
    const int mode = compress == CDC_COMPRESS_GZIP ? 2 : compress ? 1 : 0;
    const bool gzip = mode == 2;
    if (gzip)
        for (uint32_t b = 0; b < n; ++b)
            if (lens[b] > dfl::kMaxBlob) return CDC_E_UNSUPPORTED;  // ISIZE is 32 bits; Decode refuses such a stream
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    int st = cdc::upload_aes_tables(g_tab, g_te0, g_sbox);
    if (st != CDC_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool encrypt = key != nullptr;
    // plan on the host: blobs, 4-MiB blocks, 8-KiB segments, frame slots.
    // Counted first, then written straight into the pinned staging at their
    // workspace offsets (no vectors, no copy).
    size_t nk = 0, ng = 0, nsp = 0;
    uint64_t slot = 0, pieces_max = 0;
    for (uint32_t b = 0; b < n; ++b) {
        const uint64_t nblk = compress ? (lens[b] + kBlockLZ - 1) / kBlockLZ : 0;
        nk += nblk;
        if (nblk) ng += (nblk - 1) * ((kBlockLZ + kSegLZ - 1) / kSegLZ) +
                        (lens[b] - (nblk - 1) * kBlockLZ + kSegLZ - 1) / kSegLZ;
        if (gzip) nsp += (lens[b] + dfl::kSpan - 1) / dfl::kSpan;
        const uint64_t fmax = frame_max(lens[b], nblk, compress);
        slot += cdc::align_up(fmax, 16);
        pieces_max += encrypt ? (fmax + kPiece - 1) / kPiece : 0;
    }
    // one device allocation for the plan and the workspace
    const size_t nb = n;
    cdc::Carver cv(16);
    const size_t o_blobs = cv.take(nb * sizeof(BlobDesc)), o_blks = cv.take(nk * sizeof(Blk)),
                 o_segs = cv.take(ng * sizeof(Seg));
    const size_t o_spans = cv.take(nsp * sizeof(Span)), o_bsp = cv.take(gzip ? (nb + 1) * 4 : 0);
    const size_t o_rnd = cv.take(encrypt ? nb * 56 : 0), o_key = cv.take(32);
    const size_t o_recs = cv.take(ng * kRecCap * sizeof(uint2)), o_nrec = cv.take(ng * 4), o_trail = cv.take(ng * 4),
                 o_sout = cv.take(ng * 4);
    const size_t o_bsz = cv.take(nk * 4), o_bfo = cv.take(nk * 8), o_xxh = cv.take(nb * 4), o_flen = cv.take(nb * 8);
    const size_t o_oo = cv.take((nb + 1) * 8), o_pb = cv.take((nb + 1) * 4),
                 o_keys = cv.take(encrypt ? nb * sizeof(BlobKey) : 0);
    const size_t o_status = cv.take(16), o_frames = cv.take(encrypt ? slot : 0), o_xx = cv.take(mode == 1 ? nb * 4 : 0);
    const size_t o_sp = cv.take(nsp * sizeof(SpanOut)), o_splens = cv.take(nsp * kSpanLens),
                 o_sphdr = cv.take(nsp * dfl::kHdrWords * 4);
    WsCache &C = g_ws[device][cdc::t_encode_ws & 1];
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.ws.reserve(cv.bytes())) return CDC_E_DEVICE;
    uint8_t *const ws = C.ws.as<uint8_t>();
    if (!C.aux && (hipStreamCreateWithFlags(&C.aux, hipStreamNonBlocking) != hipSuccess ||
                   hipEventCreateWithFlags(&C.fork, hipEventDisableTiming) != hipSuccess ||
                   hipEventCreateWithFlags(&C.join, hipEventDisableTiming) != hipSuccess))
        return CDC_E_DEVICE;
    // The plan's tables at their workspace offsets [0, o_key + 32) in pinned
    // staging, XXH32 order after them: two DMAs.  (The call ends with a
    // stream sync under C.mu, so the staging is free again on return.)
    const size_t h_prefix = o_key + 32, h_xx = cdc::align_up(h_prefix, 16), h_need = h_xx + (mode == 1 ? nb * 4 : 0);
    if (!C.stage.reserve(h_need)) return CDC_E_NOMEM;
    uint8_t *const hp = C.stage.as<uint8_t>();
    {
        BlobDesc *blobs = reinterpret_cast<BlobDesc *>(hp + o_blobs);
        Blk *blks = reinterpret_cast<Blk *>(hp + o_blks);
        Seg *segs = reinterpret_cast<Seg *>(hp + o_segs);
        Span *spans = reinterpret_cast<Span *>(hp + o_spans);
        uint32_t *bsp = reinterpret_cast<uint32_t *>(hp + o_bsp);
        uint32_t kb = 0, kg = 0, ks = 0;
        uint64_t sl = 0;
        for (uint32_t b = 0; b < n; ++b) {
            BlobDesc D{};
            D.src = offsets[b];
            D.len = lens[b];
            D.blk0 = kb;
            D.nblk = compress ? uint32_t((lens[b] + kBlockLZ - 1) / kBlockLZ) : 0u;
            if (gzip) bsp[b] = ks;
            for (uint32_t k = 0; k < D.nblk; ++k) {
                Blk K{};
                K.src = offsets[b] + k * kBlockLZ;
                K.len = uint32_t(std::min<uint64_t>(kBlockLZ, lens[b] - k * kBlockLZ));
                K.blob = b;
                K.k = k;
                K.seg0 = kg;
                K.nseg = (K.len + kSegLZ - 1) / kSegLZ;
                for (uint32_t g = 0; gzip && g < K.nseg; g += dfl::kSpanSegs) {  // a block is whole spans but its last
                    Span P{};
                    P.src = K.src + uint64_t(g) * kSegLZ;
                    P.len = std::min<uint32_t>(dfl::kSpan, K.len - g * kSegLZ);
                    P.blob = b;
                    P.seg0 = kg + g;
                    P.nseg = std::min<uint32_t>(dfl::kSpanSegs, K.nseg - g);
                    P.k = ks - bsp[b];
                    P.last = k + 1 == D.nblk && g + dfl::kSpanSegs >= K.nseg;
                    spans[ks++] = P;
                }
                for (uint32_t g = 0; g < K.nseg; ++g) {
                    Seg S{};
                    S.src = K.src + uint64_t(g) * kSegLZ;
                    S.len = std::min<uint32_t>(kSegLZ, K.len - g * kSegLZ);
                    S.rem = K.len - g * kSegLZ;
                    S.hist = seg_hist(level, g * kSegLZ);
                    segs[kg++] = S;
                }
                blks[kb++] = K;
            }
            D.slot = sl;
            sl += cdc::align_up(frame_max(lens[b], D.nblk, compress), 16);
            blobs[b] = D;
        }
        if (gzip) bsp[n] = ks;
        if (kb != nk || kg != ng || ks != nsp) return CDC_E_INVALID;  // the counting pass and the plan disagree (a bug)
        if (encrypt) {
            std::memcpy(hp + o_rnd, random, nb * 56);
            std::memcpy(hp + o_key, key, 32);
        }
        if (mode == 1 && nb) {
            // XXH32 order: longest first (a wave's blobs end together); ties by
            // index, so the order is the stable one.  Keys (~len, index) sort
            // without an indirection per comparison.
            thread_local std::vector<uint64_t> xk;
            xk.resize(nb);
            for (uint32_t b = 0; b < n; ++b)
                xk[b] = (uint64_t(0xFFFFFFFFu - uint32_t(std::min<uint64_t>(lens[b], 0xFFFFFFFFu))) << 32) | b;
            std::sort(xk.begin(), xk.end());
            uint32_t *xx = reinterpret_cast<uint32_t *>(hp + h_xx);
            for (size_t i = 0; i < nb; ++i) xx[i] = uint32_t(xk[i]);
        }
    }
    Batch Bt{};
    Bt.base = static_cast<const uint8_t *>(d_base);
    Bt.nblobs = n;
    Bt.nsegs = uint32_t(ng);
    Bt.nblks = uint32_t(nk);
    Bt.npieces_max = uint32_t(pieces_max);
    Bt.compress = uint32_t(mode);
    Bt.encrypt = encrypt ? 1u : 0u;
    Bt.blobs = reinterpret_cast<BlobDesc *>(ws + o_blobs);
    Bt.blks = reinterpret_cast<Blk *>(ws + o_blks);
    Bt.segs = reinterpret_cast<Seg *>(ws + o_segs);
    Bt.rnd = ws + o_rnd;
    Bt.key = ws + o_key;
    Bt.frames = ws + o_frames;
    Bt.out = d_out;
    Bt.out_cap = out_cap;
    Bt.recs = reinterpret_cast<uint2 *>(ws + o_recs);
    Bt.nrec = reinterpret_cast<uint32_t *>(ws + o_nrec);
    Bt.trail = reinterpret_cast<uint32_t *>(ws + o_trail);
    Bt.seg_out = reinterpret_cast<uint32_t *>(ws + o_sout);
    Bt.blk_size = reinterpret_cast<uint32_t *>(ws + o_bsz);
    Bt.blk_foff = reinterpret_cast<uint64_t *>(ws + o_bfo);
    Bt.xxh = reinterpret_cast<uint32_t *>(ws + o_xxh);
    Bt.frame_len = reinterpret_cast<uint64_t *>(ws + o_flen);
    Bt.out_off = reinterpret_cast<uint64_t *>(ws + o_oo);
    Bt.piece_base = reinterpret_cast<uint32_t *>(ws + o_pb);
    Bt.keys = reinterpret_cast<BlobKey *>(ws + o_keys);
    Bt.status = reinterpret_cast<uint64_t *>(ws + o_status);
    Bt.xx_ids = reinterpret_cast<uint32_t *>(ws + o_xx);
    Bt.nspans = uint32_t(nsp);
    Bt.spans = reinterpret_cast<Span *>(ws + o_spans);
    Bt.blob_span0 = reinterpret_cast<uint32_t *>(ws + o_bsp);
    Bt.sp = reinterpret_cast<SpanOut *>(ws + o_sp);
    Bt.sp_lens = ws + o_splens;
    Bt.sp_hdr = reinterpret_cast<uint32_t *>(ws + o_sphdr);
    const uint32_t xx_wgs = (n + kXxWaves * kXxPerWave - 1) / (kXxWaves * kXxPerWave);
    bool ok = hipMemcpyAsync(ws, hp, h_prefix, hipMemcpyHostToDevice, s) == hipSuccess;
    if (mode == 1 && nb)
        ok = ok && hipMemcpyAsync(ws + o_xx, hp + h_xx, nb * 4, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok && n) {
        if (gzip) {
            launch_seq(Bt, level, ng, s);
            if (nsp) hipLaunchKernelGGL(k_dfl_size, dim3(uint32_t(nsp)), dim3(kDflThreads), 0, s, Bt);
        } else if (compress) {
            ok = hipEventRecord(C.fork, s) == hipSuccess && hipStreamWaitEvent(C.aux, C.fork, 0) == hipSuccess;
            hipLaunchKernelGGL(k_xxh32, dim3(xx_wgs), dim3(kXxWaves * 64), 0, C.aux, Bt);
            ok = ok && hipEventRecord(C.join, C.aux) == hipSuccess;
            launch_seq(Bt, level, ng, s);
            if (nk) hipLaunchKernelGGL(k_lz4_size, dim3(uint32_t(nk)), dim3(kBlkThreads), 0, s, Bt);
        }
        hipLaunchKernelGGL(k_enc_plan, dim3(1), dim3(kPlanThreads), 0, s, Bt);
        if (encrypt) {
            hipLaunchKernelGGL(k_blob_keys, dim3((n + kKeyThreads - 1) / kKeyThreads), dim3(kKeyThreads), 0, s, Bt);
            hipLaunchKernelGGL(k_blob_pows, dim3((n + kPowWaves - 1) / kPowWaves), dim3(kPowWaves * 64), 0, s, Bt);
        }
        if (gzip) {
            if (nsp) hipLaunchKernelGGL(k_dfl_emit, dim3(uint32_t(nsp)), dim3(kDflThreads), 0, s, Bt);
            hipLaunchKernelGGL(k_gz_fin, dim3(n), dim3(64), 0, s, Bt);
        } else if (compress) {
            if (nk) hipLaunchKernelGGL(k_lz4_emit, dim3(uint32_t(nk), kEmitSplit), dim3(kBlkThreads), 0, s, Bt);
            ok = ok && hipStreamWaitEvent(s, C.join, 0) == hipSuccess;  // the content checksums
            hipLaunchKernelGGL(k_frame_fin, dim3((n + 63) / 64), dim3(64), 0, s, Bt);
        } else if (!encrypt) {
            hipLaunchKernelGGL(k_copy, dim3(n), dim3(256), 0, s, Bt);
        }
        if (encrypt && pieces_max)
            // a persistent grid: one workgroup per CU (its LDS holds one)
            hipLaunchKernelGGL(k_gcm,
                               dim3(uint32_t(std::min<uint64_t>((pieces_max + kGcmWaves - 1) / kGcmWaves,
                                                                uint64_t(cdc::device_cus(device))))),
                               dim3(kGcmWaves * 64), 0, s, Bt);
        ok = hipGetLastError() == hipSuccess;
    }
    uint64_t status = 0;
    if (ok) {
        if (n) {
            ok = hipMemcpyAsync(out_offsets, ws + o_oo, (nb + 1) * 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
                 hipMemcpyAsync(&status, ws + o_status, 8, hipMemcpyDeviceToHost, s) == hipSuccess;
        } else if (out_offsets) {
            out_offsets[0] = 0;
        }
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
    }
    if (!ok) return CDC_E_DEVICE;
    return status ? int(int32_t(uint32_t(status))) : CDC_OK;
}

extern "C" uint64_t cdc_encode_bound(uint64_t len, int compress, int encrypt)
{
    const uint64_t f = frame_max(len, (len + kBlockLZ - 1) / kBlockLZ, compress);
    return encrypt ? 60 + f + 28 * ((f + kPiece - 1) / kPiece) : f;
}

// ---------------------------------------------------------------------------
// The streamed gzip member (see include/plakar_cdc.h).  The writer owns its
// workspace, so it shares nothing with cdc_encode_device's; the running CRC-32
// register and length live here, on the host.
// ---------------------------------------------------------------------------
struct cdc_gzip_stream {
    int device = 0;
    bool first = true, closed = false;
    int level = CDC_LEVEL_FAST;  // cdc_gzip_stream_set_level, before the first piece
    uint32_t reg = 0xFFFFFFFFu;  // CRC-32 register over the bytes so far
    uint64_t total = 0;
    std::mutex mu;
    cdc::DevBuf ws;
    cdc::PinBuf stage;
};

extern "C" int cdc_gzip_stream_new(int device, cdc_gzip_stream **out)
{
    if (!out || device < 0 || device >= cdc::kMaxDevices) return CDC_E_INVALID;
    cdc_gzip_stream *s = new (std::nothrow) cdc_gzip_stream;
    if (!s) return CDC_E_NOMEM;
    s->device = device;
    *out = s;
    return CDC_OK;
}

extern "C" void cdc_gzip_stream_free(cdc_gzip_stream *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

extern "C" uint64_t cdc_gzip_stream_bound(uint64_t len) { return dfl::stream_piece_bound(len); }

extern "C" int cdc_gzip_stream_set_level(cdc_gzip_stream *S, int level)
{
    if (!S || (!cdc::level_ok(level))) return CDC_E_INVALID;
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->first || S->closed) return CDC_E_INVALID;  // a member is written at one level
    S->level = level;
    return CDC_OK;
}

extern "C" int cdc_gzip_stream_piece(cdc_gzip_stream *S, const void *d_in, uint64_t len, int last, uint8_t *d_out,
                                     uint64_t out_cap, uint64_t *out_len, void *stream)
{
    if (!S || !out_len || (len && !d_in)) return CDC_E_INVALID;
    *out_len = 0;
    if (len > dfl::kMaxBlob) return CDC_E_UNSUPPORTED;  // a piece's bit positions and spans are planned like a blob's
    std::lock_guard<std::mutex> lk(S->mu);
    if (S->closed) return CDC_E_INVALID;
    if (len == 0 && !last) return CDC_OK;
    if (!d_out) return CDC_E_INVALID;
    if (hipSetDevice(S->device) != hipSuccess) return CDC_E_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (len == 0) {
        // nothing to deflate: the header when no piece came before, the final
        // block and the trailer, written here (gzip.Writer's Close: a stream
        // with no bytes at all is still a whole member)
        uint8_t b[10 + dfl::kFinalBytes + 8];
        uint32_t n = 0;
        if (S->first) {
            const uint8_t hdr[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};
            std::memcpy(b, hdr, 10);
            n = 10;
        }
        const uint8_t fin[dfl::kFinalBytes] = {1, 0, 0, 0xFF, 0xFF};
        std::memcpy(b + n, fin, sizeof(fin));
        n += dfl::kFinalBytes;
        const uint32_t crc = ~S->reg;
        for (int i = 0; i < 4; ++i) {
            b[n + i] = uint8_t(crc >> (8 * i));
            b[n + 4 + i] = uint8_t(uint32_t(S->total) >> (8 * i));
        }
        n += 8;
        *out_len = n;
        if (n > out_cap) return CDC_E_NOSPACE;
        if (hipMemcpyAsync(d_out, b, n, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return CDC_E_DEVICE;
        S->first = false;
        S->closed = true;
        return CDC_OK;
    }
    // the piece as one blob of a GZIP batch: 4-MiB blocks (the match search's
    // end-of-block rules), 8-KiB segments, 32-KiB spans
    const size_t nk = size_t((len + kBlockLZ - 1) / kBlockLZ), ng = size_t((len + kSegLZ - 1) / kSegLZ),
                 nsp = size_t((len + dfl::kSpan - 1) / dfl::kSpan);
    cdc::Carver cv(16);
    const size_t o_blobs = cv.take(sizeof(BlobDesc)), o_segs = cv.take(ng * sizeof(Seg)),
                 o_spans = cv.take(nsp * sizeof(Span)), o_bsp = cv.take(2 * 4);
    const size_t h_prefix = cv.bytes();
    const size_t o_recs = cv.take(ng * kRecCap * sizeof(uint2)), o_nrec = cv.take(ng * 4), o_trail = cv.take(ng * 4);
    const size_t o_flen = cv.take(8), o_oo = cv.take(2 * 8), o_status = cv.take(16), o_res = cv.take(16);
    const size_t o_sp = cv.take(nsp * sizeof(SpanOut)), o_splens = cv.take(nsp * kSpanLens),
                 o_sphdr = cv.take(nsp * dfl::kHdrWords * 4);
    if (!S->ws.reserve(cv.bytes())) return CDC_E_DEVICE;
    if (!S->stage.reserve(h_prefix)) return CDC_E_NOMEM;
    uint8_t *const ws = S->ws.as<uint8_t>(), *const hp = S->stage.as<uint8_t>();
    {
        BlobDesc D{};
        D.len = len;
        D.nblk = uint32_t(nk);
        std::memcpy(hp + o_blobs, &D, sizeof(D));
        Seg *segs = reinterpret_cast<Seg *>(hp + o_segs);
        Span *spans = reinterpret_cast<Span *>(hp + o_spans);
        uint32_t *bsp = reinterpret_cast<uint32_t *>(hp + o_bsp);
        size_t kg = 0, ks = 0;
        for (size_t k = 0; k < nk; ++k) {
            const uint64_t src = k * kBlockLZ;
            const uint32_t blen = uint32_t(std::min<uint64_t>(kBlockLZ, len - src));
            const uint32_t nseg = (blen + kSegLZ - 1) / kSegLZ;
            for (uint32_t g = 0; g < nseg; g += dfl::kSpanSegs) {
                Span P{};
                P.src = src + uint64_t(g) * kSegLZ;
                P.len = std::min<uint32_t>(dfl::kSpan, blen - g * kSegLZ);
                P.seg0 = uint32_t(kg + g);
                P.nseg = std::min<uint32_t>(dfl::kSpanSegs, nseg - g);
                P.k = uint32_t(ks);
                spans[ks++] = P;  // last = 0: no block of a piece carries BFINAL
            }
            for (uint32_t g = 0; g < nseg; ++g) {
                Seg G{};
                G.src = src + uint64_t(g) * kSegLZ;
                G.len = std::min<uint32_t>(kSegLZ, blen - g * kSegLZ);
                G.rem = blen - g * kSegLZ;
                G.hist = seg_hist(S->level, g * kSegLZ);
                segs[kg + g] = G;
            }
            kg += nseg;
        }
        bsp[0] = 0;
        bsp[1] = uint32_t(nsp);
        if (kg != ng || ks != nsp) return CDC_E_INVALID;  // the counts and the plan disagree (a bug)
    }
    Batch Bt{};
    Bt.base = static_cast<const uint8_t *>(d_in);
    Bt.nblobs = 1;
    Bt.nsegs = uint32_t(ng);
    Bt.nblks = uint32_t(nk);
    Bt.compress = 2;
    Bt.blobs = reinterpret_cast<BlobDesc *>(ws + o_blobs);
    Bt.segs = reinterpret_cast<Seg *>(ws + o_segs);
    Bt.out = d_out;
    Bt.out_cap = out_cap;
    Bt.recs = reinterpret_cast<uint2 *>(ws + o_recs);
    Bt.nrec = reinterpret_cast<uint32_t *>(ws + o_nrec);
    Bt.trail = reinterpret_cast<uint32_t *>(ws + o_trail);
    Bt.frame_len = reinterpret_cast<uint64_t *>(ws + o_flen);
    Bt.out_off = reinterpret_cast<uint64_t *>(ws + o_oo);
    Bt.status = reinterpret_cast<uint64_t *>(ws + o_status);
    Bt.nspans = uint32_t(nsp);
    Bt.spans = reinterpret_cast<Span *>(ws + o_spans);
    Bt.blob_span0 = reinterpret_cast<uint32_t *>(ws + o_bsp);
    Bt.sp = reinterpret_cast<SpanOut *>(ws + o_sp);
    Bt.sp_lens = ws + o_splens;
    Bt.sp_hdr = reinterpret_cast<uint32_t *>(ws + o_sphdr);
    StreamArgs A{};
    A.first = S->first ? 1u : 0u;
    A.last = last ? 1u : 0u;
    A.reg = S->reg;
    A.isize = uint32_t(S->total + len);
    A.res = reinterpret_cast<uint64_t *>(ws + o_res);
    static_assert(sizeof(uint64_t) * 4 == 32, "status and res are read back together");
    uint64_t back[4] = {0, 0, 0, 0};  // status[0..1], res[0..1]: consecutive 16-byte regions
    bool ok = o_res == o_status + 16 && hipMemcpyAsync(ws, hp, h_prefix, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        launch_seq(Bt, S->level, ng, s);
        hipLaunchKernelGGL(k_dfl_size, dim3(uint32_t(nsp)), dim3(kDflThreads), 0, s, Bt);
        hipLaunchKernelGGL(k_gzs_plan, dim3(1), dim3(64), 0, s, Bt, A);
        hipLaunchKernelGGL(k_dfl_emit, dim3(uint32_t(nsp)), dim3(kDflThreads), 0, s, Bt);
        hipLaunchKernelGGL(k_gzs_fin, dim3(1), dim3(64), 0, s, Bt, A);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(back, ws + o_status, sizeof(back), hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    }
    if (!ok) return CDC_E_DEVICE;
    *out_len = back[2];
    if (back[0]) return int(int32_t(uint32_t(back[0])));  // CDC_E_NOSPACE: nothing written, the writer as it was
    S->reg = infw::crc_mul(S->reg, infw::crc_shift(len)) ^ uint32_t(back[3]);
    S->total += len;
    S->first = false;
    S->closed = last != 0;
    return CDC_OK;
}
