// Decode on the device: plakar's (*Repository).Decode (repository/repository.go:
// 186-210) of a batch of blobs: encryption.DecryptStream (encryption/
// symmetric.go:165-243), then compression.InflateLZ4Stream (compression/
// compression.go:148-160; the LZ4 frame reader of github.com/pierrec/lz4/v4).
// The mirror image of cdc_encode.hip, whose AES, GHASH and XXH32 device code
// it shares (cdc_crypto_dev.h).
//
// Kernels, in launch order (one batch = the blobs of one call; the host plans
// what follows from the lengths alone: records, frame slots, short streams):
//   k_dec_keys    one thread per blob: opens Seal(key, nonce, subkey) at the
//                 blob's start (tag compared in full), the subkey's round
//                 keys, H and its 4-bit table
//   k_dec_pows    one wave per blob: H^1..H^64, the 8-bit table of H^64
//   k_rec_open    one wave per record nonce(12) || ciphertext || tag(16), the
//                 nonce read from the stream: GHASH over the ciphertext, the
//                 tag compared in full, AES-256-CTR into the blob's frame slot.
//                 Uncompressed blobs take two passes, hash first and CTR
//                 straight into d_out once the plan knows where
//   k_lz4_size    one wave per blob: the frame header, the block walk, every
//                 block's sequences validated and sized (lz4_walk.h), block
//                 checksums, content size
//   k_dec_plan    one workgroup: exclusive scan of the decoded sizes (failed
//                 blobs count 0): out_offsets, the CDC_E_NOSPACE test
//   k_lz4_emit    one wave per blob: the same walk again, now writing: literal
//                 runs and stored blocks as 16-byte copies 64 lanes wide,
//                 matches 64 lanes wide from the output written so far; then
//                 the content checksum over the output
//   k_dec_compact one workgroup, only when a content checksum failed after the
//                 plan: moves the later blobs down so that the failed one
//                 contributes no bytes
//   k_dec_copy    neither compressed nor encrypted: the blob itself
// With compressed == CDC_COMPRESS_GZIP (compression.InflateGzipStream, compression/
// compression.go:130-146) two kernels stand in the place of the LZ4 ones:
//   k_gz_size     one wave per blob: the member header, the trailer's place,
//                 ISIZE as the claimed size, the 1032 : 1 ceiling.  It does not
//                 inflate: the claim is a plan
//   k_gz_emit     one wave per blob: inflates into the planned range (at most
//                 the claim: inflate_walk.h bounds every literal and match),
//                 then CRC-32 and ISIZE against the output.  Every failure
//                 here is late (kFlagLate): k_dec_compact closes the gap
// cdc_decode_prefix_device (the first upto[i] bytes of blob i; the sizes are an
// input, so nothing is sized, planned on the device or compacted):
//   k_lz4_prefix  one wave per blob: k_lz4_emit's walk in the walker's stop
//                 mode, the sequence that crosses upto cut to the byte; block
//                 checksums of the blocks walked to their end, and the frame's
//                 end (content size and checksum) only when the walk gets there
//   k_gz_prefix   one wave per blob: k_gz_emit's walk in the stop mode; CRC-32
//                 and ISIZE only when the walk reaches the final block's end
//   k_prefix_copy not compressed: the first upto bytes, of the blob or of the
//                 records opened for it (k_rec_open into a frame slot)
//
// No block table is kept: both LZ4 passes walk the frame from its header, so
// a frame of very many short blocks needs no memory of its own (it only runs
// its blocks one after the other in its wave, as every frame does).
//
// Every read of d_in stays inside the blob it belongs to and every write
// inside the blob's planned output range: the walker bounds each sequence
// (lz4_walk.h), copies are exact to the byte, and the emit pass validates
// again instead of trusting the sizing pass (so even input that changes
// between the passes cannot write out of range).
//
// A trailing record shorter than 28 bytes is CDC_E_CORRUPT.  The reference
// errors on all such lengths but one: exactly 12 trailing bytes (a nonce and
// then a clean EOF) end its loop without error.  No writer produces that
// stream; it is rejected here too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <vector>

#include "cdc_crypto_dev.h"
#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "inflate_walk.h"
#include "lz4_walk.h"

namespace dec {

using namespace devc;

constexpr uint32_t kPiece = 65536;         // DecryptStream's chunkSize
constexpr uint32_t kRecMax = kPiece + 28;  // nonce, ciphertext, tag
constexpr uint32_t kHdr = 60;              // subkey nonce || Seal(key, nonce, subkey)

// This file's own copies of the AES tables (no relocatable device code).
__device__ uint32_t g_te0[256];
__device__ uint8_t g_sbox[256];

struct DBlob {       // planned on the host from the lengths
    uint64_t src;    // byte offset in d_in
    uint64_t len;    // stored bytes
    uint64_t slot;   // the decrypted frame's place in the frame buffer (16-B aligned)
    uint64_t flen;   // bytes after decryption (the stored length when not encrypted)
    uint32_t rec0, nrec;
};

struct DBatch {
    const uint8_t *in;
    uint32_t n, compressed, encrypted, nrecs;  // compressed: 0, 1 (LZ4) or 2 (GZIP)
    const DBlob *blobs;
    const uint8_t *key;   // repository key (32 B, device)
    uint8_t *frames;
    uint8_t *out;
    uint64_t out_cap;
    BlobKey *keys;        // per blob
    int32_t *status;      // per blob
    uint64_t *dsize;      // per blob: decoded bytes (k_lz4_size), or the claim (k_gz_size)
    uint64_t *out_off;    // n + 1
    uint32_t *flags;      // see kFlag*
};
constexpr uint32_t kFlagNoSpace = 0, kFlagTicketA = 1, kFlagTicketB = 2, kFlagLate = 3;

__device__ __forceinline__ const uint8_t *stream_ptr(const DBatch &B, const DBlob &D)
{
    return B.encrypted ? B.frames + D.slot : B.in + D.src;
}

// dst[0, n) = src[0, n), to the byte: 16-byte pieces (any alignment) by the
// threads [tid, nt), then the last n % 16 bytes one by one.
__device__ __forceinline__ void copy_exact(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t tid, uint32_t nt)
{
    const uint64_t nq = n / 16;
    for (uint64_t c = tid; c < nq; c += nt) {
        uint4 v;
        __builtin_memcpy(&v, src + 16 * c, 16);
        __builtin_memcpy(dst + 16 * c, &v, 16);
    }
    const uint32_t tail = uint32_t(n - 16 * nq);
    if (tid < tail) dst[16 * nq + tid] = src[16 * nq + tid];
}

// ---------------------------------------------------------------------------
// a. Subkey open
// ---------------------------------------------------------------------------
constexpr uint32_t kKeyThreads = 64;
constexpr uint32_t kPowWaves = 4;

__global__ __launch_bounds__(kKeyThreads) void k_dec_keys(const DBatch B)
{
    __shared__ uint32_t s_te[256];
    __shared__ uint8_t s_sb[256];
    __shared__ uint32_t s_mrk[60];
    __shared__ G128 s_mth[16];
    __shared__ uint32_t s_rk[kKeyThreads][61];  // a thread's schedule and table (LDS, not private memory)
    __shared__ G128 s_th[kKeyThreads][17];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < 256; i += kKeyThreads) {
        s_te[i] = g_te0[i];
        s_sb[i] = g_sbox[i];
    }
    __syncthreads();
    if (t == 0) {  // the repository key: schedule, H and its table
        uint8_t key[32];
        for (int i = 0; i < 32; ++i) key[i] = B.key[i];
        aes256_expand(key, s_mrk, s_sb);
        uint32_t z[4] = {0, 0, 0, 0};
        aes256_block(s_mrk, s_te, s_sb, z);
        gtable(g_from_words(z), s_mth);
    }
    __syncthreads();
    const uint32_t b = blockIdx.x * kKeyThreads + t;
    if (b >= B.n || B.status[b]) return;
    const uint8_t *h = B.in + B.blobs[b].src;  // nonce 12, sealed subkey 32, tag 16 (len >= 60: the host checked)
    uint32_t j0[3];
    for (int i = 0; i < 3; ++i)
        j0[i] = uint32_t(h[4 * i]) << 24 | uint32_t(h[4 * i + 1]) << 16 | uint32_t(h[4 * i + 2]) << 8 | h[4 * i + 3];
    G128 S = {0, 0};
    uint8_t sub[32];
    for (uint32_t i = 0; i < 2; ++i) {
        uint32_t cw[4];
        gcm_block_words(h + 12 + 16 * i, cw);
        S = gmul4(gx(S, g_from_words(cw)), s_mth);
        uint32_t c[4] = {j0[0], j0[1], j0[2], 2 + i};
        aes256_block(s_mrk, s_te, s_sb, c);
        for (int k = 0; k < 4; ++k) {
            const uint32_t p = c[k] ^ cw[k];
            sub[16 * i + 4 * k] = uint8_t(p >> 24);
            sub[16 * i + 4 * k + 1] = uint8_t(p >> 16);
            sub[16 * i + 4 * k + 2] = uint8_t(p >> 8);
            sub[16 * i + 4 * k + 3] = uint8_t(p);
        }
    }
    S = gmul4(gx(S, G128{0, 256}), s_mth);  // len(A) = 0, len(C) = 256 bits
    uint32_t tg[4] = {j0[0], j0[1], j0[2], 1};
    aes256_block(s_mrk, s_te, s_sb, tg);
    uint32_t tw[4];
    gcm_block_words(h + 44, tw);
    const G128 want = g_from_words(tw), got = gx(S, g_from_words(tg));
    if ((want.hi ^ got.hi) | (want.lo ^ got.lo)) {  // all 16 bytes, no early exit
        B.status[b] = CDC_E_AUTH;
        return;
    }
    BlobKey &K = B.keys[b];
    aes256_expand(sub, s_rk[t], s_sb);
    for (int i = 0; i < 60; ++i) K.rk[i] = s_rk[t][i];
    uint32_t z[4] = {0, 0, 0, 0};
    aes256_block(s_rk[t], s_te, s_sb, z);
    const G128 H = g_from_words(z);
    K.hpow[0] = H;
    gtable(H, s_th[t]);
    for (int i = 0; i < 16; ++i) K.th[i] = s_th[t][i];
}

__global__ __launch_bounds__(kPowWaves * 64) void k_dec_pows(const DBatch B)
{
    __shared__ PowLds S[kPowWaves];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kPowWaves + wv;
    if (b >= B.n || B.status[b]) return;
    hpow_ladder(B.keys[b], S[wv], lane);
}

// ---------------------------------------------------------------------------
// b. Record open: Encode's k_gcm run backwards.  GHASH runs over the bytes
// read, the keystream turns them into the plaintext.  mode bit 0: hash and
// compare the tag; bit 1: CTR (into the frame slot, or, kToOut, into d_out
// at the blob's planned offset).
// ---------------------------------------------------------------------------
constexpr uint32_t kOpenHash = 1, kOpenCtr = 2, kOpenToOut = 4;

__global__ __launch_bounds__(kGcmWaves * 64) void k_rec_open(const DBatch B, const uint32_t mode)
{
    __shared__ GcmLds L;
    for (uint32_t i = threadIdx.x; i < 256 * 64; i += blockDim.x)
        L.te[i] = (i & 32u) ? ror32(g_te0[i >> 6], 8) : g_te0[i >> 6];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, laneoff = (lane & 31u) << 2;
    const char *te = reinterpret_cast<const char *>(L.te);
    __syncthreads();
    if ((mode & kOpenToOut) && B.flags[kFlagNoSpace]) return;
    uint32_t *ticket = &B.flags[(mode & kOpenToOut) ? kFlagTicketB : kFlagTicketA];
    for (;;) {
    uint32_t pc = atomicAdd(ticket, lane == 0 ? 1u : 0u);  // every lane (see k_gcm)
    pc = uint32_t(__builtin_amdgcn_readfirstlane(int(pc)));
    if (pc >= B.nrecs) break;
    uint32_t b;
    {
        uint32_t lo = 0, hi = B.n;  // last blob with rec0 <= pc: the one that holds record pc
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (B.blobs[mid].rec0 <= pc) lo = mid;
            else hi = mid;
        }
        b = lo;
    }
    if (B.status[b]) continue;  // the subkey did not open (or, second pass, a record did not)
    const DBlob D = B.blobs[b];
    const BlobKey &K = B.keys[b];
    for (uint32_t i = lane; i < 60; i += 64) L.w[wv].rk[i] = K.rk[i];
    for (uint32_t i = lane; i < 60; i += 64) L.w[wv].rk16[i] = ror32(K.rk[i], 16);
    if (lane < 16) L.w[wv].th[lane] = K.th[lane];
    for (uint32_t i = lane; i < 256; i += 64) L.w[wv].t64[i] = K.t64[i];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const uint32_t k = pc - D.rec0;
    const uint64_t r0 = kHdr + uint64_t(k) * kRecMax;                       // the record in the blob
    const uint32_t m = uint32_t(min<uint64_t>(kRecMax, D.len - r0)) - 28u;  // ciphertext bytes (>= 0: the host checked)
    const uint32_t nb = (m + 15) / 16;
    const uint8_t *rec = B.in + D.src + r0;
    const gu8 *ct = reinterpret_cast<const gu8 *>(reinterpret_cast<uintptr_t>(rec + 12));
    const uint32_t ct_sh = uint32_t(reinterpret_cast<uintptr_t>(ct) & 3u);
    uint8_t *o = ((mode & kOpenToOut) ? B.out + B.out_off[b] : B.frames + D.slot) + uint64_t(k) * kPiece;
    uint32_t j0[3];
    for (int i = 0; i < 3; ++i)
        j0[i] = uint32_t(rec[4 * i]) << 24 | uint32_t(rec[4 * i + 1]) << 16 | uint32_t(rec[4 * i + 2]) << 8 |
                rec[4 * i + 3];
    const CtrPre cpre = ctr_pre(L.w[wv], te, laneoff, j0);
    const G128 *t64 = L.w[wv].t64;
    uint8_t *stage = reinterpret_cast<uint8_t *>(L.w[wv].stage);
    // The ciphertext as dwords from its aligned-down start: the dwords that
    // hold its first and last byte lie inside the record (the nonce before,
    // the tag after), and the buffer returns 0 past them.
    const uint32_t lastq = m ? (ct_sh + m - 1) >> 2 : 0u;
    const __amdgpu_buffer_rsrc_t prs = gcm_rsrc(reinterpret_cast<uintptr_t>(ct) - ct_sh, uint64_t(lastq + 1) * 4);
    const bool ct_fast = ct_sh == 0 && (m & 15u) == 0;
    G128 Z = {0, 0};
    uint32_t cnt = 0;
    const uint32_t rows = (nb + 63) / 64;
    for (uint32_t j = 0; j < rows; j += kGcmRows) {
        uint32_t c[kGcmRows][4];
        uint32_t px[kGcmRows][5];
#pragma unroll
        for (int u = 0; u < int(kGcmRows); ++u) {
            const int32_t i = int32_t(64 * (j + u) + lane);
            if (ct_fast) {
                const uint4 v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(prs, 16 * i, 0, 0));
                px[u][0] = v.x;
                px[u][1] = v.y;
                px[u][2] = v.z;
                px[u][3] = v.w;
                px[u][4] = 0;
            } else {
#pragma unroll
                for (int q = 0; q < 5; ++q)
                    px[u][q] = __builtin_amdgcn_raw_buffer_load_b32(prs, int32_t(4 * min(uint32_t(4 * i + q), lastq)), 0, 0);
            }
        }
        if (mode & kOpenCtr) {
            uint32_t ctr[kGcmRows];
#pragma unroll
            for (uint32_t u = 0; u < kGcmRows; ++u) ctr[u] = 2 + 64 * (j + u) + lane;
            aes256_ctr_lds<kGcmRows>(L.w[wv], te, laneoff, cpre, ctr, c);
        }
#pragma unroll
        for (int u = 0; u < int(kGcmRows); ++u) {
            const uint32_t i = 64 * (j + u) + lane;
            uint4 pw = make_uint4(0, 0, 0, 0);
            if (i < nb) {
                const uint32_t bytes = min(16u, m - 16 * i);
                uint32_t w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = be32(__builtin_amdgcn_alignbit(px[u][q + 1], px[u][q], 8 * ct_sh));
                if (bytes < 16) {  // what follows the ciphertext (the tag) is neither hashed nor decrypted
                    for (int q = 0; q < 4; ++q) {
                        const int keep = int(bytes) - 4 * q;
                        w[q] = keep >= 4 ? w[q] : keep <= 0 ? 0u : (w[q] & ~(0xFFFFFFFFu >> (8 * keep)));
                    }
                }
                if (mode & kOpenHash) {
                    Z = gx(gmul8(Z, t64), G128{uint64_t(w[0]) << 32 | w[1], uint64_t(w[2]) << 32 | w[3]});
                    ++cnt;
                }
                if (mode & kOpenCtr) pw = make_uint4(be32(w[0] ^ c[u][0]), be32(w[1] ^ c[u][1]), be32(w[2] ^ c[u][2]),
                                                     be32(w[3] ^ c[u][3]));
            }
            L.w[wv].stage[64 * u + lane] = pw;
        }
        __builtin_amdgcn_wave_barrier();
        if (mode & kOpenCtr) {
            // the rows' plaintext through LDS, as k_gcm stores its ciphertext:
            // exactly row_bytes bytes
            const uint32_t row_bytes = min(1024u * kGcmRows, m - 1024 * j);
            uint8_t *dst = o + 1024 * j;
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
    if (mode & kOpenHash) {
        if (cnt) {
            const uint32_t e = nb - lane - 64 * (cnt - 1);  // 1..64
            Z = gmul_bits(Z, K.hpow[e - 1]);
        }
        for (int off = 32; off; off >>= 1) {
            Z.hi ^= __shfl_xor(Z.hi, off);
            Z.lo ^= __shfl_xor(Z.lo, off);
        }
        if (lane == 0) {
            const G128 S = gmul4(gx(Z, G128{0, uint64_t(m) * 8}), L.w[wv].th);
            uint32_t t[1][4] = {{j0[0], j0[1], j0[2], 1}};
            aes256_blocks_lds<1>(L.w[wv], te, laneoff, t);
            uint32_t tw[4];
            gcm_block_words(rec + 12 + m, tw);
            const G128 want = g_from_words(tw), got = gx(S, g_from_words(t[0]));
            if ((want.hi ^ got.hi) | (want.lo ^ got.lo)) B.status[b] = CDC_E_AUTH;  // all 16 bytes, no early exit
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------
// c-e. The LZ4 frame, one wave per blob
// ---------------------------------------------------------------------------
// Byte i of a block for the walker, wave-uniform: the lanes hold the 64 bytes
// from `base` on (zero past the block's end) and a read outside them reloads
// the window at i, so a sequence costs about one load, not one per byte.
struct WaveRd {
    const uint8_t *p;
    uint32_t n, lane, base, v;
    __device__ __forceinline__ uint32_t operator()(uint32_t i)
    {
        if (i - base >= 64u) {
            base = i;
            v = i + lane < n ? p[i + lane] : 0u;
        }
        return uint32_t(__builtin_amdgcn_readlane(int(v), __builtin_amdgcn_readfirstlane(int(i - base))));
    }
};

// Stores of this wave so far are visible to its later loads, other lanes'
// included: they go through the CU's own L1, so the workgroup scope is enough
// (no write-back, no invalidate).  The fence keeps the compiler's order; the
// wait is written out because the order must not depend on whether the
// compiler thinks one is due.
__device__ __forceinline__ void wave_publish()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// One block: the decoded size, or -1.  dst == nullptr sizes only; otherwise
// dst[0, omax) at most is written.  A match reads the output before it (see
// lz4w::match_src), which earlier sequences of this wave stored: the wave
// waits for its stores only when a match reaches into bytes stored since the
// last wait.
__device__ int64_t wave_block(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t omax, uint32_t lane)
{
    WaveRd rd{src, n, lane, n, 0u};  // base = n: the first read loads the window
    uint32_t ip = 0, opos = 0, published = 0;
    for (;;) {
        lz4w::Seq s;
        const int r = lz4w::next_seq(rd, n, ip, opos, omax, s);
        if (r < 0) return -1;
        if (dst && s.lit_len) copy_exact(dst + opos, src + s.lit_src, s.lit_len, lane, 64);
        opos += s.lit_len;
        if (r == lz4w::kEnd) return int64_t(opos);
        if (dst) {
            if (opos - s.off + min(s.off, s.mlen) > published) {
                wave_publish();
                published = opos;
            }
            if (s.off >= s.mlen) {
                copy_exact(dst + opos, dst + opos - s.off, s.mlen, lane, 64);
            } else {
                for (uint32_t i = lane; i < s.mlen; i += 64) dst[opos + i] = dst[lz4w::match_src(opos, s.off, s.mlen, i)];
            }
        }
        opos += s.mlen;
    }
}

// XXH32 of p[0, n) by one wave: lanes 0-3 run the four accumulators.
__device__ uint32_t wave_xxh32(const uint8_t *p, uint64_t n, uint32_t lane)
{
    const uint32_t a = lane & 3u;
    uint32_t v = a == 0 ? P1 + P2 : a == 1 ? P2 : a == 2 ? 0u : 0u - P1;
    if (lane < 4) {
        const uint64_t stripes = n / 16;
        const uint8_t *q = p + 4 * a;
#pragma unroll 8
        for (uint64_t s = 0; s < stripes; ++s) {
            uint32_t w;
            __builtin_memcpy(&w, q + 16 * s, 4);
            v = rol32(v + w * P2, 13) * P1;
        }
    }
    const uint32_t v1 = __shfl(v, 0), v2 = __shfl(v, 1), v3 = __shfl(v, 2), v4 = __shfl(v, 3);
    return xxh_finish(v1, v2, v3, v4, p, n);
}

struct FrameHdr {
    uint32_t hlen, bmax;
    bool bchk, csize, cchk;
    uint64_t content;
};

__device__ int32_t frame_header(const uint8_t *f, uint64_t n, FrameHdr &F)
{
    if (n < 4) return CDC_E_CORRUPT;
    const uint32_t magic = ld32u(f);
    if (magic == 0x184C2102u || (magic & 0xFFFFFFF0u) == 0x184D2A50u) return CDC_E_UNSUPPORTED;  // legacy, skippable
    if (magic != 0x184D2204u || n < 7) return CDC_E_CORRUPT;
    const uint32_t flg = f[4], bd = f[5];
    if ((flg >> 6) != 1u || (flg & 2u) || (bd & 0x8Fu) || (bd >> 4) < 4u) return CDC_E_CORRUPT;
    F.bchk = flg & 16u;
    F.csize = flg & 8u;
    F.cchk = flg & 4u;
    F.bmax = 1u << (8 + 2 * (bd >> 4));
    F.hlen = 7 + (F.csize ? 8 : 0) + ((flg & 1u) ? 4 : 0);
    if (n < F.hlen) return CDC_E_CORRUPT;
    if (f[F.hlen - 1] != ((xxh_finish(0, 0, 0, 0, f + 4, F.hlen - 5) >> 8) & 255u)) return CDC_E_CORRUPT;
    if (!(flg & 32u) || (flg & 1u)) return CDC_E_UNSUPPORTED;  // linked blocks, dictionary
    F.content = F.csize ? uint64_t(ld32u(f + 6)) | uint64_t(ld32u(f + 10)) << 32 : 0;
    return CDC_OK;
}

// The frame f[0, flen): sizing (dst == nullptr) or emitting into dst[0, cap).
__device__ int32_t wave_frame(const uint8_t *f, uint64_t flen, uint8_t *dst, uint64_t cap, uint32_t lane,
                              uint64_t &total)
{
    total = 0;
    if (flen == 0) return CDC_OK;  // InflateStream's empty-input rule (compression.go:108-116)
    FrameHdr F;
    const int32_t st = frame_header(f, flen, F);
    if (st != CDC_OK) return st;
    uint64_t pos = F.hlen, opos = 0;
    for (;;) {
        if (flen - pos < 4) return CDC_E_CORRUPT;
        const uint32_t word = ld32u(f + pos);
        pos += 4;
        if (word == 0) break;  // the end mark
        const uint32_t size = word & 0x7FFFFFFFu;
        const uint64_t need = uint64_t(size) + (F.bchk ? 4 : 0);
        if (size == 0 || size > F.bmax || flen - pos < need) return CDC_E_CORRUPT;
        const uint32_t omax = dst ? uint32_t(min<uint64_t>(F.bmax, cap - opos)) : F.bmax;
        int64_t d;
        if (word >> 31) {  // stored
            if (size > omax) return CDC_E_CORRUPT;
            if (dst) copy_exact(dst + opos, f + pos, size, lane, 64);
            d = size;
        } else {
            d = wave_block(f + pos, size, dst ? dst + opos : nullptr, omax, lane);
            if (d < 0) return CDC_E_CORRUPT;
        }
        if (!dst && F.bchk && wave_xxh32(f + pos, size, lane) != ld32u(f + pos + size)) return CDC_E_CORRUPT;
        pos += need;
        opos += uint64_t(d);
        if (opos > 0xFFFFFFFFull) return CDC_E_UNSUPPORTED;  // a blob is a cdc_cut: 32-bit length
    }
    uint32_t want = 0;
    if (F.cchk) {
        if (flen - pos < 4) return CDC_E_CORRUPT;
        want = ld32u(f + pos);
        pos += 4;
    }
    if (pos != flen) return CDC_E_CORRUPT;  // bytes after the frame
    if (F.csize && opos != F.content) return CDC_E_CORRUPT;
    if (dst) {
        if (opos != cap) return CDC_E_CORRUPT;  // not what the sizing pass saw
        if (F.cchk) {
            wave_publish();
            if (wave_xxh32(dst, opos, lane) != want) return CDC_E_CORRUPT;
        }
    }
    total = opos;
    return CDC_OK;
}

constexpr uint32_t kFrameWaves = 4;

__global__ __launch_bounds__(kFrameWaves * 64) void k_lz4_size(const DBatch B)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kFrameWaves + (threadIdx.x >> 6);
    if (b >= B.n) return;
    uint64_t total = 0;
    if (B.status[b] == 0) {
        const DBlob D = B.blobs[b];
        const int32_t st = wave_frame(stream_ptr(B, D), D.flen, nullptr, 0, lane, total);
        if (st != CDC_OK) {
            total = 0;
            if (lane == 0) B.status[b] = st;
        }
    }
    if (lane == 0) B.dsize[b] = total;
}

__global__ __launch_bounds__(kFrameWaves * 64) void k_lz4_emit(const DBatch B)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kFrameWaves + (threadIdx.x >> 6);
    if (b >= B.n || B.flags[kFlagNoSpace] || B.status[b]) return;
    const DBlob D = B.blobs[b];
    uint64_t total;
    const int32_t st = wave_frame(stream_ptr(B, D), D.flen, B.out + B.out_off[b], B.dsize[b], lane, total);
    if (st != CDC_OK && lane == 0) {
        B.status[b] = st;
        B.flags[kFlagLate] = 1;
    }
}

// ---------------------------------------------------------------------------
// f. The gzip member (compressed == CDC_COMPRESS_GZIP), one wave per blob.
// inflate_walk.h decides every bound; what is here is where the bytes go.
// ---------------------------------------------------------------------------
constexpr uint32_t kGzWaves = 4;

__device__ __forceinline__ int32_t gz_status(int st)
{
    return st == infw::kOk ? CDC_OK : st == infw::kUnsupported ? CDC_E_UNSUPPORTED : CDC_E_CORRUPT;
}

// The wave's lanes share a table build; LDS traffic of one wave stays in
// order, so the barrier only has to hold the compiler.
struct WavePar {
    uint32_t lane;
    static constexpr uint32_t nl = 64;
    __device__ __forceinline__ void sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
};

// Literals wait one per lane and leave as one store; a match gathers from the
// output in global memory (flushed literals included) and waits for the wave's
// own stores only when it reaches into bytes stored since the last wait.
struct GzSink {
    uint8_t *dst;
    const uint8_t *src;
    uint32_t lane, pend, fbase, published, litv;
    __device__ __forceinline__ void flush()
    {
        if (pend) {
            if (lane < pend) dst[fbase + lane] = uint8_t(litv);
            pend = 0;
        }
    }
    __device__ __forceinline__ void lit(uint32_t o, uint32_t b)
    {
        if (pend == 0) fbase = o;
        litv = lane == pend ? b : litv;  // a select at a uniform index: lane `pend` keeps the byte
        if (++pend == 64) flush();
    }
    __device__ __forceinline__ void match(uint32_t o, uint32_t dist, uint32_t len)
    {
        flush();
        if (o - dist + min(dist, len) > published) {
            wave_publish();
            published = o;
        }
        for (uint32_t i = lane; i < len; i += 64) dst[o + i] = dst[lz4w::match_src(o, dist, len, i)];
    }
    __device__ __forceinline__ void stored(uint32_t o, uint32_t s, uint32_t len)
    {
        flush();
        copy_exact(dst + o, src + s, len, lane, 64);
    }
};

// CRC-32 of p[0, n) by one wave: every lane runs the byte table (T, in LDS)
// over its slice, and the 64 registers fold in six steps, the left half of
// each pair multiplied by x^(8 * the right half's bytes) mod P.
__device__ uint32_t wave_crc32(const uint8_t *p, uint64_t n, uint32_t lane, const uint32_t *T)
{
    if (n == 0) return 0;
    uint64_t lo, hi;
    uint32_t reg;
    infw::crc_slice(n, lane, lo, hi, reg);
    uint64_t i = lo;
    for (; i + 16 <= hi; i += 16) {
        uint32_t w[4];
        __builtin_memcpy(w, p + i, 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            reg ^= w[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) reg = T[reg & 255u] ^ (reg >> 8);
        }
    }
    for (; i < hi; ++i) reg = T[(reg ^ p[i]) & 255u] ^ (reg >> 8);
    uint32_t M = infw::crc_xpow(8u * infw::crc_slice_len(n));
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t right = __shfl_down(reg, d);
        reg = infw::crc_mul(reg, M) ^ right;
        M = infw::crc_mul(M, M);
    }
    return uint32_t(__builtin_amdgcn_readfirstlane(int(reg))) ^ 0xFFFFFFFFu;
}

// Sizing does not inflate: the header, the trailer's place, ISIZE as the
// claim, and the 1032 : 1 ceiling.  Emit proves the claim.
__global__ __launch_bounds__(kGzWaves * 64) void k_gz_size(const DBatch B)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kGzWaves + (threadIdx.x >> 6);
    if (b >= B.n) return;
    uint32_t claim = 0;
    if (B.status[b] == 0) {
        const DBlob D = B.blobs[b];
        const uint32_t n = uint32_t(min<uint64_t>(D.flen, infw::kMaxStream));
        WaveRd rd{stream_ptr(B, D), n, lane, n, 0u};
        uint32_t hlen;
        const int st = infw::member_claim(rd, D.flen, hlen, claim);
        if (st != infw::kOk) {
            claim = 0;
            if (lane == 0) B.status[b] = gz_status(st);
        }
    }
    if (lane == 0) B.dsize[b] = claim;
}

__global__ __launch_bounds__(kGzWaves * 64) void k_gz_emit(const DBatch B)
{
    __shared__ infw::Tables s_fixed;
    __shared__ infw::Tables s_dyn[kGzWaves];
    __shared__ uint32_t s_crc[256];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    WavePar par{lane};
    if (wv == 0) infw::build_fixed(par, s_fixed);
    for (uint32_t i = threadIdx.x; i < 256; i += kGzWaves * 64) s_crc[i] = infw::crc_bits(0, i);
    __syncthreads();
    const uint32_t b = blockIdx.x * kGzWaves + wv;
    if (b >= B.n || B.flags[kFlagNoSpace] || B.status[b]) return;
    const DBlob D = B.blobs[b];
    if (D.flen == 0 || D.flen > infw::kMaxStream) return;  // the empty blob (sizing refused the other)
    const uint32_t n = uint32_t(D.flen), claim = uint32_t(B.dsize[b]);
    const uint8_t *f = stream_ptr(B, D);
    uint8_t *dst = B.out + B.out_off[b];
    WaveRd rd{f, n, lane, n, 0u};
    uint32_t hlen = 0, opos = 0, end = 0;
    int st = infw::member_header(rd, n, hlen);  // again: nothing is taken from the sizing pass but the claim
    if (st == infw::kOk) {
        GzSink sink{dst, f, lane, 0u, 0u, 0u, 0u};
        st = infw::inflate_body(rd, n, hlen, sink, claim, s_dyn[wv], s_fixed, par, opos, end);
    }
    if (st == infw::kOk) {
        wave_publish();
        st = infw::member_trailer(rd, n, end, opos, wave_crc32(dst, opos, lane, s_crc));
    }
    if (st == infw::kOk && opos != claim) st = infw::kCorrupt;
    if (st != infw::kOk && lane == 0) {
        B.status[b] = gz_status(st);
        B.flags[kFlagLate] = 1;
    }
}

// ---------------------------------------------------------------------------
// g. Prefix Decode (cdc_decode_prefix_device): the first upto[b] plaintext
// bytes of blob b, one wave per blob, no sizing pass.  B.dsize holds upto and
// B.out_off the host's exclusive sum of it, both staged before the launch.
// The walkers run in their stop mode (lz4w::next_seq_stop, infw::
// inflate_body_stop), which cuts the sequence that crosses upto to the byte,
// so blob b writes B.out + [out_off[b], out_off[b] + upto[b]) and nothing
// else.  Only a walk that reaches the stream's end verifies what lies there.
// ---------------------------------------------------------------------------
__device__ int64_t wave_block_prefix(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t omax, uint32_t stop,
                                     uint32_t lane, bool &stopped)
{
    WaveRd rd{src, n, lane, n, 0u};
    uint32_t ip = 0, opos = 0, published = 0;
    for (;;) {
        lz4w::Seq s;
        const int r = lz4w::next_seq_stop(rd, n, ip, opos, omax, stop, s);
        if (r < 0) return -1;
        if (s.lit_len) copy_exact(dst + opos, src + s.lit_src, s.lit_len, lane, 64);
        opos += s.lit_len;
        if (r == lz4w::kEnd) return int64_t(opos);
        if (s.mlen) {
            if (opos - s.off + min(s.off, s.mlen) > published) {
                wave_publish();
                published = opos;
            }
            if (s.off >= s.mlen) {
                copy_exact(dst + opos, dst + opos - s.off, s.mlen, lane, 64);
            } else {
                for (uint32_t i = lane; i < s.mlen; i += 64) dst[opos + i] = dst[lz4w::match_src(opos, s.off, s.mlen, i)];
            }
        }
        opos += s.mlen;
        if (r == lz4w::kStop) {
            stopped = true;
            return int64_t(opos);
        }
    }
}

// The first upto (> 0) bytes of the frame f[0, flen) into dst[0, upto).
__device__ int32_t wave_frame_prefix(const uint8_t *f, uint64_t flen, uint8_t *dst, uint64_t upto, uint32_t lane)
{
    if (flen == 0) return CDC_E_MISMATCH;  // the empty blob ends before any byte
    FrameHdr F;
    const int32_t st = frame_header(f, flen, F);
    if (st != CDC_OK) return st;
    uint64_t pos = F.hlen, opos = 0;
    for (;;) {
        // Everything wanted is out at a block's edge: only an end mark right
        // here makes this the whole stream, anything else is left unread.
        if (opos == upto && (flen - pos < 4 || ld32u(f + pos) != 0)) return CDC_OK;
        if (flen - pos < 4) return CDC_E_CORRUPT;
        const uint32_t word = ld32u(f + pos);
        pos += 4;
        if (word == 0) break;
        const uint32_t size = word & 0x7FFFFFFFu;
        if (size == 0 || size > F.bmax || flen - pos < size) return CDC_E_CORRUPT;
        const uint32_t stop = uint32_t(min<uint64_t>(F.bmax, upto - opos));
        bool stopped = false;
        int64_t d;
        if (word >> 31) {  // stored
            d = min(size, stop);
            copy_exact(dst + opos, f + pos, uint64_t(d), lane, 64);
            stopped = size > stop;
        } else {
            d = wave_block_prefix(f + pos, size, dst + opos, F.bmax, stop, lane, stopped);
            if (d < 0) return CDC_E_CORRUPT;
        }
        opos += uint64_t(d);
        if (stopped) return CDC_OK;
        if (F.bchk && (flen - pos - size < 4 || wave_xxh32(f + pos, size, lane) != ld32u(f + pos + size)))
            return CDC_E_CORRUPT;
        pos += uint64_t(size) + (F.bchk ? 4 : 0);
    }
    // the stream's end: what cdc_decode_device verifies there
    uint32_t want = 0;
    if (F.cchk) {
        if (flen - pos < 4) return CDC_E_CORRUPT;
        want = ld32u(f + pos);
        pos += 4;
    }
    if (pos != flen) return CDC_E_CORRUPT;
    if (F.csize && opos != F.content) return CDC_E_CORRUPT;
    if (F.cchk) {
        wave_publish();
        if (wave_xxh32(dst, opos, lane) != want) return CDC_E_CORRUPT;
    }
    return opos == upto ? CDC_OK : CDC_E_MISMATCH;  // it ended before upto
}

__global__ __launch_bounds__(kFrameWaves * 64) void k_lz4_prefix(const DBatch B)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * kFrameWaves + (threadIdx.x >> 6);
    if (b >= B.n || B.status[b]) return;
    const DBlob D = B.blobs[b];
    const int32_t st = wave_frame_prefix(stream_ptr(B, D), D.flen, B.out + B.out_off[b], B.dsize[b], lane);
    if (st != CDC_OK && lane == 0) B.status[b] = st;
}

// Five waves per SIMD, as k_gz_emit has them: the stop tests cost nine more
// registers than its 96 unless the compiler is held to that budget (no spill).
__global__ __launch_bounds__(kGzWaves * 64) __attribute__((amdgpu_waves_per_eu(5))) void k_gz_prefix(const DBatch B)
{
    __shared__ infw::Tables s_fixed;
    __shared__ infw::Tables s_dyn[kGzWaves];
    __shared__ uint32_t s_crc[256];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    WavePar par{lane};
    if (wv == 0) infw::build_fixed(par, s_fixed);
    for (uint32_t i = threadIdx.x; i < 256; i += kGzWaves * 64) s_crc[i] = infw::crc_bits(0, i);
    __syncthreads();
    const uint32_t b = blockIdx.x * kGzWaves + wv;
    if (b >= B.n || B.status[b]) return;
    const DBlob D = B.blobs[b];
    const uint32_t upto = uint32_t(B.dsize[b]);  // 0 < upto < 2^32: the host checked
    int32_t res = CDC_OK;
    if (D.flen == 0) {
        res = CDC_E_MISMATCH;  // the empty blob ends before any byte
    } else if (D.flen > infw::kMaxStream) {
        res = CDC_E_UNSUPPORTED;
    } else {
        const uint32_t n = uint32_t(D.flen);
        const uint8_t *f = stream_ptr(B, D);
        uint8_t *dst = B.out + B.out_off[b];
        WaveRd rd{f, n, lane, n, 0u};
        uint32_t hlen = 0, opos = 0, end = 0;
        bool stopped = false;
        int st = infw::member_header(rd, n, hlen);
        if (st == infw::kOk) {
            GzSink sink{dst, f, lane, 0u, 0u, 0u, 0u};
            st = infw::inflate_body_stop(rd, n, hlen, sink, upto, s_dyn[wv], s_fixed, par, opos, end, stopped);
        }
        if (st == infw::kOk && !stopped) {  // the stream's end: the trailer against what is out
            wave_publish();
            st = infw::member_trailer(rd, n, end, opos, wave_crc32(dst, opos, lane, s_crc));
        }
        res = gz_status(st);
        if (res == CDC_OK && opos != upto) res = CDC_E_MISMATCH;  // it ended before upto
    }
    if (res != CDC_OK && lane == 0) B.status[b] = res;
}

// Not compressed: the first upto bytes of the blob, or of its opened records.
__global__ __launch_bounds__(256) void k_prefix_copy(const DBatch B)
{
    const uint32_t b = blockIdx.x;
    if (B.status[b]) return;
    copy_exact(B.out + B.out_off[b], stream_ptr(B, B.blobs[b]), B.dsize[b], threadIdx.x, blockDim.x);
}

// ---------------------------------------------------------------------------
// The plan: out_off = exclusive scan of the sizes of the blobs that decoded.
// ---------------------------------------------------------------------------
constexpr uint32_t kPlanThreads = 1024;

__global__ __launch_bounds__(kPlanThreads) void k_dec_plan(const DBatch B)
{
    __shared__ uint64_t s_w[kPlanThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t per = (B.n + kPlanThreads - 1) / kPlanThreads;
    const uint32_t b0 = min(B.n, t * per), b1 = min(B.n, b0 + per);
    auto size_of = [&](uint32_t b) -> uint64_t {
        return B.status[b] ? 0 : B.compressed ? B.dsize[b] : B.blobs[b].flen;
    };
    uint64_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b) sum += size_of(b);
    uint64_t inc = sum;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint64_t off = inc - sum;
    for (uint32_t i = 0; i < wv; ++i) off += s_w[i];
    for (uint32_t b = b0; b < b1; ++b) {
        B.out_off[b] = off;
        off += size_of(b);
    }
    if (t == kPlanThreads - 1) {
        B.out_off[B.n] = off;
        if (off > B.out_cap) B.flags[kFlagNoSpace] = 1;
    }
}

// A content checksum failed after the plan (kFlagLate): the blobs after it
// move down, in order (a later blob's new place may overlap an earlier one's
// old place).  Rare, so one workgroup does it all, at about 10 GiB/s
// (DESIGN.md 5.10 has the worst case).
__global__ __launch_bounds__(256) void k_dec_compact(const DBatch B)
{
    if (!B.flags[kFlagLate] || B.flags[kFlagNoSpace]) return;
    const uint32_t t = threadIdx.x;
    uint64_t oldo = 0, newo = 0;
    for (uint32_t b = 0; b < B.n; ++b) {
        const uint64_t next = B.out_off[b + 1];
        const uint64_t sz = B.status[b] ? 0 : next - oldo;
        if (sz && newo != oldo) {
            // 4-KiB pieces in ascending order: all of a piece is read before any of it is written
            for (uint64_t c = 0; c < sz; c += 4096) {
                const uint32_t m = uint32_t(min<uint64_t>(4096, sz - c));
                uint4 v = make_uint4(0, 0, 0, 0);
                uint8_t tail = 0;
                const uint32_t nq = m / 16;
                if (t < nq) __builtin_memcpy(&v, B.out + oldo + c + 16 * t, 16);
                if (t < m - 16 * nq) tail = B.out[oldo + c + 16 * nq + t];
                __syncthreads();
                if (t < nq) __builtin_memcpy(B.out + newo + c + 16 * t, &v, 16);
                if (t < m - 16 * nq) B.out[newo + c + 16 * nq + t] = tail;
                __syncthreads();
            }
        }
        __syncthreads();  // everyone has read out_off[b + 1]
        if (t == 0) B.out_off[b] = newo;
        newo += sz;
        oldo = next;
    }
    if (t == 0) B.out_off[B.n] = newo;
}

__global__ __launch_bounds__(256) void k_dec_copy(const DBatch B)
{
    const uint32_t b = blockIdx.x;
    if (B.flags[kFlagNoSpace] || B.status[b]) return;
    copy_exact(B.out + B.out_off[b], B.in + B.blobs[b].src, B.blobs[b].len, threadIdx.x, blockDim.x);
}

// cdc_check_device: row i of `got` against row i of `want` (32 bytes each).
__global__ __launch_bounds__(256) void k_check_cmp(const uint8_t *got, const uint8_t *want, uint32_t *differs, uint32_t m)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint32_t d = 0;
    for (uint32_t k = 0; k < 32; ++k) d |= uint32_t(got[32ull * i + k] ^ want[32ull * i + k]);
    differs[i] = d;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static cdc::AesTables g_tab;

// Workspace kept per device between calls (grow-only); a call holds its
// device's lock while it runs (the entry points are synchronous).
struct WsCache {
    std::mutex mu;
    cdc::DevBuf ws;
    cdc::PinBuf stage;  // pinned staging of the host plan
};
// One for Decode and one for the check, per device; never destroyed (DevBuf).
static WsCache *const g_ws = new WsCache[cdc::kMaxDevices], *const g_cws = new WsCache[cdc::kMaxDevices];

static bool bad_args(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                     const int32_t *status)
{
    return device < 0 || device >= cdc::kMaxDevices || (n && (!d_in || !offsets || !lens || !status));
}

// The hashing half of cdc_check_device, over blobs that cdc_decode_device left
// at d_scratch + oo[i] (n + 1 offsets): status[i] == CDC_OK becomes
// CDC_E_MISMATCH where the SHA-256 differs from checksums[32 i].  The plaintext
// is only read.  Synchronous on `stream`.
static int check_decoded(int device, const uint8_t *d_scratch, const uint64_t *oo, uint32_t n,
                         const uint8_t *checksums, int32_t *status, void *stream, const uint8_t *only = nullptr)
{
    // only != NULL: blob b is hashed and compared where only[b] != 0, and left alone elsewhere
    auto checked = [&](uint32_t b) { return status[b] == CDC_OK && (!only || only[b]); };
    int st;
    // SHA-256 of every blob on the device (k_chunk_digest hashes an empty chunk
    // to SHA-256("")); a blob that did not decode is an empty cut whose row is
    // ignored.  Empty cuts sit at offset 0, and when nothing decoded at all
    // the hashed buffer is 16 bytes of the workspace, not the caller's.
    const size_t m = n;
    cdc::Carver cv(16);
    const size_t o_cuts = cv.take(m * sizeof(cdc_cut)), o_want = cv.take(m * 32), h_bytes = cv.bytes();
    const size_t o_got = cv.take(m * 32), o_diff = cv.take(m * 4), o_dummy = cv.take(16);
    WsCache &C = g_cws[device];
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.ws.reserve(cv.bytes()) || !C.stage.reserve(h_bytes + m * 4)) return CDC_E_NOMEM;
    uint8_t *const ws = C.ws.as<uint8_t>(), *const hp = C.stage.as<uint8_t>();
    cdc_cut *cuts = reinterpret_cast<cdc_cut *>(hp + o_cuts);
    for (uint32_t b = 0; b < n; ++b) {
        const uint64_t len = checked(b) ? oo[b + 1] - oo[b] : 0;
        cuts[b] = cdc_cut{len ? oo[b] : 0, uint32_t(len), 0};
    }
    std::memcpy(hp + o_want, checksums, m * 32);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemcpyAsync(ws, hp, h_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return CDC_E_DEVICE;
    st = cdc_chunk_digests_device_async(device, oo[n] ? d_scratch : ws + o_dummy, oo[n],
                                        reinterpret_cast<const cdc_cut *>(ws + o_cuts), m, nullptr, ws + o_got,
                                        nullptr, stream);
    if (st != CDC_OK) return st;
    hipLaunchKernelGGL(k_check_cmp, dim3(uint32_t((m + 255) / 256)), dim3(256), 0, s, ws + o_got, ws + o_want,
                       reinterpret_cast<uint32_t *>(ws + o_diff), uint32_t(m));
    uint32_t *diff = reinterpret_cast<uint32_t *>(hp + h_bytes);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(diff, ws + o_diff, m * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return CDC_E_DEVICE;
    for (uint32_t b = 0; b < n; ++b)
        if (checked(b) && diff[b]) status[b] = CDC_E_MISMATCH;
    return CDC_OK;
}

// What the host plan takes from one blob's length: its records as the length
// counts them (nr; a blob that is not CDC_OK opens none of them), its frame
// bytes and the bytes of its frame slot.
struct BlobPlan {
    uint64_t nr, flen, slot;
    int32_t status;
};
static BlobPlan plan_blob(uint64_t len, bool encrypt, int compressed)
{
    BlobPlan P{0, len, 0, CDC_OK};
    if (!encrypt) return P;
    P.flen = 0;
    if (len < kHdr) {
        P.status = CDC_E_CORRUPT;
        return P;
    }
    const uint64_t rem = len - kHdr, nr = (rem + kRecMax - 1) / kRecMax;
    P.nr = nr;
    if (nr && rem - (nr - 1) * kRecMax < 28) P.status = CDC_E_CORRUPT;  // a trailing record too short for a nonce and a tag
    else P.flen = rem - 28 * nr;
    if (compressed) P.slot = cdc::align_up(rem - std::min<uint64_t>(rem, 28 * nr), 16);
    return P;
}

// The host plan of a prefix: what cdc_decode_device plans from the lengths,
// narrowed by upto.  A blob with upto == 0 is kSkip (nothing of it is read;
// reported as CDC_OK); without compression only the records that hold the
// prefix are opened, and they land in a frame slot that k_prefix_copy reads.
constexpr int32_t kSkip = 1;
struct PrefixPlan {
    uint64_t nr, flen, slot;
    int32_t status;
};
static PrefixPlan plan_prefix(uint64_t len, uint64_t upto, bool encrypt, int compressed)
{
    if (upto == 0) return PrefixPlan{0, 0, 0, kSkip};
    if (upto > 0xFFFFFFFFull) return PrefixPlan{0, 0, 0, CDC_E_UNSUPPORTED};  // a blob is a cdc_cut: 32-bit length
    const BlobPlan P = plan_blob(len, encrypt, compressed);
    if (P.status != CDC_OK) return PrefixPlan{0, 0, 0, P.status};
    if (compressed) return PrefixPlan{P.nr, P.flen, P.slot, CDC_OK};
    if (upto > P.flen) return PrefixPlan{0, 0, 0, CDC_E_MISMATCH};
    if (!encrypt) return PrefixPlan{0, P.flen, 0, CDC_OK};
    const uint64_t nr = (upto + kPiece - 1) / kPiece;
    return PrefixPlan{nr, P.flen, cdc::align_up(std::min<uint64_t>(P.flen, nr * kPiece), 16), CDC_OK};
}

}  // namespace dec

using namespace dec;

extern "C" int cdc_decode_prefix_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                                        const uint64_t *upto, uint32_t n, int compressed, const uint8_t *key,
                                        uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets, int32_t *status,
                                        void *stream)
{
    if (bad_args(device, d_in, offsets, lens, n, status) || (n && !upto) || !out_offsets || (!d_out && out_cap))
        return CDC_E_INVALID;
    uint64_t total = 0;
    for (uint32_t b = 0; b < n; ++b) {
        out_offsets[b] = total;
        if (upto[b] > UINT64_MAX - total) return CDC_E_INVALID;
        total += upto[b];
    }
    out_offsets[n] = total;
    if (total > out_cap) return CDC_E_NOSPACE;
    const bool encrypt = key != nullptr;
    uint64_t slot = 0, nrecs = 0;
    for (uint32_t b = 0; b < n; ++b) {
        const PrefixPlan P = plan_prefix(lens[b], upto[b], encrypt, compressed);
        status[b] = P.status == kSkip ? CDC_OK : P.status;
        nrecs += P.nr;
        slot += P.slot;
    }
    if (total == 0) return CDC_OK;  // nothing is wanted: nothing is read
    if (nrecs > 0x7FFFFFFFull) return CDC_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    int st = cdc::upload_aes_tables(g_tab, g_te0, g_sbox);
    if (st != CDC_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t nb = n;
    cdc::Carver cv(16);
    // the staged prefix (blobs, status, key, upto, offsets), then what only the device touches
    const size_t o_blobs = cv.take(nb * sizeof(DBlob)), o_status = cv.take(nb * 4), o_key = cv.take(32),
                 o_dsize = cv.take(nb * 8), o_oo = cv.take((nb + 1) * 8), h_prefix = cv.bytes();
    const size_t o_keys = cv.take(encrypt ? nb * sizeof(BlobKey) : 0), o_flags = cv.take(16),
                 o_frames = cv.take(encrypt ? slot : 0);
    WsCache &C = g_ws[device];
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.ws.reserve(cv.bytes()) || !C.stage.reserve(h_prefix)) return CDC_E_NOMEM;
    const int cus = cdc::device_cus(device);
    uint8_t *const ws = C.ws.as<uint8_t>(), *const hp = C.stage.as<uint8_t>();
    {
        DBlob *blobs = reinterpret_cast<DBlob *>(hp + o_blobs);
        int32_t *hst = reinterpret_cast<int32_t *>(hp + o_status);
        uint64_t sl = 0;
        uint32_t rec = 0;
        for (uint32_t b = 0; b < n; ++b) {
            const PrefixPlan P = plan_prefix(lens[b], upto[b], encrypt, compressed);
            DBlob D{};
            D.src = offsets[b];
            D.len = lens[b];
            D.flen = P.flen;
            D.rec0 = rec;
            D.nrec = uint32_t(P.nr);
            D.slot = sl;
            hst[b] = P.status;
            sl += P.slot;
            rec += D.nrec;
            blobs[b] = D;
        }
        std::memcpy(hp + o_dsize, upto, nb * 8);
        std::memcpy(hp + o_oo, out_offsets, (nb + 1) * 8);
        if (encrypt) std::memcpy(hp + o_key, key, 32);
    }
    DBatch B{};
    B.in = static_cast<const uint8_t *>(d_in);
    B.n = n;
    B.compressed = compressed == CDC_COMPRESS_GZIP ? 2u : compressed ? 1u : 0u;
    B.encrypted = encrypt ? 1u : 0u;
    B.nrecs = uint32_t(nrecs);
    B.blobs = reinterpret_cast<const DBlob *>(ws + o_blobs);
    B.key = ws + o_key;
    B.frames = ws + o_frames;
    B.out = d_out;
    B.out_cap = out_cap;
    B.keys = reinterpret_cast<BlobKey *>(ws + o_keys);
    B.status = reinterpret_cast<int32_t *>(ws + o_status);
    B.dsize = reinterpret_cast<uint64_t *>(ws + o_dsize);
    B.out_off = reinterpret_cast<uint64_t *>(ws + o_oo);
    B.flags = reinterpret_cast<uint32_t *>(ws + o_flags);
    bool ok = hipMemcpyAsync(ws, hp, h_prefix, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemsetAsync(ws + o_flags, 0, 16, s) == hipSuccess;
    if (ok) {
        if (encrypt) {
            const uint32_t open_wgs = uint32_t(std::min<uint64_t>((nrecs + kGcmWaves - 1) / kGcmWaves, uint64_t(cus)));
            hipLaunchKernelGGL(k_dec_keys, dim3((n + kKeyThreads - 1) / kKeyThreads), dim3(kKeyThreads), 0, s, B);
            hipLaunchKernelGGL(k_dec_pows, dim3((n + kPowWaves - 1) / kPowWaves), dim3(kPowWaves * 64), 0, s, B);
            if (nrecs)
                hipLaunchKernelGGL(k_rec_open, dim3(open_wgs), dim3(kGcmWaves * 64), 0, s, B, kOpenHash | kOpenCtr);
        }
        if (B.compressed == 2u)
            hipLaunchKernelGGL(k_gz_prefix, dim3((n + kGzWaves - 1) / kGzWaves), dim3(kGzWaves * 64), 0, s, B);
        else if (B.compressed)
            hipLaunchKernelGGL(k_lz4_prefix, dim3((n + kFrameWaves - 1) / kFrameWaves), dim3(kFrameWaves * 64), 0, s, B);
        else
            hipLaunchKernelGGL(k_prefix_copy, dim3(n), dim3(256), 0, s, B);
        ok = hipGetLastError() == hipSuccess;
    }
    // the repository key does not outlive the call (see cdc_decode_device)
    if (encrypt) ok = ok && hipMemsetAsync(ws + o_key, 0, 32, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(status, ws + o_status, nb * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    if (encrypt) std::memset(hp + o_key, 0, 32);
    if (!ok) return CDC_E_DEVICE;
    for (uint32_t b = 0; b < n; ++b)
        if (status[b] == kSkip) status[b] = CDC_OK;
    return CDC_OK;
}

extern "C" int cdc_decode_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                                 uint32_t n, int compressed, const uint8_t *key, uint8_t *d_out, uint64_t out_cap,
                                 uint64_t *out_offsets, int32_t *status, void *stream)
{
    if (bad_args(device, d_in, offsets, lens, n, status) || !out_offsets || (!d_out && out_cap)) return CDC_E_INVALID;
    if (n == 0) {
        out_offsets[0] = 0;
        return CDC_OK;
    }
    const bool encrypt = key != nullptr;
    // plan on the host: records and frame slots follow from the lengths
    uint64_t slot = 0, nrecs = 0;
    for (uint32_t b = 0; b < n; ++b) {
        const BlobPlan P = plan_blob(lens[b], encrypt, compressed);
        nrecs += P.nr;
        slot += P.slot;
    }
    if (nrecs > 0x7FFFFFFFull) return CDC_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    int st = cdc::upload_aes_tables(g_tab, g_te0, g_sbox);
    if (st != CDC_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t nb = n;
    cdc::Carver cv(16);
    // the staged prefix (blobs, status, key), then what only the device touches
    const size_t o_blobs = cv.take(nb * sizeof(DBlob)), o_status = cv.take(nb * 4), o_key = cv.take(32),
                 h_prefix = cv.bytes();
    const size_t o_keys = cv.take(encrypt ? nb * sizeof(BlobKey) : 0), o_dsize = cv.take(nb * 8),
                 o_oo = cv.take((nb + 1) * 8);
    const size_t o_flags = cv.take(16), o_frames = cv.take(encrypt && compressed ? slot : 0);
    WsCache &C = g_ws[device];
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.ws.reserve(cv.bytes()) || !C.stage.reserve(h_prefix)) return CDC_E_NOMEM;
    const int cus = cdc::device_cus(device);
    uint8_t *const ws = C.ws.as<uint8_t>(), *const hp = C.stage.as<uint8_t>();
    {
        DBlob *blobs = reinterpret_cast<DBlob *>(hp + o_blobs);
        int32_t *hst = reinterpret_cast<int32_t *>(hp + o_status);
        uint64_t sl = 0;
        uint32_t rec = 0;
        for (uint32_t b = 0; b < n; ++b) {
            const BlobPlan P = plan_blob(lens[b], encrypt, compressed);
            DBlob D{};
            D.src = offsets[b];
            D.len = lens[b];
            D.flen = P.flen;
            D.rec0 = rec;
            D.nrec = P.status == CDC_OK ? uint32_t(P.nr) : 0u;
            hst[b] = P.status;
            if (encrypt && compressed && lens[b] >= kHdr) D.slot = sl;
            sl += P.slot;
            rec += D.nrec;
            blobs[b] = D;
        }
        nrecs = rec;
        if (encrypt) std::memcpy(hp + o_key, key, 32);
    }
    DBatch B{};
    B.in = static_cast<const uint8_t *>(d_in);
    B.n = n;
    B.compressed = compressed == CDC_COMPRESS_GZIP ? 2u : compressed ? 1u : 0u;
    B.encrypted = encrypt ? 1u : 0u;
    B.nrecs = uint32_t(nrecs);
    B.blobs = reinterpret_cast<const DBlob *>(ws + o_blobs);
    B.key = ws + o_key;
    B.frames = ws + o_frames;
    B.out = d_out;
    B.out_cap = out_cap;
    B.keys = reinterpret_cast<BlobKey *>(ws + o_keys);
    B.status = reinterpret_cast<int32_t *>(ws + o_status);
    B.dsize = reinterpret_cast<uint64_t *>(ws + o_dsize);
    B.out_off = reinterpret_cast<uint64_t *>(ws + o_oo);
    B.flags = reinterpret_cast<uint32_t *>(ws + o_flags);
    const uint32_t open_wgs = uint32_t(std::min<uint64_t>((nrecs + kGcmWaves - 1) / kGcmWaves, uint64_t(cus)));
    const dim3 frame_grid((n + kFrameWaves - 1) / kFrameWaves);
    bool ok = hipMemcpyAsync(ws, hp, h_prefix, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemsetAsync(ws + o_flags, 0, 16, s) == hipSuccess;
    if (ok) {
        if (encrypt) {
            hipLaunchKernelGGL(k_dec_keys, dim3((n + kKeyThreads - 1) / kKeyThreads), dim3(kKeyThreads), 0, s, B);
            hipLaunchKernelGGL(k_dec_pows, dim3((n + kPowWaves - 1) / kPowWaves), dim3(kPowWaves * 64), 0, s, B);
            if (nrecs)
                hipLaunchKernelGGL(k_rec_open, dim3(open_wgs), dim3(kGcmWaves * 64), 0, s, B,
                                   compressed ? (kOpenHash | kOpenCtr) : kOpenHash);
        }
        const bool gzip = B.compressed == 2u;
        const dim3 gz_grid((n + kGzWaves - 1) / kGzWaves);
        if (gzip) hipLaunchKernelGGL(k_gz_size, gz_grid, dim3(kGzWaves * 64), 0, s, B);
        else if (compressed) hipLaunchKernelGGL(k_lz4_size, frame_grid, dim3(kFrameWaves * 64), 0, s, B);
        hipLaunchKernelGGL(k_dec_plan, dim3(1), dim3(kPlanThreads), 0, s, B);
        if (compressed) {
            if (gzip) hipLaunchKernelGGL(k_gz_emit, gz_grid, dim3(kGzWaves * 64), 0, s, B);
            else hipLaunchKernelGGL(k_lz4_emit, frame_grid, dim3(kFrameWaves * 64), 0, s, B);
            hipLaunchKernelGGL(k_dec_compact, dim3(1), dim3(256), 0, s, B);
        } else if (encrypt) {
            if (nrecs)
                hipLaunchKernelGGL(k_rec_open, dim3(open_wgs), dim3(kGcmWaves * 64), 0, s, B, kOpenCtr | kOpenToOut);
        } else {
            hipLaunchKernelGGL(k_dec_copy, dim3(n), dim3(256), 0, s, B);
        }
        ok = hipGetLastError() == hipSuccess;
    }
    // The repository key does not outlive the call in the cached workspace or
    // its pinned staging (k_dec_keys, its only reader, is done by now on this
    // stream).  The blobs' own subkey schedules (BlobKey) stay in the workspace
    // until the next call overwrites them, as Encode's do: each opens one blob.
    if (encrypt) ok = ok && hipMemsetAsync(ws + o_key, 0, 32, s) == hipSuccess;
    uint32_t flags[4] = {0, 0, 0, 0};
    ok = ok && hipMemcpyAsync(out_offsets, ws + o_oo, (nb + 1) * 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipMemcpyAsync(status, ws + o_status, nb * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipMemcpyAsync(flags, ws + o_flags, 16, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    if (encrypt) std::memset(hp + o_key, 0, 32);
    if (!ok) return CDC_E_DEVICE;
    return flags[kFlagNoSpace] ? CDC_E_NOSPACE : CDC_OK;
}

extern "C" int cdc_check_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                                uint32_t n, int compressed, const uint8_t *key, const uint8_t *checksums,
                                uint8_t *d_scratch, uint64_t scratch_cap, uint64_t *needed, int32_t *status,
                                void *stream)
{
    if (bad_args(device, d_in, offsets, lens, n, status) || (n && !checksums) || (!d_scratch && scratch_cap))
        return CDC_E_INVALID;
    if (n == 0) {
        if (needed) *needed = 0;
        return CDC_OK;
    }
    std::vector<uint64_t> oo(size_t(n) + 1);
    int st = cdc_decode_device(device, d_in, offsets, lens, n, compressed, key, d_scratch, scratch_cap, oo.data(),
                               status, stream);
    if (needed) *needed = oo[n];
    if (st != CDC_OK) return st;
    return check_decoded(device, d_scratch, oo.data(), n, checksums, status, stream);
}

// cdc_restore.cpp's seam: Decode and, with checksums, the check, in one call
// that reports the offsets and the statuses and leaves the plaintext in d_out.
int cdc::decode_checked(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                        int compressed, const uint8_t *key, const uint8_t *checksums, uint8_t *d_out, uint64_t out_cap,
                        uint64_t *out_offsets, int32_t *status, void *stream, double *decode_s, double *verify_s)
{
    const auto t0 = std::chrono::steady_clock::now();
    int st = cdc_decode_device(device, d_in, offsets, lens, n, compressed, key, d_out, out_cap, out_offsets, status,
                               stream);
    const auto t1 = std::chrono::steady_clock::now();
    if (decode_s) *decode_s += std::chrono::duration<double>(t1 - t0).count();
    if (st != CDC_OK || !checksums || n == 0) return st;
    st = check_decoded(device, d_out, out_offsets, n, checksums, status, stream);
    if (verify_s) *verify_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return st;
}

// cdc_restore.cpp's seam for ranged reads: prefix Decode and, with checksums,
// the check of the blobs that were decoded whole.
int cdc::decode_prefix_checked(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                               const uint64_t *upto, uint32_t n, int compressed, const uint8_t *key,
                               const uint8_t *checksums, const uint8_t *whole, uint8_t *d_out, uint64_t out_cap,
                               uint64_t *out_offsets, int32_t *status, void *stream, double *decode_s, double *verify_s)
{
    const auto t0 = std::chrono::steady_clock::now();
    int st = cdc_decode_prefix_device(device, d_in, offsets, lens, upto, n, compressed, key, d_out, out_cap, out_offsets,
                                      status, stream);
    const auto t1 = std::chrono::steady_clock::now();
    if (decode_s) *decode_s += std::chrono::duration<double>(t1 - t0).count();
    if (st != CDC_OK || !checksums || !whole || n == 0) return st;
    bool any = false;
    for (uint32_t b = 0; b < n; ++b) any = any || (whole[b] && status[b] == CDC_OK);
    if (!any) return st;
    st = check_decoded(device, d_out, out_offsets, n, checksums, status, stream, whole);
    if (verify_s) *verify_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return st;
}
