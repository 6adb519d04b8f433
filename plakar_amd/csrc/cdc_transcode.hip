// Transcode on the device: what sync's synchronize() does to every blob the
// destination lacks (cmd/plakar/subcommands/sync/sync.go:182-266): GetBlob
// decodes it with the source repository's compression and key, PutBlob encodes
// it with the destination's.  cdc_transcode_device does that for a batch
// without the plaintext crossing PCIe, and, when both repositories name the
// same compression, without inflating at all: only the GCM envelope changes.
//
// The re-key path (same compression, both keys) is this file's own kernel:
//   k_tc_keys     one thread per blob: opens the source's sealed subkey (tag
//                 compared in full: CDC_E_AUTH), expands it and the
//                 destination's subkey (from `random`), both H and their 4-bit
//                 tables, and writes the destination's 60-byte header
//   k_tc_pows     one wave per blob and side: H^1..H^64, the 8-bit table of H^64
//   k_rekey       one wave per record nonce(12) || ciphertext || tag(16), in one
//                 pass: GHASH over the source ciphertext and the source tag
//                 compared in full, the source keystream and the destination
//                 keystream XORed in in registers, GHASH over the new
//                 ciphertext, and the new nonce, ciphertext and tag written to
//                 the same record position of the output blob
//   k_tc_compact  one workgroup, only when a tag failed: the blobs after a
//                 failed one move down, so that it contributes no bytes
//
// The plaintext never exists in HBM on this path.  It lives in VGPRs (one
// XOR between the two keystreams) and nowhere else; what passes through the
// wave's LDS stage is already the new ciphertext.  That is why the kernel is
// fused and not k_rec_open into a frame buffer followed by k_gcm, and why the
// workspace has no frame buffer.
//
// LDS: the 64-KiB T-table and, per wave, two key sets (rk, rk16, th, t64:
// 4,832 B each) and one 2-KiB stage: 65,536 + 8 x 11,712 = 159,232 B, so
// eight waves per workgroup, one workgroup per CU, two waves per SIMD (twelve
// waves would need 206,080 B of the CU's 160 KiB).
//
// The other paths are the existing Decode and Encode, called from here
// (transcode_plan.h chooses): see cdc_transcode_device at the end.
//
// Every read of d_in stays inside the blob it belongs to, and every write
// inside the blob's planned range of d_out: a record's place and length in
// the output are those it has in the input, both from the blob's length.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "cdc_crypto_dev.h"
#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "transcode_plan.h"

namespace tc {

using namespace devc;

constexpr uint32_t kRecMax = uint32_t(tplan::kRecMax);
constexpr uint32_t kHdr = uint32_t(tplan::kHdr);

// This file's own copies of the AES tables (no relocatable device code).
__device__ uint32_t g_te0[256];
__device__ uint8_t g_sbox[256];

struct RBlob {      // planned on the host from the lengths
    uint64_t src;   // byte offset in d_in
    uint64_t len;   // stored bytes, in and out
    uint32_t rec0, nrec;
};

struct RBatch {
    const uint8_t *in;
    uint8_t *out;
    uint32_t n, nrecs;
    const RBlob *blobs;
    const uint8_t *keys;  // source repository key (32 B), destination repository key (32 B)
    const uint8_t *rnd;   // per blob: subkey 32, subkey nonce 12, data nonce 12
    BlobKey *bk;          // per blob: [2 b] the source subkey's state, [2 b + 1] the destination's
    int32_t *status;      // per blob
    uint64_t *out_off;    // n + 1, planned on the host; k_tc_compact rewrites it
    uint32_t *flags;      // see kFlag*
};
constexpr uint32_t kFlagTicket = 0, kFlagFailed = 1;

__device__ __forceinline__ void nonce_words(const uint8_t *p, uint32_t (&j0)[3])
{
    for (int i = 0; i < 3; ++i)
        j0[i] = uint32_t(p[4 * i]) << 24 | uint32_t(p[4 * i + 1]) << 16 | uint32_t(p[4 * i + 2]) << 8 | p[4 * i + 3];
}

__device__ __forceinline__ void put_be32(uint8_t *o, uint32_t v)
{
    o[0] = uint8_t(v >> 24);
    o[1] = uint8_t(v >> 16);
    o[2] = uint8_t(v >> 8);
    o[3] = uint8_t(v);
}

// ---------------------------------------------------------------------------
// a. Key setup
// ---------------------------------------------------------------------------
constexpr uint32_t kKeyThreads = 64;
constexpr uint32_t kPowWaves = 4;

struct MasterKey {  // a repository key: its schedule and the 4-bit table of its H
    uint32_t rk[60];
    G128 th[16];
};

__device__ void master_setup(const uint8_t *key32, MasterKey &M, const uint32_t *te, const uint8_t *sb)
{
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = key32[i];
    aes256_expand(key, M.rk, sb);
    uint32_t z[4] = {0, 0, 0, 0};
    aes256_block(M.rk, te, sb, z);
    gtable(g_from_words(z), M.th);
}

// Seal(master, nonce j0, 32 bytes) both ways: AES-CTR over the two blocks at
// `in` (ciphertext when opening, plaintext when sealing) into out32, and the
// tag over the ciphertext.
__device__ G128 seal32(const MasterKey &M, const uint32_t (&j0)[3], const uint8_t *in, bool opening, uint8_t out32[32],
                       const uint32_t *te, const uint8_t *sb)
{
    G128 S = {0, 0};
    for (uint32_t i = 0; i < 2; ++i) {
        uint32_t iw[4];
        gcm_block_words(in + 16 * i, iw);
        uint32_t c[4] = {j0[0], j0[1], j0[2], 2 + i};
        aes256_block(M.rk, te, sb, c);
        uint32_t ow[4];
        for (int k = 0; k < 4; ++k) {
            ow[k] = c[k] ^ iw[k];
            put_be32(out32 + 16 * i + 4 * k, ow[k]);
        }
        S = gmul4(gx(S, g_from_words(opening ? iw : ow)), M.th);
    }
    S = gmul4(gx(S, G128{0, 256}), M.th);  // len(A) = 0, len(C) = 256 bits
    uint32_t tg[4] = {j0[0], j0[1], j0[2], 1};
    aes256_block(M.rk, te, sb, tg);
    return gx(S, g_from_words(tg));
}

// A subkey's state but the power ladder: round keys, H, its 4-bit table
// (rk and th: the calling thread's rows in LDS, not private memory).
__device__ void subkey_setup(const uint8_t sub[32], BlobKey &K, uint32_t *rk, G128 *th, const uint32_t *te,
                             const uint8_t *sb)
{
    aes256_expand(sub, rk, sb);
    for (int i = 0; i < 60; ++i) K.rk[i] = rk[i];
    uint32_t z[4] = {0, 0, 0, 0};
    aes256_block(rk, te, sb, z);
    const G128 H = g_from_words(z);
    K.hpow[0] = H;
    gtable(H, th);
    for (int i = 0; i < 16; ++i) K.th[i] = th[i];
}

__global__ __launch_bounds__(kKeyThreads) void k_tc_keys(const RBatch B)
{
    __shared__ uint32_t s_te[256];
    __shared__ uint8_t s_sb[256];
    __shared__ MasterKey s_m[2];
    __shared__ uint32_t s_rk[kKeyThreads][61];
    __shared__ G128 s_th[kKeyThreads][17];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < 256; i += kKeyThreads) {
        s_te[i] = g_te0[i];
        s_sb[i] = g_sbox[i];
    }
    __syncthreads();
    if (t < 2) master_setup(B.keys + 32 * t, s_m[t], s_te, s_sb);
    __syncthreads();
    const uint32_t b = blockIdx.x * kKeyThreads + t;
    if (b >= B.n || B.status[b]) return;
    const uint8_t *h = B.in + B.blobs[b].src;  // nonce 12, sealed subkey 32, tag 16 (len >= 60: the host checked)
    uint32_t j0[3];
    nonce_words(h, j0);
    uint8_t sub[32];
    const G128 got = seal32(s_m[0], j0, h + 12, true, sub, s_te, s_sb);
    uint32_t tw[4];
    gcm_block_words(h + 44, tw);
    const G128 want = g_from_words(tw);
    if ((want.hi ^ got.hi) | (want.lo ^ got.lo)) {  // all 16 bytes, no early exit
        B.status[b] = CDC_E_AUTH;
        B.flags[kFlagFailed] = 1;
        return;
    }
    subkey_setup(sub, B.bk[2 * b], s_rk[t], s_th[t], s_te, s_sb);
    const uint8_t *r = B.rnd + 56ull * b;
    subkey_setup(r, B.bk[2 * b + 1], s_rk[t], s_th[t], s_te, s_sb);
    // the destination's header: subkey nonce || Seal(destination key, subkey nonce, subkey)
    uint8_t *o = B.out + B.out_off[b];
    for (int i = 0; i < 12; ++i) o[i] = r[32 + i];
    nonce_words(r + 32, j0);
    uint8_t sealed[32];
    const G128 tag = seal32(s_m[1], j0, r, false, sealed, s_te, s_sb);
    for (int i = 0; i < 32; ++i) o[12 + i] = sealed[i];
    for (int k = 0; k < 8; ++k) {
        o[44 + k] = uint8_t(tag.hi >> (56 - 8 * k));
        o[52 + k] = uint8_t(tag.lo >> (56 - 8 * k));
    }
}

__global__ __launch_bounds__(kPowWaves * 64) void k_tc_pows(const RBatch B)
{
    __shared__ PowLds S[kPowWaves];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * kPowWaves + wv;  // blob i / 2, side i % 2
    if (i >= 2 * B.n || B.status[i >> 1]) return;
    hpow_ladder(B.bk[i], S[wv], lane);
}

// ---------------------------------------------------------------------------
// b. The fused record pass
// ---------------------------------------------------------------------------
constexpr uint32_t kRekeyWaves = 8;  // one workgroup per CU (LDS), two waves per SIMD

struct RekeyLds {
    uint32_t te[256 * 64];  // GcmLds's layout (cdc_crypto_dev.h)
    struct PerWave {
        GcmLds::PerWave s;  // the source subkey's set, and the wave's stage
        struct Keys {       // the destination's: the same set without a stage
            uint32_t rk[60];
            uint32_t rk16[60];
            G128 th[16];
            G128 t64[256];
        } d;
    } w[kRekeyWaves];
};
static_assert(sizeof(RekeyLds) == 65536 + kRekeyWaves * 11712 && sizeof(RekeyLds) <= 160 * 1024,
              "eight waves' key sets beside the T-table fill the CU's LDS");

template <class KS>
__device__ __forceinline__ void load_keys(KS &W, const BlobKey &K, uint32_t lane)
{
    for (uint32_t i = lane; i < 60; i += 64) W.rk[i] = K.rk[i];
    for (uint32_t i = lane; i < 60; i += 64) W.rk16[i] = ror32(K.rk[i], 16);
    if (lane < 16) W.th[lane] = K.th[lane];
    for (uint32_t i = lane; i < 256; i += 64) W.t64[i] = K.t64[i];
}

// The lanes' Horner sums closed: each by its power of H, XORed over the wave
// (every lane returns the sum).
__device__ __forceinline__ G128 ghash_close(G128 Z, uint32_t cnt, uint32_t nb, uint32_t lane, const BlobKey &K)
{
    if (cnt) {
        const uint32_t e = nb - lane - 64 * (cnt - 1);  // 1..64
        Z = gmul_bits(Z, K.hpow[e - 1]);
    }
    for (int off = 32; off; off >>= 1) {
        Z.hi ^= __shfl_xor(Z.hi, off);
        Z.lo ^= __shfl_xor(Z.lo, off);
    }
    return Z;
}

__global__ __launch_bounds__(kRekeyWaves * 64) void k_rekey(const RBatch B)
{
    __shared__ RekeyLds L;
    for (uint32_t i = threadIdx.x; i < 256 * 64; i += blockDim.x)
        L.te[i] = (i & 32u) ? ror32(g_te0[i >> 6], 8) : g_te0[i >> 6];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, laneoff = (lane & 31u) << 2;
    const char *te = reinterpret_cast<const char *>(L.te);
    __syncthreads();
    RekeyLds::PerWave &W = L.w[wv];
    // With few records, only as many waves per workgroup as share them out
    // evenly over the grid stay: the others would draw tickets beside them
    // and crowd one CU's LDS pipe while other CUs idle.  (No barrier follows.)
#ifndef REKEY_DIAG_PACKED_GRID  // build-time diagnostic only: the packed grid of DESIGN.md 5.14's A/B
    if (wv >= (B.nrecs + gridDim.x - 1) / gridDim.x) return;
#endif
    // Persistent, as k_gcm and k_rec_open: each wave takes records from a
    // counter until none is left.
    for (;;) {
    uint32_t pc = atomicAdd(&B.flags[kFlagTicket], lane == 0 ? 1u : 0u);  // every lane (see k_gcm)
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
    if (B.status[b]) continue;  // the subkey did not open, or another record of the blob did not
    const RBlob D = B.blobs[b];
    const BlobKey &Ks = B.bk[2 * b], &Kd = B.bk[2 * b + 1];
    // this wave's tables (the previous record's reads of them are done: the
    // wave barrier at the end of its loop body)
    load_keys(W.s, Ks, lane);
    load_keys(W.d, Kd, lane);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    const uint32_t k = pc - D.rec0;
    const uint64_t r0 = kHdr + uint64_t(k) * kRecMax;                       // the record in the blob, in and out
    const uint32_t m = uint32_t(min<uint64_t>(kRecMax, D.len - r0)) - 28u;  // ciphertext bytes (>= 0: the host checked)
    const uint32_t nb = (m + 15) / 16;
    const uint8_t *rec = B.in + D.src + r0;
    const gu8 *ct = reinterpret_cast<const gu8 *>(reinterpret_cast<uintptr_t>(rec + 12));
    const uint32_t ct_sh = uint32_t(reinterpret_cast<uintptr_t>(ct) & 3u);
    uint8_t *o = B.out + B.out_off[b] + r0;
    uint32_t js[3], jd[3];
    nonce_words(rec, js);  // the source's nonce is the one the record carries
    nonce_words(B.rnd + 56ull * b + 44, jd);
    jd[2] ^= k;  // Encode's rule: the data nonce with its last four bytes XOR k
    if (lane < 12) o[lane] = uint8_t(jd[lane >> 2] >> (24 - 8 * (lane & 3)));
    uint8_t *oct = o + 12;
    const CtrPre pre_s = ctr_pre(W.s, te, laneoff, js), pre_d = ctr_pre(W.d, te, laneoff, jd);
    const G128 *t64s = W.s.t64, *t64d = W.d.t64;
    uint8_t *stage = reinterpret_cast<uint8_t *>(W.s.stage);
    // The ciphertext as dwords from its aligned-down start: the dwords that
    // hold its first and last byte lie inside the record (the nonce before,
    // the tag after), and the buffer returns 0 past them.
    const uint32_t lastq = m ? (ct_sh + m - 1) >> 2 : 0u;
    const __amdgpu_buffer_rsrc_t prs = gcm_rsrc(reinterpret_cast<uintptr_t>(ct) - ct_sh, uint64_t(lastq + 1) * 4);
    const bool ct_fast = ct_sh == 0 && (m & 15u) == 0;  // whole aligned blocks: one 16-byte load each
    G128 Zs = {0, 0}, Zd = {0, 0};
    uint32_t cnt = 0;
    const uint32_t rows = (nb + 63) / 64;
    for (uint32_t j = 0; j < rows; j += kGcmRows) {
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
        // both keystreams of the step's blocks; they meet the ciphertext in
        // registers only
        uint32_t ks[kGcmRows][4], kd[kGcmRows][4];
        {
            uint32_t ctr[kGcmRows];
#pragma unroll
            for (uint32_t u = 0; u < kGcmRows; ++u) ctr[u] = 2 + 64 * (j + u) + lane;
            aes256_ctr_lds<kGcmRows>(W.s, te, laneoff, pre_s, ctr, ks);
            aes256_ctr_lds<kGcmRows>(W.d, te, laneoff, pre_d, ctr, kd);
        }
#pragma unroll
        for (int u = 0; u < int(kGcmRows); ++u) {
            const uint32_t i = 64 * (j + u) + lane;
            uint4 cw = make_uint4(0, 0, 0, 0);
            if (i < nb) {
                const uint32_t bytes = min(16u, m - 16 * i);
                uint32_t w[4], x[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = be32(__builtin_amdgcn_alignbit(px[u][q + 1], px[u][q], 8 * ct_sh));
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = w[q] ^ ks[u][q] ^ kd[u][q];
                if (bytes < 16) {  // what follows the ciphertext (the tag) is neither hashed nor re-keyed
                    for (int q = 0; q < 4; ++q) {
                        const int keep = int(bytes) - 4 * q;
                        const uint32_t mask = keep >= 4 ? 0xFFFFFFFFu : keep <= 0 ? 0u : ~(0xFFFFFFFFu >> (8 * keep));
                        w[q] &= mask;
                        x[q] &= mask;
                    }
                }
                Zs = gx(gmul8(Zs, t64s), G128{uint64_t(w[0]) << 32 | w[1], uint64_t(w[2]) << 32 | w[3]});
                Zd = gx(gmul8(Zd, t64d), G128{uint64_t(x[0]) << 32 | x[1], uint64_t(x[2]) << 32 | x[3]});
                ++cnt;
                cw = make_uint4(be32(x[0]), be32(x[1]), be32(x[2]), be32(x[3]));
            }
            W.s.stage[64 * u + lane] = cw;
        }
        __builtin_amdgcn_wave_barrier();
        // the rows' new ciphertext through LDS, as k_gcm stores its own:
        // exactly row_bytes bytes
        {
            const uint32_t row_bytes = min(1024u * kGcmRows, m - 1024 * j);
            uint8_t *dst = oct + 1024 * j;
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
    Zs = ghash_close(Zs, cnt, nb, lane, Ks);
    Zd = ghash_close(Zd, cnt, nb, lane, Kd);
    if (lane == 0) {
        const G128 lenblk = {0, uint64_t(m) * 8};
        const G128 Ss = gmul4(gx(Zs, lenblk), W.s.th), Sd = gmul4(gx(Zd, lenblk), W.d.th);
        uint32_t ts[1][4] = {{js[0], js[1], js[2], 1}}, td[1][4] = {{jd[0], jd[1], jd[2], 1}};
        aes256_blocks_lds<1>(W.s, te, laneoff, ts);
        aes256_blocks_lds<1>(W.d, te, laneoff, td);
        uint32_t tw[4];
        gcm_block_words(rec + 12 + m, tw);
        const G128 want = g_from_words(tw), got = gx(Ss, g_from_words(ts[0]));
        if ((want.hi ^ got.hi) | (want.lo ^ got.lo)) {  // all 16 bytes, no early exit
            B.status[b] = CDC_E_AUTH;
            B.flags[kFlagFailed] = 1;
        }
        const G128 tag = gx(Sd, g_from_words(td[0]));
        uint8_t *tp = oct + m;
        for (int q = 0; q < 8; ++q) {
            tp[q] = uint8_t(tag.hi >> (56 - 8 * q));
            tp[8 + q] = uint8_t(tag.lo >> (56 - 8 * q));
        }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    }
}

// A tag failed (kFlagFailed): the blob's planned range holds nothing a reader
// may use, and the blobs after it move down over it, in order (a later blob's
// new place may overlap an earlier one's old place), as k_dec_compact moves
// Decode's.  Rare, so one workgroup does it all.
__global__ __launch_bounds__(256) void k_tc_compact(const RBatch B)
{
    if (!B.flags[kFlagFailed]) return;
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

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static cdc::AesTables g_tab;

// Kept per device between calls (grow-only); a call holds its device's lock
// while it runs (the entry point is synchronous).
struct WsCache {
    std::mutex mu;
    cdc::DevBuf ws;     // the re-key path's plan and key states
    cdc::PinBuf stage;  // pinned staging of that plan
    cdc::DevBuf plain;  // the decoded blobs of the check and of the re-encode path
};
static WsCache *const g_ws = new WsCache[cdc::kMaxDevices];  // never destroyed (DevBuf)

// The re-key of m blobs (both keys, same compression).  CDC_E_NOSPACE with
// oo[m] the capacity needed, before anything is launched.
static int rekey_batch(WsCache &C, int device, const uint8_t *d_in, const uint64_t *offsets, const uint64_t *lens,
                       uint32_t m, const uint8_t *src_key, const uint8_t *dst_key, const uint8_t *random, uint8_t *d_out,
                       uint64_t out_cap, uint64_t *oo, int32_t *status, hipStream_t s)
{
    tplan::BatchPlan P;
    int st = tplan::plan_batch(lens, m, true, true, P);
    if (st != CDC_OK) return st;
    if (P.total > out_cap) {
        oo[m] = P.total;
        return CDC_E_NOSPACE;
    }
    st = cdc::upload_aes_tables(g_tab, g_te0, g_sbox);
    if (st != CDC_OK) return st;
    const size_t nb = m;
    cdc::Carver cv(16);
    // the staged prefix, then what only the device touches
    const size_t o_blobs = cv.take(nb * sizeof(RBlob)), o_status = cv.take(nb * 4), o_oo = cv.take((nb + 1) * 8),
                 o_rnd = cv.take(nb * 56), o_keys = cv.take(64), h_prefix = cv.bytes();
    const size_t o_bk = cv.take(2 * nb * sizeof(BlobKey)), o_flags = cv.take(16);
    if (!C.ws.reserve(cv.bytes()) || !C.stage.reserve(h_prefix)) return CDC_E_NOMEM;
    uint8_t *const ws = C.ws.as<uint8_t>(), *const hp = C.stage.as<uint8_t>();
    {
        RBlob *blobs = reinterpret_cast<RBlob *>(hp + o_blobs);
        int32_t *hst = reinterpret_cast<int32_t *>(hp + o_status);
        for (uint32_t b = 0; b < m; ++b) {
            blobs[b] = RBlob{offsets[b], lens[b], uint32_t(P.rec0[b]), uint32_t(P.blobs[b].nrec)};
            hst[b] = P.blobs[b].status;
        }
        std::memcpy(hp + o_oo, P.out_off.data(), (nb + 1) * 8);
        std::memcpy(hp + o_rnd, random, nb * 56);
        std::memcpy(hp + o_keys, src_key, 32);
        std::memcpy(hp + o_keys + 32, dst_key, 32);
    }
    RBatch B{};
    B.in = d_in;
    B.out = d_out;
    B.n = m;
    B.nrecs = uint32_t(P.nrecs);
    B.blobs = reinterpret_cast<const RBlob *>(ws + o_blobs);
    B.keys = ws + o_keys;
    B.rnd = ws + o_rnd;
    B.bk = reinterpret_cast<BlobKey *>(ws + o_bk);
    B.status = reinterpret_cast<int32_t *>(ws + o_status);
    B.out_off = reinterpret_cast<uint64_t *>(ws + o_oo);
    B.flags = reinterpret_cast<uint32_t *>(ws + o_flags);
    bool ok = hipMemcpyAsync(ws, hp, h_prefix, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemsetAsync(ws + o_flags, 0, 16, s) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_tc_keys, dim3((m + kKeyThreads - 1) / kKeyThreads), dim3(kKeyThreads), 0, s, B);
        hipLaunchKernelGGL(k_tc_pows, dim3((2 * m + kPowWaves - 1) / kPowWaves), dim3(kPowWaves * 64), 0, s, B);
        if (P.nrecs) {
            // A persistent grid: one workgroup per CU (its LDS holds one).  With
            // fewer records than the device has waves, a workgroup per record
            // all the same, and k_rekey keeps only the waves that share the
            // records out evenly: eight waves of one workgroup would crowd one
            // CU's LDS pipe while other CUs idle.
#ifdef REKEY_DIAG_PACKED_GRID
            const uint64_t wgs = (P.nrecs + kRekeyWaves - 1) / kRekeyWaves;
#else
            const uint64_t wgs = P.nrecs;
#endif
            hipLaunchKernelGGL(k_rekey, dim3(uint32_t(std::min<uint64_t>(wgs, uint64_t(cdc::device_cus(device))))),
                               dim3(kRekeyWaves * 64), 0, s, B);
        }
        hipLaunchKernelGGL(k_tc_compact, dim3(1), dim3(256), 0, s, B);
        ok = hipGetLastError() == hipSuccess;
    }
    // Neither repository key outlives the call in the cached workspace or its
    // pinned staging (k_tc_keys, their only reader, is done by now on this
    // stream).  The blobs' own subkey states stay until the next call
    // overwrites them, as Decode's and Encode's do: each opens one blob.
    ok = ok && hipMemsetAsync(ws + o_keys, 0, 64, s) == hipSuccess &&
         hipMemcpyAsync(oo, ws + o_oo, (nb + 1) * 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipMemcpyAsync(status, ws + o_status, nb * 4, hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    std::memset(hp + o_keys, 0, 64);
    return ok ? CDC_OK : CDC_E_DEVICE;
}

}  // namespace tc

extern "C" int64_t cdc_transcode_size(uint64_t len, int src_encrypted, int dst_encrypted)
{
    const tplan::BlobPlan P = tplan::plan_blob(len, src_encrypted != 0, dst_encrypted != 0);
    return P.status != CDC_OK ? int64_t(P.status) : int64_t(P.out_len);
}

extern "C" int cdc_transcode_device(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                                    uint32_t n, const cdc_codec *src, const cdc_codec *dst, const uint8_t *checksums,
                                    const uint8_t *random, uint8_t *d_out, uint64_t out_cap, uint64_t *out_offsets,
                                    int32_t *status, void *stream)
{
    return cdc_transcode_device_level(device, d_in, offsets, lens, n, src, dst, checksums, random, d_out, out_cap,
                                      out_offsets, status, CDC_LEVEL_FAST, stream);
}

extern "C" int cdc_transcode_device_level(int device, const void *d_in, const uint64_t *offsets, const uint64_t *lens,
                                          uint32_t n, const cdc_codec *src, const cdc_codec *dst,
                                          const uint8_t *checksums, const uint8_t *random, uint8_t *d_out,
                                          uint64_t out_cap, uint64_t *out_offsets, int32_t *status, int level,
                                          void *stream)
{
    if (!cdc::level_ok(level)) return CDC_E_INVALID;
    if (device < 0 || device >= cdc::kMaxDevices || !src || !dst || !out_offsets ||
        (n && (!d_in || !offsets || !lens || !status)) || (!d_out && out_cap) || (dst->key && !random))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    if (n == 0) {
        out_offsets[0] = 0;
        return CDC_OK;
    }
    const tplan::Path path = tplan::choose_path(src->compress, src->key != nullptr, dst->compress, dst->key != nullptr);
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    tc::WsCache &C = tc::g_ws[device];
    std::lock_guard<std::mutex> lk(C.mu);
    if (!C.plain.reserve(16)) return CDC_E_NOMEM;
    const uint8_t *const in = static_cast<const uint8_t *>(d_in);
    std::fill(status, status + n, int32_t(CDC_OK));

    // 1. The check, and the re-encode path's Decode: the blobs decoded into the
    // library's workspace (sized by the call's own report), and with checksums
    // hashed and compared there (cdc_check_device's steps).
    std::vector<uint64_t> poff;  // n + 1: the decoded blobs in C.plain
    if (checksums || path == tplan::kPathReencode) {
        poff.resize(size_t(n) + 1);
        for (int attempt = 0;; ++attempt) {
            const int st = cdc::decode_checked(device, d_in, offsets, lens, n, src->compress, src->key, checksums,
                                               C.plain.as<uint8_t>(), C.plain.cap(), poff.data(), status, stream,
                                               nullptr, nullptr);
            if (st == CDC_E_NOSPACE && attempt == 0 && poff[n] > C.plain.cap()) {
                if (!C.plain.reserve(poff[n])) return CDC_E_NOMEM;
                continue;
            }
            if (st != CDC_OK) return st == CDC_E_NOSPACE ? CDC_E_DEVICE : st;  // the sizes changed between two passes
            break;
        }
    }
    // 2. What follows runs over the blobs that are still CDC_OK (all of them
    // without a check), so a failed blob is never encoded as an empty one.
    std::vector<uint32_t> live;
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] == CDC_OK) live.push_back(i);
    const uint32_t m = uint32_t(live.size());
    const bool all = m == n;
    std::vector<uint64_t> soff, slen, soo(size_t(m) + 1, 0);
    std::vector<int32_t> sst(m, CDC_OK);
    std::vector<uint8_t> srnd;
    const bool from_plain = path == tplan::kPathReencode;
    if (!all || from_plain) {
        soff.resize(m);
        slen.resize(m);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = live[j];
            soff[j] = from_plain ? poff[i] : offsets[i];
            slen[j] = from_plain ? poff[i + 1] - poff[i] : lens[i];
        }
    }
    const uint64_t *const p_off = (!all || from_plain) ? soff.data() : offsets;
    const uint64_t *const p_len = (!all || from_plain) ? slen.data() : lens;
    const uint8_t *p_rnd = random;
    if (dst->key && !all) {
        srnd.resize(size_t(m) * 56);
        for (uint32_t j = 0; j < m; ++j) std::memcpy(&srnd[size_t(j) * 56], random + size_t(live[j]) * 56, 56);
        p_rnd = srnd.data();
    }
    uint8_t *const out = d_out ? d_out : C.plain.as<uint8_t>();  // Encode wants a pointer even for out_cap = 0
    int st = CDC_OK;
    if (m) {
        switch (path) {
        case tplan::kPathCopy:
        case tplan::kPathOpen:
            st = cdc_decode_device(device, d_in, p_off, p_len, m, CDC_COMPRESS_NONE, src->key, d_out, out_cap, soo.data(),
                                   sst.data(), stream);
            break;
        case tplan::kPathSeal:
            st = cdc_encode_device(device, d_in, p_off, p_len, m, CDC_COMPRESS_NONE, dst->key, p_rnd, out, out_cap,
                                   soo.data(), stream);
            break;
        case tplan::kPathRekey:
            st = tc::rekey_batch(C, device, in, p_off, p_len, m, src->key, dst->key, p_rnd, d_out, out_cap, soo.data(),
                                 sst.data(), s);
            break;
        case tplan::kPathReencode:
            st = cdc_encode_device_level(device, C.plain.data(), p_off, p_len, m, dst->compress, dst->key, p_rnd, out,
                                         out_cap, soo.data(), level, stream);
            break;
        }
    }
    if (st == CDC_E_NOSPACE) {
        out_offsets[n] = soo[m];
        return st;
    }
    if (st != CDC_OK) return st;
    tplan::spread_results(live.data(), m, soo.data(), sst.data(), n, out_offsets, status);
    return CDC_OK;
}
