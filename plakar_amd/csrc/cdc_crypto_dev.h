// Device helpers that Encode (cdc_encode.hip) and Decode (cdc_decode.hip) share:
// AES-256 (key schedule, T-table rounds, the bank-conflict-free LDS form and
// its counter-mode caching), GF(2^128) multiplies for GHASH, the XXH32
// finish and the wide copy.  Functions only: the library is not built with
// relocatable device code, so each .hip file defines and uploads its own
// __device__ tables and hands them in.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace devc {

__device__ __forceinline__ uint32_t ror32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ uint32_t rol32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// AES-256 key schedule (FIPS-197 §5.2), words big-endian.
__device__ void aes256_expand(const uint8_t key[32], uint32_t rk[60], const uint8_t *sbox)
{
    for (int i = 0; i < 8; ++i)
        rk[i] = uint32_t(key[4 * i]) << 24 | uint32_t(key[4 * i + 1]) << 16 | uint32_t(key[4 * i + 2]) << 8 |
                key[4 * i + 3];
    uint32_t rcon = 1;
    for (int i = 8; i < 60; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 8 == 0) {
            t = rol32(t, 8);
            t = uint32_t(sbox[t >> 24]) << 24 | uint32_t(sbox[(t >> 16) & 255]) << 16 |
                uint32_t(sbox[(t >> 8) & 255]) << 8 | sbox[t & 255];
            t ^= rcon << 24;
            rcon = (rcon << 1) ^ ((rcon & 0x80) ? 0x1B : 0);
        } else if (i % 8 == 4) {
            t = uint32_t(sbox[t >> 24]) << 24 | uint32_t(sbox[(t >> 16) & 255]) << 16 |
                uint32_t(sbox[(t >> 8) & 255]) << 8 | sbox[t & 255];
        }
        rk[i] = rk[i - 8] ^ t;
    }
}

// One block, words big-endian (T-table form; Te1..3 are rotations of Te0).
__device__ __forceinline__ void aes256_block(const uint32_t *rk, const uint32_t *te, const uint8_t *sb, uint32_t s[4])
{
    uint32_t s0 = s[0] ^ rk[0], s1 = s[1] ^ rk[1], s2 = s[2] ^ rk[2], s3 = s[3] ^ rk[3];
#pragma unroll
    for (int r = 1; r < 14; ++r) {
        const uint32_t t0 = te[s0 >> 24] ^ ror32(te[(s1 >> 16) & 255], 8) ^ ror32(te[(s2 >> 8) & 255], 16) ^
                            ror32(te[s3 & 255], 24) ^ rk[4 * r];
        const uint32_t t1 = te[s1 >> 24] ^ ror32(te[(s2 >> 16) & 255], 8) ^ ror32(te[(s3 >> 8) & 255], 16) ^
                            ror32(te[s0 & 255], 24) ^ rk[4 * r + 1];
        const uint32_t t2 = te[s2 >> 24] ^ ror32(te[(s3 >> 16) & 255], 8) ^ ror32(te[(s0 >> 8) & 255], 16) ^
                            ror32(te[s1 & 255], 24) ^ rk[4 * r + 2];
        const uint32_t t3 = te[s3 >> 24] ^ ror32(te[(s0 >> 16) & 255], 8) ^ ror32(te[(s1 >> 8) & 255], 16) ^
                            ror32(te[s2 & 255], 24) ^ rk[4 * r + 3];
        s0 = t0;
        s1 = t1;
        s2 = t2;
        s3 = t3;
    }
    s[0] = (uint32_t(sb[s0 >> 24]) << 24 | uint32_t(sb[(s1 >> 16) & 255]) << 16 | uint32_t(sb[(s2 >> 8) & 255]) << 8 |
            sb[s3 & 255]) ^ rk[56];
    s[1] = (uint32_t(sb[s1 >> 24]) << 24 | uint32_t(sb[(s2 >> 16) & 255]) << 16 | uint32_t(sb[(s3 >> 8) & 255]) << 8 |
            sb[s0 & 255]) ^ rk[57];
    s[2] = (uint32_t(sb[s2 >> 24]) << 24 | uint32_t(sb[(s3 >> 16) & 255]) << 16 | uint32_t(sb[(s0 >> 8) & 255]) << 8 |
            sb[s1 & 255]) ^ rk[58];
    s[3] = (uint32_t(sb[s3 >> 24]) << 24 | uint32_t(sb[(s0 >> 16) & 255]) << 16 | uint32_t(sb[(s1 >> 8) & 255]) << 8 |
            sb[s2 & 255]) ^ rk[59];
}

// ---------------------------------------------------------------------------
// GF(2^128) in GCM's bit order (SP 800-38D §6.3): an element is (hi, lo) =
// the big-endian halves of its 16 bytes.  4-bit tables: T[i] = i * V for the
// 4-bit value i read MSB-first (T[8] = V, T[4] = V x, ...).
// ---------------------------------------------------------------------------
struct G128 {
    uint64_t hi, lo;
};

__device__ __forceinline__ G128 gx(G128 a, G128 b) { return {a.hi ^ b.hi, a.lo ^ b.lo}; }

__device__ void gtable(G128 v, G128 t[16])
{
    auto half = [](G128 x) {  // x * x^1 (one right shift with reduction)
        const uint64_t r = (x.lo & 1) ? 0xE100000000000000ull : 0;
        return G128{(x.hi >> 1) ^ r, (x.lo >> 1) | (x.hi << 63)};
    };
    t[0] = {0, 0};
    t[8] = v;
    t[4] = half(t[8]);
    t[2] = half(t[4]);
    t[1] = half(t[2]);
    for (int i = 3; i < 16; ++i)
        if (i & (i - 1)) t[i] = gx(t[i & -i], t[i & (i - 1)]);
}

// rem_4bit[r]: the reduction of the 4 bits shifted out, in the top 16 bits.
__device__ __forceinline__ uint64_t rem4(uint32_t r)
{
    uint64_t x = 0;
    if (r & 1) x ^= 0x1C20;
    if (r & 2) x ^= 0x3840;
    if (r & 4) x ^= 0x7080;
    if (r & 8) x ^= 0xE100;
    return x << 48;
}

// x * V with V's 4-bit table (processed nibble by nibble from the last byte).
template <typename TAB>
__device__ __forceinline__ G128 gmul4(G128 x, const TAB &t)
{
    G128 z = {0, 0};
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        const uint64_t w = i >= 16 ? x.lo : x.hi;
        const uint32_t nib = uint32_t(w >> (4 * ((31 - i) & 15))) & 15;
        if (i != 31) {
            const uint32_t rem = uint32_t(z.lo) & 15;
            z.lo = (z.hi << 60) | (z.lo >> 4);
            z.hi = (z.hi >> 4) ^ rem4(rem);
        }
        const G128 e = t[nib];
        z.hi ^= e.hi;
        z.lo ^= e.lo;
    }
    return z;
}

// a * b bit by bit (SP 800-38D Algorithm 1), for a per-lane multiplier.
__device__ G128 gmul_bits(G128 a, G128 b)
{
    // branch-free: the bit of a as a sign mask (v_ashrrev), z ^= v & mask and
    // the reduction's 0xE1 as one v_bitop3 each, v shifted by v_alignbit
    uint32_t z[4] = {0, 0, 0, 0};
    uint32_t v[4] = {uint32_t(b.hi >> 32), uint32_t(b.hi), uint32_t(b.lo >> 32), uint32_t(b.lo)};
    const uint32_t aw[4] = {uint32_t(a.hi >> 32), uint32_t(a.hi), uint32_t(a.lo >> 32), uint32_t(a.lo)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t w = aw[k];
#pragma unroll 8
        for (int i = 0; i < 32; ++i) {
            const uint32_t m = uint32_t(int32_t(w) >> 31);
#pragma unroll
            for (int q = 0; q < 4; ++q) z[q] = __builtin_amdgcn_bitop3_b32(z[q], v[q], m, 0x78);  // z ^ (v & m)
            w <<= 1;
            const uint32_t r = uint32_t(int32_t(v[3] << 31) >> 31);  // v's last bit as a mask
            v[3] = __builtin_amdgcn_alignbit(v[2], v[3], 1);
            v[2] = __builtin_amdgcn_alignbit(v[1], v[2], 1);
            v[1] = __builtin_amdgcn_alignbit(v[0], v[1], 1);
            v[0] = __builtin_amdgcn_bitop3_b32(v[0] >> 1, r, 0xE1000000u, 0x78);  // (v0 >> 1) ^ (r & 0xE1..)
        }
    }
    return {uint64_t(z[0]) << 32 | z[1], uint64_t(z[2]) << 32 | z[3]};
}

__device__ __forceinline__ G128 g_from_words(const uint32_t w[4])
{
    return {uint64_t(w[0]) << 32 | w[1], uint64_t(w[2]) << 32 | w[3]};
}

// Per-blob GCM state (workspace): AES round keys of the subkey, the 4-bit
// tables of H and H^64, and H^1..H^64.
struct BlobKey {
    uint32_t rk[60];
    uint32_t pad[4];
    G128 th[16];      // 4-bit table of H (the length block)
    G128 hpow[64];    // H^1 .. H^64
    G128 t64[256];    // 8-bit table of H^64 (the lanes' Horner steps)
};

// Global-memory views (global_load, counted in vmcnt only; a generic pointer
// gives flat loads, which also count in lgkmcnt).
typedef __attribute__((address_space(1))) const uint32_t gu32;
typedef __attribute__((address_space(1))) const uint8_t gu8;

__device__ __forceinline__ uint32_t ld32u(const uint8_t *p)  // unaligned
{
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;

// The merge of the four accumulators, the tail and the avalanche.
__device__ uint32_t xxh_finish(uint32_t v1, uint32_t v2, uint32_t v3, uint32_t v4, const uint8_t *p, uint64_t n)
{
    uint32_t h = n >= 16 ? rol32(v1, 1) + rol32(v2, 7) + rol32(v3, 12) + rol32(v4, 18) : P5;
    h += uint32_t(n);
    uint64_t i = n / 16 * 16;
    for (; i + 4 <= n; i += 4) h = rol32(h + ld32u(p + i) * P3, 17) * P4;
    for (; i < n; ++i) h = rol32(h + p[i] * P5, 11) * P1;
    h ^= h >> 15;
    h *= P2;
    h ^= h >> 13;
    h *= P3;
    h ^= h >> 16;
    return h;
}

// dst[0, n) = src[0, n) by the threads [tid, nt): aligned dword stores, each
// from two aligned source dwords (v_alignbit); the source's last aligned dword
// is read whole, never past it.
__device__ void copy_span(uint8_t *dst, const uint8_t *src, uint64_t n, uint32_t tid, uint32_t nt)
{
    const uint32_t head = uint32_t(min<uint64_t>(n, (4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    if (tid < head) dst[tid] = src[tid];
    dst += head;
    src += head;
    n -= head;
    const uint64_t nw = n / 4;
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst);
    const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(src) & 3u) * 8u;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(src) & ~uintptr_t(3));
    if (sh) {
        for (uint64_t i = tid; i < nw; i += nt) dw[i] = __builtin_amdgcn_alignbit(sw[i + 1], sw[i], sh);
    } else {
        for (uint64_t i = tid; i < nw; i += nt) dw[i] = sw[i];
    }
    for (uint64_t i = 4 * nw + tid; i < n; i += nt) dst[i] = src[i];
}

__device__ __forceinline__ void gcm_block_words(const uint8_t *p, uint32_t w[4])
{
    for (int i = 0; i < 4; ++i)
        w[i] = uint32_t(p[4 * i]) << 24 | uint32_t(p[4 * i + 1]) << 16 | uint32_t(p[4 * i + 2]) << 8 | p[4 * i + 3];
}

__device__ __forceinline__ G128 ghalf(G128 x)  // x times the field's x (one right shift with reduction)
{
    const uint64_t r = (x.lo & 1) ? 0xE100000000000000ull : 0;
    return G128{(x.hi >> 1) ^ r, (x.lo >> 1) | (x.hi << 63)};
}

// Raw buffer resource over [base, base + bytes): reads past the end return 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gcm_rsrc(uint64_t base, uint64_t bytes)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(base));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(base >> 32));
    const uint32_t n = __builtin_amdgcn_readfirstlane(uint32_t(bytes));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>((uint64_t(hi) << 32) | lo), 0, int(n), 0x00020000);
}

// One row per step with 16 waves (12 VGPRs spilled) and one row with 12 waves
// were 1 % and 19 % slower (profiles/r04_gcm_ab.txt, call 5).
constexpr uint32_t kGcmWaves = 12;  // one workgroup per CU (LDS: the 64-KiB table), three waves per SIMD
constexpr uint32_t kGcmRows = 2;    // rows of 64 blocks per step (their AES interleaved)

// LDS of a GCM workgroup.  Two T-tables, A = Te0 and B = Te0 rotated right by
// 8 bits, 32 copies each, in one 256-byte row per entry: A's copy c at byte
// 256 e + 4 c, B's at 256 e + 128 + 4 c.  A ds_read_b32 serves its lanes in
// two groups of 32 with banks (a/4) mod 32, so lane l reading copy l & 31 is
// conflict-free whatever the state bytes, and the address is ONE v_perm of
// the state word and the lane's offset (B: the instruction's offset 128).
// With B, a column is A[a] ^ B[b] ^ ror16(A[c] ^ B[d] ^ ror16(rk)): one
// rotate instead of three (rk16 holds the round keys rotated by 16).
struct GcmLds {
    uint32_t te[256 * 64];
    struct PerWave {
        uint32_t rk[60];
        uint32_t rk16[60];
        G128 th[16];
        G128 t64[256];
        uint4 stage[64 * kGcmRows];
    } w[kGcmWaves];
};

// Address of state byte k of word w in the 64-copy table.
__device__ __forceinline__ uint32_t te_addr(uint32_t laneoff, uint32_t w, uint32_t k)
{
    return __builtin_amdgcn_perm(laneoff, w, 0x0C0C0004u | (k << 8));
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// (PW: anything with GcmLds::PerWave's rk and rk16; cdc_transcode.hip keeps a
// second key set per wave that has no stage of its own.)
template <int N, class PW>
__device__ __forceinline__ void aes256_blocks_lds(const PW &pw, const char *te, uint32_t laneoff,
                                                  uint32_t (&st)[N][4])
{
    const uint32_t *rk = pw.rk, *rk16 = pw.rk16;
    auto A = [&](uint32_t w, uint32_t k) { return *reinterpret_cast<const uint32_t *>(te + te_addr(laneoff, w, k)); };
    auto B = [&](uint32_t w, uint32_t k) {
        return *reinterpret_cast<const uint32_t *>(te + te_addr(laneoff, w, k) + 128);
    };
    uint32_t s[N][4];
#pragma unroll
    for (int n = 0; n < N; ++n)
        for (int q = 0; q < 4; ++q) s[n][q] = st[n][q] ^ rk[q];
#pragma unroll
    for (int r = 1; r < 14; ++r) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            uint32_t t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t u = xor3(A(s[n][(q + 2) & 3], 1), B(s[n][(q + 3) & 3], 0), rk16[4 * r + q]);
                t[q] = xor3(A(s[n][q], 3), B(s[n][(q + 1) & 3], 2), ror32(u, 16));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) s[n][q] = t[q];
        }
    }
    // last round: S-box bytes (byte 2 of A's entries) gathered by v_perm
    auto S4 = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        const uint32_t hi = __builtin_amdgcn_perm(A(a, 3), A(b, 2), 0x0602FFFFu);  // [Sa, Sb, -, -]
        const uint32_t lo = __builtin_amdgcn_perm(A(c, 1), A(d, 0), 0xFFFF0602u);  // [-, -, Sc, Sd]
        return (hi & 0xFFFF0000u) | (lo & 0xFFFFu);
    };
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            st[n][q] = S4(s[n][q], s[n][(q + 1) & 3], s[n][(q + 2) & 3], s[n][(q + 3) & 3]) ^ rk[56 + q];
}

// Counter mode within one piece: the counter block is (J0[0..2], ctr) with
// ctr < 2^16 (at most 4,097 blocks), so after the first AddRoundKey the
// words s0..s2 and bytes 2-3 of s3 are the piece's constants.  Round 1's
// outputs t2, t3 are then constants, and t0, t1 each depend on one counter
// byte; round 2 takes 8 of its 16 lookups from t2, t3.  Those are done once
// per piece (CtrPre, wave-uniform: SGPRs), leaving 2 + 8 lookups for rounds
// 1-2 instead of 32 (counter-mode caching).
struct CtrPre {
    uint32_t p0t, p0u, p1t, p1u;  // round 1: t0 = p0t ^ ror16(p0u ^ B(s3, 0)), t1 = p1t ^ ror16(p1u ^ A(s3, 1))
    uint32_t r0, w1, v1, w2, w3, v3;  // round 2's constant terms
};

template <class PW>
__device__ __forceinline__ CtrPre ctr_pre(const PW &pw, const char *te, uint32_t laneoff, const uint32_t (&j0)[3])
{
    const uint32_t *rk = pw.rk, *rk16 = pw.rk16;
    auto A = [&](uint32_t w, uint32_t k) { return *reinterpret_cast<const uint32_t *>(te + te_addr(laneoff, w, k)); };
    auto B = [&](uint32_t w, uint32_t k) {
        return *reinterpret_cast<const uint32_t *>(te + te_addr(laneoff, w, k) + 128);
    };
    auto u = [](uint32_t x) { return uint32_t(__builtin_amdgcn_readfirstlane(int(x))); };
    const uint32_t s0 = j0[0] ^ rk[0], s1 = j0[1] ^ rk[1], s2 = j0[2] ^ rk[2], s3 = rk[3];  // s3: bytes 2-3 only
    CtrPre c;
    c.p0t = u(A(s0, 3) ^ B(s1, 2));
    c.p0u = u(A(s2, 1) ^ rk16[4]);
    c.p1t = u(A(s1, 3) ^ B(s2, 2));
    c.p1u = u(B(s0, 0) ^ rk16[5]);
    const uint32_t t2 = xor3(A(s2, 3), B(s3, 2), ror32(xor3(A(s0, 1), B(s1, 0), rk16[6]), 16));
    const uint32_t t3 = xor3(A(s3, 3), B(s0, 2), ror32(xor3(A(s1, 1), B(s2, 0), rk16[7]), 16));
    c.r0 = u(ror32(xor3(A(t2, 1), B(t3, 0), rk16[8]), 16));
    c.w1 = u(B(t2, 2));
    c.v1 = u(A(t3, 1) ^ rk16[9]);
    c.w2 = u(A(t2, 3) ^ B(t3, 2));
    c.w3 = u(A(t3, 3));
    c.v3 = u(B(t2, 0) ^ rk16[11]);
    return c;
}

// AES-256 of N counter blocks (J0[0..2], ctr[n]) of the piece CtrPre was made for.
template <int N, class PW>
__device__ __forceinline__ void aes256_ctr_lds(const PW &pw, const char *te, uint32_t laneoff, const CtrPre &c,
                                               const uint32_t (&ctr)[N], uint32_t (&st)[N][4])
{
    const uint32_t *rk = pw.rk, *rk16 = pw.rk16;
    auto A = [&](uint32_t w, uint32_t k) { return *reinterpret_cast<const uint32_t *>(te + te_addr(laneoff, w, k)); };
    auto B = [&](uint32_t w, uint32_t k) {
        return *reinterpret_cast<const uint32_t *>(te + te_addr(laneoff, w, k) + 128);
    };
    uint32_t s[N][4];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const uint32_t s3 = ctr[n] ^ rk[3];
        const uint32_t t0 = c.p0t ^ ror32(c.p0u ^ B(s3, 0), 16);
        const uint32_t t1 = c.p1t ^ ror32(c.p1u ^ A(s3, 1), 16);
        s[n][0] = xor3(A(t0, 3), B(t1, 2), c.r0);
        s[n][1] = xor3(A(t1, 3), c.w1, ror32(c.v1 ^ B(t0, 0), 16));
        s[n][2] = c.w2 ^ ror32(xor3(A(t0, 1), B(t1, 0), rk16[10]), 16);
        s[n][3] = xor3(c.w3, B(t0, 2), ror32(A(t1, 1) ^ c.v3, 16));
    }
#pragma unroll
    for (int r = 3; r < 14; ++r) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            uint32_t t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t v = xor3(A(s[n][(q + 2) & 3], 1), B(s[n][(q + 3) & 3], 0), rk16[4 * r + q]);
                t[q] = xor3(A(s[n][q], 3), B(s[n][(q + 1) & 3], 2), ror32(v, 16));
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) s[n][q] = t[q];
        }
    }
    auto S4 = [&](uint32_t a, uint32_t b, uint32_t cc, uint32_t d) {
        const uint32_t hi = __builtin_amdgcn_perm(A(a, 3), A(b, 2), 0x0602FFFFu);
        const uint32_t lo = __builtin_amdgcn_perm(A(cc, 1), A(d, 0), 0xFFFF0602u);
        return (hi & 0xFFFF0000u) | (lo & 0xFFFFu);
    };
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            st[n][q] = S4(s[n][q], s[n][(q + 1) & 3], s[n][(q + 2) & 3], s[n][(q + 3) & 3]) ^ rk[56 + q];
}

// x * V with V's 8-bit table, reduced once.  x = sum over its bytes b_i
// (i = 0: the top byte of hi, GCM's x^0..x^7) of b_i x^(8 i), so x V =
// sum t[b_i] x^(8 i): each entry shifted right by 8 i bits into a 256-bit
// sum D[0..7] (dwords, D[0] the most significant), then the part past x^127
// folded back once, x^128 = 1 + x + x^2 + x^7.  The entries of one byte
// offset (i = g, g + 4, g + 8, g + 12) add at whole dwords, so only four
// partial sums are shifted; no reduction per byte (Horner's byte-by-byte
// shift and reduce took twice the VALU), and no step waits on another.
__device__ __forceinline__ G128 gmul8(G128 x, const G128 *t)
{
    const uint32_t xw[4] = {uint32_t(x.hi >> 32), uint32_t(x.hi), uint32_t(x.lo >> 32), uint32_t(x.lo)};
    uint32_t D[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        uint32_t a[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const G128 e = t[(xw[j] >> (24 - 8 * g)) & 255u];
            const uint32_t ew[4] = {uint32_t(e.hi >> 32), uint32_t(e.hi), uint32_t(e.lo >> 32), uint32_t(e.lo)};
#pragma unroll
            for (int k = 0; k < 4; ++k) a[j + k] ^= ew[k];
        }
        if (g == 0) {
#pragma unroll
            for (int k = 0; k < 7; ++k) D[k] = a[k];
            D[7] = 0;
        } else {
            const uint32_t s = 8u * g;
            D[0] ^= a[0] >> s;
#pragma unroll
            for (int k = 1; k < 7; ++k) D[k] ^= __builtin_amdgcn_alignbit(a[k - 1], a[k], s);
            D[7] ^= a[6] << (32u - s);
        }
    }
    // fold: V = D[4..7] (x^128..x^247, so V (1 + x + x^2 + x^7) stays below x^127)
    uint32_t F[4];
    F[0] = xor3(D[4], D[4] >> 1, D[4] >> 2) ^ (D[4] >> 7);
#pragma unroll
    for (int k = 1; k < 4; ++k)
        F[k] = xor3(D[4 + k], __builtin_amdgcn_alignbit(D[3 + k], D[4 + k], 1),
                    __builtin_amdgcn_alignbit(D[3 + k], D[4 + k], 2)) ^
               __builtin_amdgcn_alignbit(D[3 + k], D[4 + k], 7);
    return G128{uint64_t(D[0] ^ F[0]) << 32 | (D[1] ^ F[1]), uint64_t(D[2] ^ F[2]) << 32 | (D[3] ^ F[3])};
}

__device__ __forceinline__ uint32_t be32(uint32_t x) { return __builtin_bswap32(x); }

// One wave: K.hpow[0] = H in, H^1..H^64 and the 8-bit table of H^64 out.
struct PowLds {
    G128 pw[64];
    G128 tab[16];
};

__device__ __forceinline__ void hpow_ladder(BlobKey &K, PowLds &L, uint32_t lane)
{
    if (lane == 0) L.pw[0] = K.hpow[0];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t m = 1; m < 64; m <<= 1) {
        if (lane < 16) {  // 4-bit table of X = H^m: entry i = XOR of X * x^(3 - j) over the bits j of i
            G128 v = L.pw[m - 1], e = {0, 0};
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                if ((lane >> j) & 1) e = gx(e, v);
                v = ghalf(v);
            }
            L.tab[lane] = e;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
        if (lane >= m && lane < 2 * m) L.pw[lane] = gmul4(L.pw[lane - m], L.tab);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
    K.hpow[lane] = L.pw[lane];
    // 8-bit table of V = H^64: T[i] = XOR of v_j over the bits j of i, v_7 = V,
    // v_(j-1) = v_j * x (a halving)
    G128 v[8];
    v[7] = L.pw[63];
#pragma unroll
    for (int j = 7; j > 0; --j) v[j - 1] = ghalf(v[j]);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t i = 4 * lane + q;
        G128 e = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if ((i >> j) & 1) e = gx(e, v[j]);
        K.t64[i] = e;
    }
}

}  // namespace devc
