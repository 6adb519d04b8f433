// SHA-256 block arithmetic of one message of `total` bytes (FIPS 180-4, 5.1.1),
// for host and device: how many 64-byte blocks the padded message has, which
// bytes of block b are data, where 0x80 goes and the bit-length words.
// k_object_digest (cdc_digest.hip) pads with it; tests/c/check_plan_check.cpp
// runs it on the CPU for totals no GPU test can afford (the 64-bit bit
// length).  total < 2^61: the bit length is a 64-bit field.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SHAB_FN __host__ __device__ inline
#else
#define SHAB_FN inline
#endif

namespace shab {

constexpr uint64_t kMaxTotal = (1ull << 61) - 1;

// blocks of the padded message: the full ones, then 1 or 2
SHAB_FN uint64_t blocks(uint64_t total) { return total / 64u + ((total % 64u) <= 55u ? 1u : 2u); }

// Message bytes from block b on, clamped to [-128, 128]: 64 or more is a block
// of data only, 0..63 the block where the data ends (0x80 follows its last
// byte), negative a block past the data (-64 < r < 0: the second padding
// block, zeros and the length).
SHAB_FN int32_t remaining(uint64_t total, uint64_t b)
{
    const uint64_t done = 64u * b;
    if (done <= total) return total - done >= 128u ? 128 : int32_t(total - done);
    return done - total >= 128u ? -128 : -int32_t(done - total);
}

// Big-endian word q (0..15) of a block with r = remaining(): the bits that
// stay data, and the 0x80 byte.
SHAB_FN uint32_t keep_mask(int32_t r, int q)
{
    const int32_t rem = r - 4 * q;
    return rem >= 4 ? 0xFFFFFFFFu : rem <= 0 ? 0u : ~(0xFFFFFFFFu >> (8 * rem));
}
SHAB_FN uint32_t pad_byte(int32_t r, int q)
{
    const int32_t rem = r - 4 * q;
    return (rem >= 0 && rem < 4) ? (0x80000000u >> (8 * rem)) : 0u;
}
// The block carries padding at all / the bit length in words 14 and 15.
SHAB_FN bool has_padding(int32_t r) { return r < 64 && r > -64; }
SHAB_FN bool has_length(int32_t r) { return r <= 55 && r > -64; }
SHAB_FN uint32_t bits_hi(uint64_t total) { return uint32_t(total >> 29); }
SHAB_FN uint32_t bits_lo(uint64_t total) { return uint32_t(total << 3); }

}  // namespace shab
