// The LZ4 block sequence walker and validator: every bound that Decode's block
// kernels rely on is decided here.  cdc_decode.hip walks a block with it (one
// wave, the bytes through a wave-wide window) and tests/c/lz4d_host_fuzz.cpp
// compiles the same text under plain g++ (address and undefined-behaviour
// sanitizers, exactly-sized heap buffers) against liblz4.
//
// A block is a chain of sequences: token (literal length nibble, match length
// nibble), literal length extension bytes (255 steps), the literals, then a
// 2-byte little-endian offset and the match length extension.  The block ends
// with a sequence that has literals only.  Rejected (the caller reports
// CDC_E_CORRUPT):
//   - a token, an extension, a literal run or an offset past the block's input;
//   - offset 0, or an offset that reaches before the block's first output byte
//     (blocks are independent: there is nothing before it);
//   - output past `omax` (the frame's block maximum while sizing, the bytes
//     planned for the block's blob while emitting);
//   - input that is not consumed exactly by a final literal-only sequence, or
//     (the format's end-of-block rule, which liblz4's decoder relies on) a
//     final sequence of fewer than 5 literals after a match.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZ4W_HD __host__ __device__ inline
#else
#define LZ4W_HD inline
#endif

namespace lz4w {

constexpr uint32_t kMaxBlockIn = 4u << 20;  // BD 7: no block is larger (lengths then stay far below 2^32)
constexpr uint32_t kLastLiterals = 5;

enum { kSeq = 0, kEnd = 1, kBad = -1 };

struct Seq {
    uint32_t lit_src;  // index of the first literal in the block's input
    uint32_t lit_len;
    uint32_t off;      // 0 on the final sequence
    uint32_t mlen;     // 0 on the final sequence
};

// A length nibble of 15 continues in bytes that add up, the last one below 255.
template <class Rd>
LZ4W_HD bool ext_len(Rd &rd, uint32_t n, uint32_t &ip, uint32_t &len)
{
    for (;;) {
        if (ip >= n) return false;
        const uint32_t b = rd(ip++);
        len += b;  // at most 255 n < 2^31
        if (b != 255u) return true;
    }
}

// The sequence at input index ip of a block of n bytes (rd(i): byte i, asked
// only for i < n) when opos bytes are decoded and at most omax may be.  On
// kSeq and kEnd, s holds a sequence whose literals lie inside the input and
// whose output [opos, opos + lit_len + mlen) lies inside [0, omax), its match
// source inside [0, opos + lit_len); ip is the next sequence's token.
template <class Rd>
LZ4W_HD int next_seq(Rd &rd, uint32_t n, uint32_t &ip, uint32_t opos, uint32_t omax, Seq &s)
{
    if (n > kMaxBlockIn || opos > omax) return kBad;
    if (ip >= n) return kBad;  // the input ended after a match (or the block is empty)
    const uint32_t tok = rd(ip++);
    uint32_t ll = tok >> 4;
    if (ll == 15u && !ext_len(rd, n, ip, ll)) return kBad;
    if (ll > n - ip || ll > omax - opos) return kBad;
    s.lit_src = ip;
    s.lit_len = ll;
    s.off = s.mlen = 0;
    ip += ll;
    if (ip == n) return (opos != 0 && ll < kLastLiterals) ? kBad : kEnd;
    if (n - ip < 2) return kBad;
    const uint32_t off = rd(ip) | rd(ip + 1) << 8;
    ip += 2;
    uint32_t ml = tok & 15u;
    if (ml == 15u && !ext_len(rd, n, ip, ml)) return kBad;
    ml += 4;
    const uint32_t pos = opos + ll;
    if (off == 0 || off > pos || ml > omax - pos) return kBad;
    s.off = off;
    s.mlen = ml;
    return kSeq;
}

// The stop mode (prefix Decode): next_seq for a caller that wants the block's
// output only up to `stop` (<= omax).  kStop is a fourth answer: s is the
// sequence cut to the byte, so that opos + lit_len + mlen == stop (either
// part may be empty), and the walk ends there.  What a cut sequence leaves out
// is not looked at: the literals past the cut need not lie inside the input,
// and when the literals end exactly at `stop` the match that follows is not
// read.  A sequence that ends at or before `stop` is judged as next_seq
// judges it, so a block that ends exactly at `stop` answers kEnd, not kStop,
// and has passed every test of the full walk.  Output past omax is kBad even
// where it would also pass `stop`.  With opos >= stop nothing is read.
enum { kStop = 2 };

template <class Rd>
LZ4W_HD int next_seq_stop(Rd &rd, uint32_t n, uint32_t &ip, uint32_t opos, uint32_t omax, uint32_t stop, Seq &s)
{
    if (n > kMaxBlockIn || opos > omax || stop > omax) return kBad;
    s.lit_src = ip;
    s.lit_len = s.off = s.mlen = 0;
    if (opos >= stop) return kStop;
    if (ip >= n) return kBad;
    const uint32_t tok = rd(ip++);
    uint32_t ll = tok >> 4;
    if (ll == 15u && !ext_len(rd, n, ip, ll)) return kBad;
    if (ll > omax - opos) return kBad;
    s.lit_src = ip;
    if (ll > stop - opos) {  // the cut falls inside the literals
        s.lit_len = stop - opos;
        if (s.lit_len > n - ip) return kBad;
        return kStop;
    }
    if (ll > n - ip) return kBad;
    s.lit_len = ll;
    ip += ll;
    if (ip == n) return (opos != 0 && ll < kLastLiterals) ? kBad : kEnd;
    const uint32_t pos = opos + ll;
    if (pos == stop) return kStop;  // a match is at least 4 bytes: none of it is wanted
    if (n - ip < 2) return kBad;
    const uint32_t off = rd(ip) | rd(ip + 1) << 8;
    ip += 2;
    uint32_t ml = tok & 15u;
    if (ml == 15u && !ext_len(rd, n, ip, ml)) return kBad;
    ml += 4;
    if (off == 0 || off > pos || ml > omax - pos) return kBad;
    s.off = off;
    if (ml > stop - pos) {  // the cut falls inside the match
        s.mlen = stop - pos;
        return kStop;
    }
    s.mlen = ml;
    return kSeq;
}

// Byte i of a match of mlen bytes at output position pos with this offset is
// a copy of the output byte at this index, which lies in [pos - off, pos):
// an overlapping match (off < mlen) repeats its last off bytes, so no byte of
// a match depends on another byte of the same match.
LZ4W_HD uint32_t match_src(uint32_t pos, uint32_t off, uint32_t mlen, uint32_t i)
{
    return pos - off + (off >= mlen ? i : i % off);
}

// One block, serially: the decoded size, or -1.  dst == nullptr sizes only.
// Writes dst[0, omax) at most.
template <class Rd>
LZ4W_HD int64_t decode_block(Rd &rd, uint32_t n, uint8_t *dst, uint32_t omax)
{
    uint32_t ip = 0, opos = 0;
    for (;;) {
        Seq s;
        const int r = next_seq(rd, n, ip, opos, omax, s);
        if (r < 0) return -1;
        if (dst)
            for (uint32_t i = 0; i < s.lit_len; ++i) dst[opos + i] = uint8_t(rd(s.lit_src + i));
        opos += s.lit_len;
        if (r == kEnd) return int64_t(opos);
        if (dst)
            for (uint32_t i = 0; i < s.mlen; ++i) dst[opos + i] = dst[match_src(opos, s.off, s.mlen, i)];
        opos += s.mlen;
    }
}

// One block in the stop mode, serially: the bytes written (<= stop), or -1.
// `stopped` says whether the walk ended at the cut (kStop) or at the block's
// end (kEnd).  Writes dst[0, stop) at most.
template <class Rd>
LZ4W_HD int64_t decode_block_stop(Rd &rd, uint32_t n, uint8_t *dst, uint32_t omax, uint32_t stop, bool &stopped)
{
    uint32_t ip = 0, opos = 0;
    stopped = false;
    for (;;) {
        Seq s;
        const int r = next_seq_stop(rd, n, ip, opos, omax, stop, s);
        if (r < 0) return -1;
        for (uint32_t i = 0; i < s.lit_len; ++i) dst[opos + i] = uint8_t(rd(s.lit_src + i));
        opos += s.lit_len;
        if (r == kEnd) return int64_t(opos);
        for (uint32_t i = 0; i < s.mlen; ++i) dst[opos + i] = dst[match_src(opos, s.off, s.mlen, i)];
        opos += s.mlen;
        if (r == kStop) {
            stopped = true;
            return int64_t(opos);
        }
    }
}

}  // namespace lz4w
