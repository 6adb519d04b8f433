// The gzip member (RFC 1952) and DEFLATE (RFC 1951) walker and validator: every
// bound that Decode's GZIP kernels rely on is decided here.  cdc_decode.hip
// walks a stream with it (one wave, the bytes through a wave-wide window, the
// code tables in LDS and built by the wave's lanes together) and
// tests/c/inflate_host_fuzz.cpp compiles the same text under plain g++
// (address and undefined-behaviour sanitizers, exactly-sized heap buffers)
// against zlib.
//
// The walker is a template over
//   Rd    rd(i): byte i of the stream, asked only for i < n;
//   Sink  lit / match / stored / flush: where the output goes.  The walker
//         checks every call against `omax` and the output so far before it
//         makes it, so a sink needs no bounds of its own;
//   Par   lane, nl, sync(): how table building is shared.  Serial{} is one
//         lane; the device passes its 64 lanes and a wave barrier.  Everything
//         outside the `for (i = lane; ...; i += nl)` loops is computed alike
//         by every lane.
//
// One member is read: magic 1f 8b, CM 8, FLG, MTIME, XFL, OS, then FEXTRA,
// FNAME, FCOMMENT and FHCRC as FLG says, the DEFLATE body, CRC-32 and ISIZE.
// The last four bytes of the stream are taken as the claimed size first (the
// plan); the walk then proves it.  Rejected as corrupt (CDC_E_CORRUPT):
//   - a stream shorter than header + 8; a wrong magic; CM != 8; a reserved FLG
//     bit (5-7); an optional field that runs past the stream; an FHCRC that is
//     not the low 16 bits of the header's CRC-32;
//   - a claim of more than 1032 bytes per body byte (DEFLATE's ceiling);
//   - input that ends inside a block header, a code or a stored block;
//   - BTYPE 3; a stored block whose LEN is not ~NLEN;
//   - HLIT > 286 or HDIST > 30 symbols; a code-length, literal/length or
//     distance set that is over-subscribed; one that is incomplete, except a
//     distance set with no code at all or with a single code of one bit;
//     repeat code 16 with no previous length; a repeat run past HLIT + HDIST;
//     a literal/length set without the end-of-block code;
//   - a bit pattern that is no code of its set; literal/length symbols 286 and
//     287 and distance symbols 30 and 31 when met (the fixed code has them);
//   - a distance that reaches before the member's first output byte (there is
//     no preset dictionary);
//   - output past the claim, or less than it;
//   - a trailer that does not fit, a CRC-32 or an ISIZE that differs from the
//     output's;
//   - bytes after the trailer, unless they begin with 1f 8b: a second member
//     is CDC_E_UNSUPPORTED (Go's reader would concatenate it; its writer makes
//     none).
// Stricter than zlib in one place: zlib accepts a literal/length set that is a
// single one-bit end-of-block code; this walker calls it incomplete.
// A stream of 2 GiB or more is CDC_E_UNSUPPORTED (indices are 32-bit).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INFW_HD __host__ __device__ inline
#else
#define INFW_HD inline
#endif
// A value every lane holds alike, said to the device compiler.
#if defined(__HIP_DEVICE_COMPILE__)
#define INFW_UNI(x) uint32_t(__builtin_amdgcn_readfirstlane(int(x)))
#else
#define INFW_UNI(x) uint32_t(x)
#endif

namespace infw {

enum { kOk = 0, kCorrupt = -1, kUnsupported = -2 };

constexpr uint32_t kLitBits = 10, kDistBits = 8;  // primary lookups; longer codes take the canonical walk
constexpr uint32_t kMaxLit = 288, kMaxDist = 32, kMaxRatio = 1032;
constexpr uint32_t kMaxStream = 0x7FFFFFFFu;
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// One set of code tables (a wave's own in LDS, or the fixed code's).  A
// primary entry is symbol << 4 | length, 0 where the index is no complete code
// of at most the primary's bits.  sym holds the symbols sorted by length, then
// value; cnt the number of codes of each length.
struct Tables {
    uint16_t lit[1u << kLitBits];
    uint16_t dist[1u << kDistBits];
    uint16_t litsym[kMaxLit], distsym[kMaxDist], clsym[20];
    uint16_t litcnt[16], distcnt[16], clcnt[16];
    uint8_t lens[kMaxLit + kMaxDist];  // a dynamic block's HLIT + HDIST lengths
    uint8_t cllens[20];
};

struct Serial {
    uint32_t lane = 0, nl = 1;
    INFW_HD void sync() {}
};

// ---- CRC-32 (reflected, polynomial 0xEDB88320) ------------------------------------
INFW_HD uint32_t crc_bits(uint32_t reg, uint32_t byte)  // one byte, bit by bit
{
    reg ^= byte;
    for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ ((reg & 1u) ? kCrcPoly : 0u);
    return reg;
}

// a(x) b(x) mod P in the reflected representation (bit 31 is x^0).
INFW_HD uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

// x^e mod P: multiplying a register by it is feeding e / 8 zero bytes.
INFW_HD uint32_t crc_xpow(uint32_t e)
{
    uint32_t r = 0x80000000u, b = 0x40000000u;
    for (; e; e >>= 1) {
        if (e & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
    }
    return r;
}

// x^(8 bytes) mod P for crc_mul (the polynomial is primitive: exponents count mod 2^32 - 1).
INFW_HD uint32_t crc_shift(uint64_t bytes) { return crc_xpow(uint32_t(8 * bytes % 0xFFFFFFFFull)); }

// The lanes' slices: the n bytes, with 64 S - n zero bytes imagined before
// them, are cut into 64 slices of S bytes.  A register of 0 passes leading
// zeros unchanged, so the slice that holds byte 0 starts from 0xFFFFFFFF there
// and every other from 0.  [lo, hi) are the slice's real bytes.
INFW_HD uint32_t crc_slice_len(uint64_t n) { return uint32_t((n + 63) / 64); }
INFW_HD void crc_slice(uint64_t n, uint32_t lane, uint64_t &lo, uint64_t &hi, uint32_t &init)
{
    const uint64_t S = crc_slice_len(n), pad = 64 * S - n;
    const uint64_t v0 = S * lane, v1 = v0 + S;
    lo = v0 > pad ? v0 - pad : 0;
    hi = v1 > pad ? v1 - pad : 0;
    init = (hi > 0 && lo == 0) ? 0xFFFFFFFFu : 0u;
}

// ---- code tables ------------------------------------------------------------------
// The canonical walk (bits: the stream's next bits, first bit lowest): the
// symbol and its length, or -1 when no code of at most maxlen bits matches.
INFW_HD int canon(uint32_t bits, const uint16_t *cnt, const uint16_t *sym, uint32_t maxlen, uint32_t &len)
{
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= maxlen; ++l) {
        code |= bits & 1u;
        bits >>= 1;
        const uint32_t c = cnt[l];
        if (code >= first && code - first < c) {
            len = l;
            return int(sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

enum Kind { kCl = 0, kLit = 1, kDist = 2 };

// zlib's rules for a set of code lengths, from the counts per length.
INFW_HD bool counts_ok(const uint16_t *cnt, Kind kind)
{
    int32_t left = 1;
    uint32_t total = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left <<= 1;
        left -= int32_t(cnt[l]);
        if (left < 0) return false;  // over-subscribed
        total += cnt[l];
    }
    if (left == 0) return true;
    return kind == kDist && (total == 0 || (total == 1 && cnt[1] == 1));  // incomplete
}

// cnt, sym and (pbits != 0) the primary lookup of the n lengths in lens.
// False when the set is not allowed; the primary is then left unbuilt.
template <class Par>
INFW_HD bool build_code(Par &par, const uint8_t *lens, uint32_t n, Kind kind, uint16_t *cnt, uint16_t *sym,
                        uint16_t *prim, uint32_t pbits)
{
    par.sync();  // earlier readers of these tables are done
    for (uint32_t k = par.lane; k < 16; k += par.nl) {  // count per length
        uint32_t c = 0;
        if (k)
            for (uint32_t s = 0; s < n; ++s) c += lens[s] == k;
        cnt[k] = uint16_t(c);
    }
    par.sync();
    for (uint32_t k = 1 + par.lane; k < 16; k += par.nl) {  // each length's symbols, in order
        uint32_t at = 0;
        for (uint32_t l = 1; l < k; ++l) at += cnt[l];
        if (cnt[k])
            for (uint32_t s = 0; s < n; ++s)
                if (lens[s] == k) sym[at++] = uint16_t(s);
    }
    par.sync();
    uint16_t c[16];
    for (uint32_t l = 0; l < 16; ++l) c[l] = uint16_t(INFW_UNI(cnt[l]));
    if (!counts_ok(c, kind)) return false;
    if (pbits) {
        for (uint32_t i = par.lane; i < (1u << pbits); i += par.nl) {  // each lane fills its entries
            uint32_t len = 0;
            const int s = canon(i, cnt, sym, pbits, len);
            prim[i] = s < 0 ? uint16_t(0) : uint16_t(uint32_t(s) << 4 | len);
        }
        par.sync();
    }
    return true;
}

template <class Par>
INFW_HD void build_fixed(Par &par, Tables &T)
{
    for (uint32_t s = par.lane; s < kMaxLit; s += par.nl) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    for (uint32_t s = par.lane; s < kMaxDist; s += par.nl) T.lens[kMaxLit + s] = 5;
    build_code(par, T.lens, kMaxLit, kLit, T.litcnt, T.litsym, T.lit, kLitBits);
    build_code(par, T.lens + kMaxLit, kMaxDist, kDist, T.distcnt, T.distsym, T.dist, kDistBits);
}

// ---- the bit stream -----------------------------------------------------------------
template <class Rd>
struct Bits {
    Rd &rd;
    uint32_t n, ip;  // ip: the next byte to load
    uint64_t buf;
    uint32_t cnt;
    INFW_HD void refill()
    {
        while (cnt <= 56 && ip < n) {
            buf |= uint64_t(rd(ip++)) << cnt;
            cnt += 8;
        }
    }
    INFW_HD uint32_t peek(uint32_t k) const { return uint32_t(buf) & ((1u << k) - 1u); }  // k <= 16; zeros past the end
    INFW_HD bool drop(uint32_t k)
    {
        if (k > cnt) return false;  // the input ended
        buf >>= k;
        cnt -= k;
        return true;
    }
    INFW_HD bool take(uint32_t k, uint32_t &v)
    {
        v = peek(k);
        return drop(k);
    }
    // To the next byte boundary; the byte index there.  The buffer is emptied.
    INFW_HD uint32_t align()
    {
        const uint32_t at = ip - cnt / 8;
        buf = 0;
        cnt = 0;
        ip = at;
        return at;
    }
};

template <class Rd>
INFW_HD int decode_sym(Bits<Rd> &B, const uint16_t *prim, uint32_t pbits, const uint16_t *cnt, const uint16_t *sym)
{
    const uint32_t bits = B.peek(15);
    uint32_t len = 0;
    int s;
    const uint32_t e = pbits ? INFW_UNI(prim[bits & ((1u << pbits) - 1u)]) : 0u;
    if (e) {
        s = int(e >> 4);
        len = e & 15u;
    } else {
        s = canon(bits, cnt, sym, 15, len);
        if (s < 0) return -1;
        s = int(INFW_UNI(s));
        len = INFW_UNI(len);
    }
    return B.drop(len) ? s : -1;
}

// A dynamic block's header: the lengths into T.lens, the tables built.
template <class Rd, class Par>
INFW_HD bool read_dynamic(Bits<Rd> &B, Tables &T, Par &par)
{
    static_assert(sizeof(T.lens) >= 286 + 30, "lens holds HLIT + HDIST");
    uint32_t v;
    B.refill();
    if (!B.take(14, v)) return false;
    const uint32_t nlit = (v & 31u) + 257, ndist = ((v >> 5) & 31u) + 1, ncl = (v >> 10) + 4;
    if (nlit > 286 || ndist > 30) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    par.sync();
    for (uint32_t i = 0; i < 19; ++i) {
        uint32_t l = 0;
        if (i < ncl) {
            B.refill();
            if (!B.take(3, l)) return false;
        }
        T.cllens[order[i]] = uint8_t(l);
    }
    if (!build_code(par, T.cllens, 19, kCl, T.clcnt, T.clsym, nullptr, 0)) return false;
    const uint32_t total = nlit + ndist;
    uint32_t i = 0, prev = 0;
    while (i < total) {
        B.refill();
        const int s = decode_sym(B, nullptr, 0, T.clcnt, T.clsym);
        if (s < 0) return false;
        if (s < 16) {
            T.lens[i++] = uint8_t(s);
            prev = uint32_t(s);
            continue;
        }
        uint32_t rep, fill = 0;
        if (s == 16) {
            if (i == 0) return false;  // nothing to repeat
            if (!B.take(2, rep)) return false;
            rep += 3;
            fill = prev;
        } else if (s == 17) {
            if (!B.take(3, rep)) return false;
            rep += 3;
        } else {
            if (!B.take(7, rep)) return false;
            rep += 11;
        }
        if (rep > total - i) return false;  // a run past HLIT + HDIST
        for (uint32_t k = 0; k < rep; ++k) T.lens[i + k] = uint8_t(fill);
        i += rep;
        prev = fill;
    }
    par.sync();
    if (INFW_UNI(T.lens[256]) == 0) return false;  // no end-of-block code
    if (!build_code(par, T.lens, nlit, kLit, T.litcnt, T.litsym, T.lit, kLitBits)) return false;
    return build_code(par, T.lens + nlit, ndist, kDist, T.distcnt, T.distsym, T.dist, kDistBits);
}

// The DEFLATE stream that starts at byte ip0 of rd[0, n): kOk with `opos` the
// bytes produced (<= omax) and `end` the index of the byte after the last
// block, or kCorrupt.  Every sink call lies inside [0, omax) and its sources
// inside the input or the output before it.
//
// kStop is the stop mode (prefix Decode): omax is then the number of bytes
// wanted, and output that would pass it is no fault.  The literal, match or
// stored block that crosses the cut is cut to the byte (a stored block's bytes
// past the cut need not lie inside the input), the sink is flushed, `stopped`
// is set and the walk ends with kOk; `end` is then not set.  Once omax bytes
// are out, nothing read after them can fail the walk: a block header, a code
// set or a code that is not well formed ends it the same way, stopped.  Only a
// walk that reaches the end of the final block with stopped == false has seen
// the whole stream, judged as the full walk judges it.
template <bool kStop, class Rd, class Sink, class Par>
INFW_HD int inflate_walk(Rd &rd, uint32_t n, uint32_t ip0, Sink &sink, uint32_t omax, Tables &dyn, const Tables &fixed,
                         Par &par, uint32_t &opos, uint32_t &end, bool &stopped)
{
    Bits<Rd> B{rd, n, ip0, 0, 0};
    opos = 0;
    stopped = false;
    // A fault: kCorrupt, or in the stop mode with everything wanted out, the end of the walk.
#define INFW_FAIL()                        \
    do {                                   \
        if (kStop && opos >= omax) {       \
            sink.flush();                  \
            stopped = true;                \
            return kOk;                    \
        }                                  \
        return kCorrupt;                   \
    } while (0)
    for (;;) {
        uint32_t hdr;
        B.refill();
        if (!B.take(3, hdr)) INFW_FAIL();
        const uint32_t btype = hdr >> 1;
        if (btype == 3) INFW_FAIL();
        if (btype == 0) {
            B.drop(B.cnt & 7u);
            const uint32_t at = B.align();
            if (n - at < 4) INFW_FAIL();
            uint32_t len = rd(at) | rd(at + 1) << 8;
            const uint32_t nlen = rd(at + 2) | rd(at + 3) << 8;
            if ((len ^ nlen) != 0xFFFFu) INFW_FAIL();
            const bool cut = kStop && len > omax - opos;
            if (cut) len = omax - opos;
            if (len > n - (at + 4) || len > omax - opos) INFW_FAIL();
            if (len) sink.stored(opos, at + 4, len);
            opos += len;
            if (cut) {
                sink.flush();
                stopped = true;
                return kOk;
            }
            B.ip = at + 4 + len;
        } else {
            if (btype == 2 && !read_dynamic(B, dyn, par)) INFW_FAIL();
            const Tables &T = btype == 2 ? dyn : fixed;
            for (;;) {
                B.refill();  // 15 + 5 + 15 + 13 bits at the most until the next refill
                const int s = decode_sym(B, T.lit, kLitBits, T.litcnt, T.litsym);
                if (s < 0) INFW_FAIL();
                if (s < 256) {
                    if (opos >= omax) INFW_FAIL();
                    sink.lit(opos, uint32_t(s));
                    ++opos;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) INFW_FAIL();
                const uint32_t c = uint32_t(s) - 257;
                uint32_t len, x;
                if (c < 8) {
                    len = 3 + c;
                } else if (c == 28) {
                    len = 258;
                } else {
                    const uint32_t e = (c >> 2) - 1;
                    if (!B.take(e, x)) INFW_FAIL();
                    len = 3 + ((4 + (c & 3u)) << e) + x;
                }
                const int d = decode_sym(B, T.dist, kDistBits, T.distcnt, T.distsym);
                if (d < 0 || d > 29) INFW_FAIL();
                uint32_t dist;
                if (d < 4) {
                    dist = 1 + uint32_t(d);
                } else {
                    const uint32_t e = (uint32_t(d) >> 1) - 1;
                    if (!B.take(e, x)) INFW_FAIL();
                    dist = 1 + ((2 + (uint32_t(d) & 1u)) << e) + x;
                }
                if (dist > opos) INFW_FAIL();
                if (len > omax - opos) {
                    if (!kStop) return kCorrupt;
                    len = omax - opos;
                    if (len) sink.match(opos, dist, len);
                    opos += len;
                    sink.flush();
                    stopped = true;
                    return kOk;
                }
                sink.match(opos, dist, len);
                opos += len;
            }
        }
        sink.flush();
        if (hdr & 1u) break;
    }
#undef INFW_FAIL
    B.drop(B.cnt & 7u);
    end = B.align();
    return kOk;
}

template <class Rd, class Sink, class Par>
INFW_HD int inflate_body(Rd &rd, uint32_t n, uint32_t ip0, Sink &sink, uint32_t omax, Tables &dyn, const Tables &fixed,
                         Par &par, uint32_t &opos, uint32_t &end)
{
    bool stopped;
    return inflate_walk<false>(rd, n, ip0, sink, omax, dyn, fixed, par, opos, end, stopped);
}

// The stop mode of inflate_body: the first `stop` bytes of the stream.
template <class Rd, class Sink, class Par>
INFW_HD int inflate_body_stop(Rd &rd, uint32_t n, uint32_t ip0, Sink &sink, uint32_t stop, Tables &dyn,
                              const Tables &fixed, Par &par, uint32_t &opos, uint32_t &end, bool &stopped)
{
    return inflate_walk<true>(rd, n, ip0, sink, stop, dyn, fixed, par, opos, end, stopped);
}

// ---- the member --------------------------------------------------------------------
template <class Rd>
INFW_HD uint32_t le32(Rd &rd, uint32_t i)
{
    return rd(i) | rd(i + 1) << 8 | rd(i + 2) << 16 | rd(i + 3) << 24;
}

// The header of the member rd[0, n): kOk and hlen (the body's first byte).
template <class Rd>
INFW_HD int member_header(Rd &rd, uint32_t n, uint32_t &hlen)
{
    if (n < 10) return kCorrupt;
    if (rd(0) != 0x1Fu || rd(1) != 0x8Bu || rd(2) != 8u) return kCorrupt;
    const uint32_t flg = rd(3);
    if (flg & 0xE0u) return kCorrupt;
    uint32_t p = 10;
    if (flg & 4u) {  // FEXTRA
        if (n - p < 2) return kCorrupt;
        const uint32_t xlen = rd(p) | rd(p + 1) << 8;
        p += 2;
        if (n - p < xlen) return kCorrupt;
        p += xlen;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: to the zero byte
        if (!(flg & f)) continue;
        for (;;) {
            if (p >= n) return kCorrupt;
            if (rd(p++) == 0) break;
        }
    }
    if (flg & 2u) {  // FHCRC
        if (n - p < 2) return kCorrupt;
        uint32_t reg = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < p; ++i) reg = crc_bits(reg, rd(i));
        if (((reg ^ 0xFFFFFFFFu) & 0xFFFFu) != (rd(p) | rd(p + 1) << 8)) return kCorrupt;
        p += 2;
    }
    hlen = p;
    return kOk;
}

// Sizing: the header, the trailer's place, the claim (ISIZE) and whether
// DEFLATE can reach it.  n == 0 is the empty blob (claim 0, hlen 0).
template <class Rd>
INFW_HD int member_claim(Rd &rd, uint64_t n64, uint32_t &hlen, uint32_t &claim)
{
    hlen = claim = 0;
    if (n64 == 0) return kOk;
    if (n64 > kMaxStream) return kUnsupported;
    const uint32_t n = uint32_t(n64);
    const int st = member_header(rd, n, hlen);
    if (st != kOk) return st;
    if (n - hlen < 8) return kCorrupt;
    claim = le32(rd, n - 4);
    if (uint64_t(claim) > uint64_t(kMaxRatio) * (n - hlen - 8)) return kCorrupt;
    return kOk;
}

// After the body: the trailer at `end` against the output (its CRC-32 and
// length), then what follows the trailer.
template <class Rd>
INFW_HD int member_trailer(Rd &rd, uint32_t n, uint32_t end, uint32_t opos, uint32_t crc)
{
    if (n - end < 8) return kCorrupt;
    if (le32(rd, end) != crc || le32(rd, end + 4) != opos) return kCorrupt;
    const uint32_t rest = n - (end + 8);
    if (rest == 0) return kOk;
    return (rest >= 2 && rd(end + 8) == 0x1Fu && rd(end + 9) == 0x8Bu) ? kUnsupported : kCorrupt;
}

// ---- serial sinks (host) -------------------------------------------------------------
struct CountSink {
    INFW_HD void lit(uint32_t, uint32_t) {}
    INFW_HD void match(uint32_t, uint32_t, uint32_t) {}
    INFW_HD void stored(uint32_t, uint32_t, uint32_t) {}
    INFW_HD void flush() {}
};

template <class Rd>
struct MemSink {
    uint8_t *dst;
    Rd &rd;
    INFW_HD void lit(uint32_t o, uint32_t b) { dst[o] = uint8_t(b); }
    INFW_HD void match(uint32_t o, uint32_t dist, uint32_t len)
    {
        for (uint32_t i = 0; i < len; ++i) dst[o + i] = dst[o - dist + (dist >= len ? i : i % dist)];
    }
    INFW_HD void stored(uint32_t o, uint32_t src, uint32_t len)
    {
        for (uint32_t i = 0; i < len; ++i) dst[o + i] = uint8_t(rd(src + i));
    }
    INFW_HD void flush() {}
};

}  // namespace infw
