// The DEFLATE writer (RFC 1951) of GZIP Encode: everything that decides whether
// an inflater can read the member is decided here.  cdc_encode.hip runs this
// text with one workgroup per span (256 lanes, tables in LDS) and
// tests/c/deflate_host_fuzz.cpp compiles the same text under plain g++ (address
// and undefined-behaviour sanitizers) against zlib.
//
// A blob is cut into spans of kSpanSegs match-search segments (32 KiB).  The
// match search's records (k_lz4_seq or k_lz_seq_wide: match start, offset,
// length, segment-relative, sorted, not overlapping, length >= 4; the offset
// reaches at most the segment's `hist` bytes before it, 0 for k_lz4_seq, and
// never past 32,768) are the input; what lies between the matches is
// literals.  A span becomes one block: stored, fixed Huffman or dynamic
// Huffman, whichever is smallest by exact bit count at the bit position where
// it starts (choose_block).
//
// The work inside a span is shared by "stretches" of kStretch bytes: a lane owns
// the symbols that start inside its stretch (the literals there and every piece
// of a match that starts there), so its work is bounded by the stretch and by
// one segment's longest match, never by the span.  The same walk (walk) feeds
// the histograms, the bit counts and the packing, so they agree by construction.
//
// Par is how the lanes share: lane, nl, sync(), add() and bor() (atomic add / or
// on a word the lanes share).  Serial{} is one lane.  Everything outside the
// `for (i = par.lane; ...; i += par.nl)` loops and the `par.lane == 0` parts is
// computed alike by every lane.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFL_HD __host__ __device__ inline
#else
#define DFL_HD inline
#endif

namespace dfl {

constexpr uint32_t kSeg = 8192;                  // the match search's segment
constexpr uint32_t kSpanSegs = 4;
constexpr uint32_t kSpan = kSeg * kSpanSegs;     // 32 KiB: one block, at most 65,535 bytes when stored
constexpr uint32_t kStretch = 128;
constexpr uint32_t kStretches = kSpan / kStretch;
constexpr uint32_t kNLit = 286, kNDist = 30, kNCl = 19, kEob = 256;
constexpr uint32_t kLitSlots = 288, kDistSlots = 32;
constexpr uint32_t kMaxTok = kNLit + kNDist;     // code lengths in a dynamic header, and its tokens at most
constexpr uint32_t kHdrWords = 96;               // >= (14 + 57 + 7 * kMaxTok) bits: see write_header
constexpr uint32_t kStored = 0, kFixed = 1, kDynamic = 2;
constexpr uint32_t kMaxDist = 32768;             // DEFLATE's window, and the wide match search's
constexpr uint64_t kMaxBlob = 0x7FFFFFFFull;     // ISIZE is 32 bits and Decode refuses 2 GiB or more

struct Rec {                                     // uint2 on the device
    uint32_t x;                                  // match start | offset << 16
    uint32_t y;                                  // length
};

struct Serial {
    uint32_t lane = 0, nl = 1;
    DFL_HD void sync() {}
    DFL_HD void add(uint32_t *p, uint32_t v) { *p += v; }
    DFL_HD void bor(uint32_t *p, uint32_t v) { *p |= v; }
};

// ---- symbol mapping -------------------------------------------------------------------
DFL_HD uint32_t ilog2(uint32_t v)  // v >= 1
{
    uint32_t r = 0;
    while (v >>= 1) ++r;
    return r;
}

// Length 3..258: its literal/length symbol, the number of extra bits and their value.
DFL_HD void len_sym(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ex)
{
    const uint32_t m = len - 3;
    eb = ex = 0;
    if (len == 258) {
        sym = 285;
    } else if (m < 8) {
        sym = 257 + m;
    } else {
        eb = ilog2(m) - 2;
        sym = 257 + 4 * (eb + 1) + ((m >> eb) & 3u);
        ex = m & ((1u << eb) - 1u);
    }
}

// Distance 1..32768.
DFL_HD void dist_sym(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ex)
{
    const uint32_t m = dist - 1;
    eb = ex = 0;
    if (m < 4) {
        sym = m;
    } else {
        eb = ilog2(m) - 1;
        sym = 2 * (eb + 1) + ((m >> eb) & 1u);
        ex = m & ((1u << eb) - 1u);
    }
}

DFL_HD uint32_t fixed_lit_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// ---- match splitting --------------------------------------------------------------------
// A record of L >= 4 bytes is ceil(L / 258) pairs of 3..258 bytes that add up to
// L.  A last piece of 1 or 2 bytes is made 3 by shortening the pair before it.
DFL_HD uint32_t split_count(uint32_t L) { return (L + 257) / 258; }
DFL_HD uint32_t split_piece(uint32_t L, uint32_t k)
{
    const uint32_t n = split_count(L), r = L - (n - 1) * 258;  // 1..258
    if (r >= 3) return k + 1 < n ? 258u : r;
    if (k + 2 < n) return 258;
    return k + 2 == n ? 255 + r : 3;
}

// ---- the walk -------------------------------------------------------------------------
// Whether a record is written as a match.  The match search writes no offset
// of 0, none that reaches further than hist bytes before the segment or past
// DEFLATE's 32,768, and no length under 4: such a record's bytes are literals,
// in the range where it starts and in the ranges it reaches into.
DFL_HD bool rec_taken(const Rec &r, uint32_t hist)
{
    const uint32_t off = r.x >> 16;
    return off - 1u < (r.x & 0xFFFFu) + hist && off <= kMaxDist && r.y >= 4;
}

// The symbols that start in [p0, p1) of a segment, in order: f.lit(p) for a
// literal at p, f.match(offset, length) for a record that starts there.  A
// record that reaches into the range from before it covers the range's first
// bytes.  A record that starts before the walk's position (none is written by
// the match search) is passed over, its bytes literals.  hist: the bytes in
// front of the segment that a record's offset may reach (SpanView).
template <class F>
DFL_HD void walk(const Rec *rec, uint32_t nrec, uint32_t hist, uint32_t p0, uint32_t p1, F &f)
{
    uint32_t lo = 0, hi = nrec;  // the first record that starts at or after p0
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((rec[mid].x & 0xFFFFu) < p0) lo = mid + 1;
        else hi = mid;
    }
    uint32_t i = lo, p = p0;
    if (i > 0 && rec_taken(rec[i - 1], hist)) {
        const uint32_t e = (rec[i - 1].x & 0xFFFFu) + rec[i - 1].y;
        if (e > p) p = e;
    }
    while (p < p1) {
        while (i < nrec && (rec[i].x & 0xFFFFu) < p) ++i;
        if (i < nrec && (rec[i].x & 0xFFFFu) == p && rec_taken(rec[i], hist)) {
            const Rec r = rec[i++];
            f.match(r.x >> 16, r.y);
            p += r.y;
        } else {
            f.lit(p);
            ++p;
        }
    }
}

// A span as the walk sees it: its bytes through rd(i), i span-relative, and the
// records of its segments.
struct SpanView {
    const Rec *rec[kSpanSegs];
    uint32_t nrec[kSpanSegs];
    uint32_t len;
    uint32_t hist[kSpanSegs];  // bytes before each segment that its records may copy from (0: none)
};

// Stretch t of the span: its segment and range there; false past the span's end.
DFL_HD bool stretch_range(const SpanView &V, uint32_t t, uint32_t &seg, uint32_t &p0, uint32_t &p1)
{
    const uint32_t a = t * kStretch;
    if (a >= V.len) return false;
    seg = a / kSeg;
    p0 = a % kSeg;
    const uint32_t seg_len = V.len - seg * kSeg < kSeg ? V.len - seg * kSeg : kSeg;
    p1 = p0 + kStretch < seg_len ? p0 + kStretch : seg_len;
    return true;
}

// ---- histograms ---------------------------------------------------------------------------
template <class Par, class Rd>
struct HistF {
    Par &par;
    Rd &rd;
    uint32_t base;  // the segment's first byte in the span
    uint32_t *lfreq, *dfreq;
    uint32_t xbits;
    DFL_HD void lit(uint32_t p) { par.add(&lfreq[rd(base + p)], 1u); }
    DFL_HD void match(uint32_t off, uint32_t len)
    {
        uint32_t ds, de, dx;
        dist_sym(off, ds, de, dx);
        const uint32_t n = split_count(len);
        par.add(&dfreq[ds], n);
        xbits += n * de;
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t ls, le, lx;
            len_sym(split_piece(len, k), ls, le, lx);
            par.add(&lfreq[ls], 1u);
            xbits += le;
        }
    }
};

// lfreq[kLitSlots], dfreq[kDistSlots] and *xbits (the extra bits of all pairs)
// are zero on entry and shared by the lanes; the end-of-block symbol is counted.
template <class Par, class Rd>
DFL_HD void span_hist(Par &par, const SpanView &V, Rd &rd, uint32_t *lfreq, uint32_t *dfreq, uint32_t *xbits)
{
    for (uint32_t t = par.lane; t < kStretches; t += par.nl) {
        uint32_t seg, p0, p1;
        if (!stretch_range(V, t, seg, p0, p1)) break;
        HistF<Par, Rd> f{par, rd, seg * kSeg, lfreq, dfreq, 0};
        walk(V.rec[seg], V.nrec[seg], V.hist[seg], p0, p1, f);
        if (f.xbits) par.add(xbits, f.xbits);
    }
    if (par.lane == 0) par.add(&lfreq[kEob], 1u);
    par.sync();
}

// ---- code lengths ---------------------------------------------------------------------------
struct CodeWork {
    uint32_t w[2 * kLitSlots];       // weights, then depths, of the tree's nodes
    uint16_t parent[2 * kLitSlots];
    uint16_t order[kLitSlots];       // the used symbols by ascending (frequency, symbol)
    uint16_t cnt[16];
    uint32_t m;                      // used symbols, the forced ones included
    uint32_t force[2];               // symbols taken as used once (n: none)
};

DFL_HD uint32_t eff_freq(const uint32_t *freq, const CodeWork &W, uint32_t s)
{
    return freq[s] ? freq[s] : (s == W.force[0] || s == W.force[1]) ? 1u : 0u;
}

// Code lengths of at most `limit` bits for the n frequencies (their sum below
// 2^32): a Huffman code, and when that is deeper than the limit the counts per
// length are folded at the limit and repaired until the Kraft sum is 1 again
// (one code leaves the limit's level and a shorter code becomes two of the next
// length, the sum falling by one unit each time); the lengths are then dealt
// out by frequency.  At least two symbols are used (as zlib's build_tree forces
// them: the first unused ones count once), so the set is always complete:
// Kraft sum exactly 1.  n <= kLitSlots and n <= 2^limit.
template <class Par>
DFL_HD void build_lengths(Par &par, const uint32_t *freq, uint32_t n, uint32_t limit, uint8_t *lens, CodeWork &W)
{
    par.sync();
    if (par.lane == 0) {
        uint32_t used = 0;
        for (uint32_t s = 0; s < n; ++s) used += freq[s] != 0;
        W.force[0] = W.force[1] = n;
        for (uint32_t s = 0, k = 0; used < 2 && s < n; ++s)
            if (!freq[s]) {
                W.force[k++] = s;
                ++used;
            }
        W.m = used;
    }
    par.sync();
    for (uint32_t s = par.lane; s < n; s += par.nl) {  // rank sort
        lens[s] = 0;
        const uint32_t fs = eff_freq(freq, W, s);
        if (!fs) continue;
        uint32_t rank = 0;
        for (uint32_t t = 0; t < n; ++t) {
            const uint32_t ft = eff_freq(freq, W, t);
            rank += ft && (ft < fs || (ft == fs && t < s));
        }
        W.order[rank] = uint16_t(s);
    }
    par.sync();
    if (par.lane == 0) {
        const uint32_t m = W.m;
        // leaves 0..m-1 by ascending weight; internal nodes m.. are made in
        // ascending weight too, so the two smallest are at the two queues' heads
        for (uint32_t i = 0; i < m; ++i) W.w[i] = eff_freq(freq, W, W.order[i]);
        uint32_t leaf = 0, inode = m, nn = m;
        while (nn < 2 * m - 1) {
            uint32_t a[2];
            for (int k = 0; k < 2; ++k) {
                if (leaf < m && (inode >= nn || W.w[leaf] <= W.w[inode])) a[k] = leaf++;
                else a[k] = inode++;
            }
            W.w[nn] = W.w[a[0]] + W.w[a[1]];
            W.parent[a[0]] = W.parent[a[1]] = uint16_t(nn);
            ++nn;
        }
        for (uint32_t l = 0; l < 16; ++l) W.cnt[l] = 0;
        W.w[2 * m - 2] = 0;  // the root's depth; a parent's index is above its children's
        for (uint32_t i = 2 * m - 2; i-- > 0;) {
            W.w[i] = W.w[W.parent[i]] + 1;
            if (i < m) ++W.cnt[W.w[i] < limit ? W.w[i] : limit];
        }
        uint32_t total = 0;
        for (uint32_t l = 1; l <= limit; ++l) total += uint32_t(W.cnt[l]) << (limit - l);
        while (total > (1u << limit) && W.cnt[limit]) {
            --W.cnt[limit];
            for (uint32_t l = limit - 1; l >= 1; --l)
                if (W.cnt[l]) {
                    --W.cnt[l];
                    W.cnt[l + 1] = uint16_t(W.cnt[l + 1] + 2);
                    break;
                }
            --total;
        }
        uint32_t i = 0;  // the rarest symbols take the longest codes
        for (uint32_t l = limit; l >= 1; --l)
            for (uint32_t c = 0; c < W.cnt[l]; ++c) lens[W.order[i++]] = uint8_t(l);
    }
    par.sync();
}

DFL_HD uint32_t bit_reverse(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// Canonical codes (RFC 1951 3.2.2) of a complete or empty set, bit-reversed:
// DEFLATE packs Huffman codes from their most significant bit.
template <class Par>
DFL_HD void assign_codes(Par &par, const uint8_t *lens, uint32_t n, uint16_t *codes)
{
    for (uint32_t s = par.lane; s < n; s += par.nl) {
        const uint32_t l = lens[s];
        uint32_t code = 0;
        if (l)
            for (uint32_t t = 0; t < n; ++t) {
                const uint32_t lt = lens[t];
                if (lt && lt < l) code += 1u << (l - lt);
                else if (lt == l && t < s) ++code;
            }
        codes[s] = uint16_t(bit_reverse(code, l));
    }
    par.sync();
}

// ---- bits -----------------------------------------------------------------------------------
// Appends at a bit position of a zeroed word array that other lanes write too:
// whole words leave by par.bor like the partial ones at a range's two ends.
template <class Par>
struct BitW {
    Par &par;
    uint32_t *words;
    uint64_t acc;
    uint32_t fill, w;
    DFL_HD BitW(Par &p, uint32_t *words_, uint64_t bitpos)
        : par(p), words(words_), acc(0), fill(uint32_t(bitpos & 31u)), w(uint32_t(bitpos >> 5))
    {
    }
    DFL_HD void put(uint32_t v, uint32_t n)  // n <= 16 bits, v < 2^n
    {
        acc |= uint64_t(v) << fill;
        fill += n;
        if (fill >= 32) {
            par.bor(&words[w++], uint32_t(acc));
            acc >>= 32;
            fill -= 32;
        }
    }
    DFL_HD void flush()
    {
        if (fill) par.bor(&words[w], uint32_t(acc));  // the last partial word; pos() stays
    }
    DFL_HD uint64_t pos() const { return uint64_t(w) * 32 + fill; }
};

// ---- the dynamic header -----------------------------------------------------------------------
struct HdrWork {
    uint16_t tok[kMaxTok];  // code-length symbol | extra value << 5
    uint32_t ntok, nlit, ndist, ncl;
    uint32_t clfreq[kNCl + 1];
    uint8_t cllen[kNCl + 1];
    uint16_t clcode[kNCl + 1];
};

DFL_HD uint32_t cl_extra_bits(uint32_t s) { return s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u; }
DFL_HD uint32_t cl_order(uint32_t i)
{
    const uint8_t order[kNCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// One lane: HLIT and HDIST (trailing zero lengths dropped), the lengths of both
// sets as one sequence run-length coded by symbols 16 / 17 / 18, and the
// code-length symbols' frequencies.
DFL_HD void header_tokens(const uint8_t *llen, const uint8_t *dlen, HdrWork &H)
{
    uint32_t nlit = kNLit, ndist = kNDist;
    while (nlit > 257 && !llen[nlit - 1]) --nlit;
    while (ndist > 1 && !dlen[ndist - 1]) --ndist;
    H.nlit = nlit;
    H.ndist = ndist;
    for (uint32_t s = 0; s <= kNCl; ++s) H.clfreq[s] = 0;
    const uint32_t total = nlit + ndist;
    auto at = [&](uint32_t i) -> uint32_t { return i < nlit ? llen[i] : dlen[i - nlit]; };
    uint32_t nt = 0;
    auto tok = [&](uint32_t s, uint32_t x) {
        H.tok[nt++] = uint16_t(s | x << 5);
        ++H.clfreq[s];
    };
    uint32_t i = 0;
    while (i < total) {
        const uint32_t v = at(i);
        uint32_t run = 1;
        while (i + run < total && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const uint32_t r = run < 138 ? run : 138;
                tok(18, r - 11);
                run -= r;
            }
            if (run >= 3) {
                tok(17, run - 3);
                run = 0;
            }
            for (; run; --run) tok(0, 0);
        } else {
            tok(v, 0);
            --run;
            while (run >= 3) {
                const uint32_t r = run < 6 ? run : 6;
                tok(16, r - 3);
                run -= r;
            }
            for (; run; --run) tok(v, 0);
        }
    }
    H.ntok = nt;
}

// One lane, after the code-length code's lengths and codes are built: HCLEN, the
// header's size in bits, and (words != nullptr) its bits from bit 0 of the
// zeroed words.  A token costs at most 7 bits per length it covers (18: 14 bits
// for 11 or more, 16 and 17: 10 for 3 or more), so the header is at most
// 14 + 57 + 7 * kMaxTok bits: kHdrWords words hold it.
DFL_HD uint32_t write_header(HdrWork &H, uint32_t *words)
{
    uint32_t ncl = kNCl;
    while (ncl > 4 && !H.cllen[cl_order(ncl - 1)]) --ncl;
    H.ncl = ncl;
    uint32_t bits = 14 + 3 * ncl;
    for (uint32_t k = 0; k < H.ntok; ++k) {
        const uint32_t s = H.tok[k] & 31u;
        bits += H.cllen[s] + cl_extra_bits(s);
    }
    if (words) {
        Serial one;
        BitW<Serial> B(one, words, 0);
        B.put(H.nlit - 257, 5);
        B.put(H.ndist - 1, 5);
        B.put(ncl - 4, 4);
        for (uint32_t k = 0; k < ncl; ++k) B.put(H.cllen[cl_order(k)], 3);
        for (uint32_t k = 0; k < H.ntok; ++k) {
            const uint32_t s = H.tok[k] & 31u;
            B.put(H.clcode[s], H.cllen[s]);
            if (s >= 16) B.put(uint32_t(H.tok[k]) >> 5, cl_extra_bits(s));
        }
        B.flush();
    }
    return bits;
}

// ---- sizes ----------------------------------------------------------------------------------
// A block's bits after its 3 header bits and (dynamic) its code header.
DFL_HD uint32_t body_bits(const uint32_t *lfreq, const uint32_t *dfreq, const uint8_t *llen, const uint8_t *dlen,
                          uint32_t xbits)
{
    uint32_t bits = xbits;
    for (uint32_t s = 0; s < kNLit; ++s) bits += lfreq[s] * (llen ? llen[s] : fixed_lit_len(s));
    for (uint32_t s = 0; s < kNDist; ++s) bits += dfreq[s] * (dlen ? dlen[s] : 5u);
    return bits;
}

// A stored block of len <= 65,535 bytes that starts at bit P of the member: 3
// header bits, zeros to the next byte boundary, LEN, NLEN, the bytes.
DFL_HD uint64_t stored_bits(uint64_t P, uint32_t len) { return ((P + 3 + 7) & ~7ull) - P + 32 + 8ull * len; }

// The smallest of the three at bit P (fixed_bits and dyn_bits: whole blocks,
// the 3 header bits included).  A span is coded only when that is no larger
// than storing it; a tie between the codes goes to the fixed one.
DFL_HD uint32_t choose_block(uint64_t P, uint32_t len, uint32_t fixed_bits, uint32_t dyn_bits, uint64_t &bits)
{
    const uint64_t st = stored_bits(P, len);
    uint32_t type = kFixed;
    bits = fixed_bits;
    if (dyn_bits < bits) {
        type = kDynamic;
        bits = dyn_bits;
    }
    if (st < bits) {
        type = kStored;
        bits = st;
    }
    return type;
}

// The member of a blob of len > 0 bytes is at most this long: a span costs at
// most 5 bytes more than its content, whatever bit it starts at (the stored
// form ends on a byte boundary, and its header takes the rest of the byte the
// block before it ended in or one new byte), plus 10 bytes of header and 8 of
// trailer.  The bound handed out keeps 5 bytes more, and so also covers what
// zlib writes at level 0 for any length (an empty blob's 23 bytes included).
DFL_HD uint64_t member_bound(uint64_t len) { return len + 18 + 5 * ((len + kSpan - 1) / kSpan + 1); }

// ---- the stream form ----------------------------------------------------------------------------
// One member written piece by piece (cdc_gzip_stream_piece): a piece's blocks
// all have BFINAL clear, and an empty stored block after them (the joiner: 000,
// zeros to the byte boundary, LEN 0, NLEN ffff) ends the piece on a byte
// boundary, so the next piece starts at bit 0.  The last piece then adds the
// final empty stored block (01 00 00 ff ff), as Go's compress/flate writes on
// Close, before the member's CRC-32 and ISIZE.
DFL_HD uint64_t joiner_bits(uint64_t P) { return stored_bits(P, 0); }
constexpr uint32_t kFinalBytes = 5;

// The joiner where the piece's last block ended: o is the byte that holds that
// bit, sh the bit's place in it (0: a new byte) and edge the block's bits
// there.  With `final` the final block follows.  Returns the bytes written
// from o, the shared byte included: 5, or 6 from bit 6 on, and kFinalBytes more.
DFL_HD uint32_t stream_end(uint8_t *o, uint32_t edge, uint32_t sh, bool final)
{
    const uint32_t a = (sh + 3 + 7) >> 3;  // bytes up to LEN: the shared or new one, and one more from bit 6 on
    o[0] = uint8_t(sh ? edge & ((1u << sh) - 1u) : 0u);
    if (a > 1) o[1] = 0;
    o[a] = o[a + 1] = 0;
    o[a + 2] = o[a + 3] = 0xFF;
    uint32_t n = a + 4;
    if (final) {
        o[n] = 1;
        o[n + 1] = o[n + 2] = 0;
        o[n + 3] = o[n + 4] = 0xFF;
        n += kFinalBytes;
    }
    return n;
}

// The most one piece of len bytes writes: the ten header bytes (first piece),
// len and 5 bytes per span as in member_bound, 6 for the joiner, and the final
// block, CRC-32 and ISIZE (last piece).
DFL_HD uint64_t stream_piece_bound(uint64_t len) { return 10 + len + 5 * ((len + kSpan - 1) / kSpan) + 6 + kFinalBytes + 8; }

// ---- packing ----------------------------------------------------------------------------------
struct Codes {
    uint16_t lcode[kLitSlots], dcode[kDistSlots];
    uint8_t llen[kLitSlots], dlen[kDistSlots];
};

template <class Rd>
struct CountWalk {
    const Codes &C;
    Rd &rd;
    uint32_t base;
    uint32_t bits;
    DFL_HD void lit(uint32_t p) { bits += C.llen[rd(base + p)]; }
    DFL_HD void match(uint32_t off, uint32_t len)
    {
        uint32_t ds, de, dx;
        dist_sym(off, ds, de, dx);
        const uint32_t n = split_count(len);
        bits += n * (C.dlen[ds] + de);
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t ls, le, lx;
            len_sym(split_piece(len, k), ls, le, lx);
            bits += C.llen[ls] + le;
        }
    }
};

template <class Par, class Rd>
struct PackWalk {
    const Codes &C;
    Rd &rd;
    uint32_t base;
    BitW<Par> &B;
    DFL_HD void lit(uint32_t p)
    {
        const uint32_t s = rd(base + p);
        B.put(C.lcode[s], C.llen[s]);
    }
    DFL_HD void match(uint32_t off, uint32_t len)
    {
        uint32_t ds, de, dx;
        dist_sym(off, ds, de, dx);
        const uint32_t n = split_count(len);
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t ls, le, lx;
            len_sym(split_piece(len, k), ls, le, lx);
            B.put(C.lcode[ls], C.llen[ls]);
            if (le) B.put(lx, le);
            B.put(C.dcode[ds], C.dlen[ds]);
            if (de) B.put(dx, de);
        }
    }
};

// The fixed code's lengths, or the given ones, and their codes.
template <class Par>
DFL_HD void load_codes(Par &par, Codes &C, const uint8_t *llen, const uint8_t *dlen)
{
    par.sync();
    for (uint32_t s = par.lane; s < kLitSlots; s += par.nl) C.llen[s] = llen ? (s < kNLit ? llen[s] : 0) : uint8_t(fixed_lit_len(s));
    for (uint32_t s = par.lane; s < kDistSlots; s += par.nl) C.dlen[s] = dlen ? (s < kNDist ? dlen[s] : 0) : uint8_t(5);
    par.sync();
    assign_codes(par, C.llen, kLitSlots, C.lcode);
    assign_codes(par, C.dlen, kDistSlots, C.dcode);
}

// The bits of each stretch's symbols into sbits[kStretches] (0 past the span).
template <class Par, class Rd>
DFL_HD void span_count(Par &par, const SpanView &V, Rd &rd, const Codes &C, uint32_t *sbits)
{
    for (uint32_t t = par.lane; t < kStretches; t += par.nl) {
        uint32_t seg, p0, p1, bits = 0;
        if (stretch_range(V, t, seg, p0, p1)) {
            CountWalk<Rd> f{C, rd, seg * kSeg, 0};
            walk(V.rec[seg], V.nrec[seg], V.hist[seg], p0, p1, f);
            bits = f.bits;
        }
        sbits[t] = bits;
    }
    par.sync();
}

// The block at bit `at` of the zeroed words: its 3 header bits, the dynamic
// header's hdr_bits bits (hdr, from write_header), each stretch's symbols at the
// place the stretches before it leave, and the end-of-block code.  Returns the
// bit after the block, alike in every lane.
template <class Par, class Rd>
DFL_HD uint64_t span_pack(Par &par, const SpanView &V, Rd &rd, const Codes &C, const uint32_t *sbits, uint32_t type,
                          bool final, const uint32_t *hdr, uint32_t hdr_bits, uint32_t *words, uint64_t at)
{
    if (par.lane == 0) {
        BitW<Par> B(par, words, at);
        B.put((final ? 1u : 0u) | type << 1, 3);
        B.flush();
    }
    const uint64_t h0 = at + 3;
    if (type == kDynamic)
        for (uint32_t i = par.lane; i < (hdr_bits + 31) / 32; i += par.nl) {
            const uint64_t pos = h0 + 32ull * i;
            const uint32_t sh = uint32_t(pos & 31u), v = hdr[i];
            par.bor(&words[pos >> 5], v << sh);
            if (sh && (v >> (32 - sh))) par.bor(&words[(pos >> 5) + 1], v >> (32 - sh));
        }
    else
        hdr_bits = 0;
    const uint64_t s0 = h0 + hdr_bits;
    uint64_t total = 0;
    for (uint32_t t = 0; t < kStretches; ++t) total += sbits[t];
    for (uint32_t t = par.lane; t < kStretches; t += par.nl) {
        uint32_t seg, p0, p1;
        if (!stretch_range(V, t, seg, p0, p1)) break;
        uint64_t off = 0;
        for (uint32_t u = 0; u < t; ++u) off += sbits[u];
        BitW<Par> B(par, words, s0 + off);
        PackWalk<Par, Rd> f{C, rd, seg * kSeg, B};
        walk(V.rec[seg], V.nrec[seg], V.hist[seg], p0, p1, f);
        B.flush();
    }
    if (par.lane == 0) {
        BitW<Par> B(par, words, s0 + total);
        B.put(C.lcode[kEob], C.llen[kEob]);
        B.flush();
    }
    par.sync();
    return s0 + total + C.llen[kEob];
}

}  // namespace dfl
