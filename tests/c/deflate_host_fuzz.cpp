// CPU safety net of GZIP Encode's DEFLATE writer (plakar_amd/csrc/deflate_enc.h,
// the header the device kernels take symbol mapping, match splitting, code
// lengths, canonical codes, the dynamic header and block sizes from), built with
//   g++ -fsanitize=address,undefined
// and linked with the system's zlib only.  Every table lives in a heap buffer
// of exactly its size, so one entry read or written out of range is a
// sanitizer report.
//
//   deflate_host_fuzz [--out FILE]
//
// 1. Seeded histograms through build_lengths: each set is checked here (lengths
//    within the limit, Kraft sum exactly 1, at least two codes, every used
//    symbol coded) and printed for the test to judge again:
//      H <name> <limit> <n> <length> ...
// 2. Whole members written on the host from hand-made record lists, span by
//    span as the device does (histograms, lengths, header, choice at the running
//    bit position, packing by stretches).  The size computed for each block must
//    equal the bits written; zlib must inflate each member to the content.  With
//    --out each member goes to FILE as u32 length, member, u32 length, content,
//    and a line
//      M <name> <member bytes> <content bytes> <stored> <fixed> <dynamic>
//    counts its blocks by kind.
// 3. The member's CRC-32 as the device assembles it, restated serially with the
//    shared functions (inflate_walk.h: crc_bits, crc_mul, crc_shift): a register
//    from zero over every 128-byte stretch, moved to its span's end; the spans'
//    registers moved to the member's end; the 0xFFFFFFFF start moved past the
//    whole length; the complement.  Against zlib's crc32 over random contents:
//      C <bytes> <crc32 in hex>
//    and the shift alone over 2^29 + 3 zero bytes, where 8 * bytes passes 2^32:
//      S <bytes> <crc32 in hex>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../plakar_amd/csrc/deflate_enc.h"
#include "../../plakar_amd/csrc/inflate_walk.h"

#if __has_include(<zlib.h>)
#include <zlib.h>
#else
extern "C" {  // zlib's ABI (1.2.x, LP64) where its header is not installed
typedef struct z_stream_s {
    const unsigned char *next_in;
    unsigned avail_in;
    unsigned long total_in;
    unsigned char *next_out;
    unsigned avail_out;
    unsigned long total_out;
    const char *msg;
    void *state, *zalloc, *zfree, *opaque;
    int data_type;
    unsigned long adler, reserved;
} z_stream;
const char *zlibVersion(void);
int inflateInit2_(z_stream *, int, const char *, int);
int inflate(z_stream *, int);
int inflateEnd(z_stream *);
unsigned long crc32(unsigned long, const unsigned char *, unsigned);
}
#define Z_FINISH 4
#define Z_STREAM_END 1
#define Z_OK 0
#define inflateInit2(s, w) inflateInit2_((s), (w), zlibVersion(), int(sizeof(z_stream)))
#endif

typedef std::vector<uint8_t> Bytes;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 16);
}

static int g_fail = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            printf("FAIL %s: ", #c);          \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            ++g_fail;                         \
        }                                     \
    } while (0)

// ---- 1. histograms ---------------------------------------------------------------------
static void lengths_case(const char *name, const std::vector<uint32_t> &freq, uint32_t limit)
{
    const uint32_t n = uint32_t(freq.size());
    // exactly-sized heap copies: the builder reads freq[0, n) and writes lens[0, n)
    std::unique_ptr<uint32_t[]> f(new uint32_t[n]);
    std::unique_ptr<uint8_t[]> lens(new uint8_t[n]);
    std::unique_ptr<dfl::CodeWork> W(new dfl::CodeWork);
    memcpy(f.get(), freq.data(), n * 4);
    memset(lens.get(), 0xEE, n);
    dfl::Serial par;
    dfl::build_lengths(par, f.get(), n, limit, lens.get(), *W);
    uint64_t kraft = 0;
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s) {
        CHECK(lens[s] <= limit, "%s: symbol %u has %u bits", name, s, lens[s]);
        CHECK(!freq[s] || lens[s], "%s: used symbol %u has no code", name, s);
        if (lens[s] && lens[s] <= limit) {
            kraft += 1ull << (limit - lens[s]);
            ++used;
        }
    }
    CHECK(kraft == 1ull << limit, "%s: Kraft sum %llu / %llu", name, (unsigned long long)kraft, 1ull << limit);
    CHECK(used >= 2, "%s: %u codes", name, used);
    std::unique_ptr<uint16_t[]> codes(new uint16_t[n]);
    dfl::assign_codes(par, lens.get(), n, codes.get());
    for (uint32_t s = 0; s < n; ++s)  // prefix-free: no two codes equal on the shorter one's bits
        for (uint32_t t = s + 1; t < n && n <= 64; ++t)
            if (lens[s] && lens[t]) {
                const uint32_t l = lens[s] < lens[t] ? lens[s] : lens[t], mask = (1u << l) - 1u;
                CHECK((codes[s] & mask) != (codes[t] & mask), "%s: codes of %u and %u collide", name, s, t);
            }
    printf("H %s %u %u", name, limit, n);
    for (uint32_t s = 0; s < n; ++s) printf(" %u", lens[s]);
    printf("\n");
}

static void histogram_cases()
{
    std::vector<uint32_t> f;
    // Fibonacci-like: the unlimited tree is a chain, 39 deep
    f.assign(286, 0);
    {
        uint32_t a = 1, b = 1;
        for (uint32_t i = 0; i < 40; ++i) {
            f[3 * i] = a;
            const uint32_t c = a + b;
            a = b;
            b = c;
        }
    }
    f[256] = 1;
    lengths_case("fib-lit", f, 15);
    f.assign(30, 0);
    {
        uint32_t a = 1, b = 2;
        for (uint32_t i = 0; i < 30; ++i) {
            f[i] = a;
            const uint32_t c = a + b;
            a = b;
            b = c;
        }
    }
    lengths_case("fib-dist", f, 15);
    f.assign(286, 0);
    f[256] = 1;
    lengths_case("one-used-lit", f, 15);       // only the end-of-block symbol
    f.assign(30, 0);
    lengths_case("none-used-dist", f, 15);     // a block without matches: two one-bit codes
    f[0] = 9;
    lengths_case("one-used-dist-0", f, 15);
    f.assign(30, 0);
    f[17] = 9;
    lengths_case("one-used-dist-17", f, 15);
    f.assign(30, 0);
    f[3] = 5;
    f[29] = 1;
    lengths_case("two-used-dist", f, 15);
    f.assign(286, 0);
    f[256] = 1;
    f['x'] = 31000;
    lengths_case("eob-and-one-literal", f, 15);
    f.assign(286, 1);
    lengths_case("all-286-equal", f, 15);
    for (uint32_t i = 0; i < 286; ++i) f[i] = 1 + (rnd() % 1000) * (rnd() % 7 == 0 ? 100 : 1);
    lengths_case("all-286-random", f, 15);
    for (uint32_t i = 0; i < 286; ++i) f[i] = 1u << (i % 24);
    lengths_case("all-286-powers", f, 15);
    f.assign(30, 1);
    lengths_case("all-30-equal", f, 15);
    for (uint32_t i = 0; i < 30; ++i) f[i] = 1u << i;
    lengths_case("all-30-powers", f, 15);
    // the code-length code: 19 symbols, 7 bits
    f.assign(19, 0);
    {
        uint32_t a = 1, b = 1;
        for (uint32_t i = 0; i < 19; ++i) {
            f[i] = a;
            const uint32_t c = a + b;
            a = b;
            b = c;
        }
    }
    lengths_case("fib-cl", f, 7);
    for (uint32_t i = 0; i < 19; ++i) f[i] = 1u << i;
    lengths_case("powers-cl", f, 7);
    f.assign(19, 0);
    f[18] = 2;
    lengths_case("one-used-cl", f, 7);
    f.assign(19, 0);
    f[0] = 100;
    f[8] = 1;
    lengths_case("two-used-cl", f, 7);
    for (int k = 0; k < 200; ++k) {  // seeded: sparse and dense, flat and steep
        const uint32_t n = k % 3 == 0 ? 286 : k % 3 == 1 ? 30 : 19, limit = n == 19 ? 7 : 15;
        f.assign(n, 0);
        const uint32_t dens = 1 + rnd() % 8, steep = rnd() % 23;
        for (uint32_t i = 0; i < n; ++i)
            if (rnd() % dens == 0) f[i] = 1 + (rnd() >> (9 + rnd() % (steep + 1)));
        char name[32];
        snprintf(name, sizeof name, "seeded-%d", k);
        lengths_case(name, f, limit);
    }
}

// ---- 2. members ------------------------------------------------------------------------
struct Blob {
    Bytes content;
    std::vector<std::vector<dfl::Rec>> recs;  // per 8-KiB segment
};

struct ByteRd {
    const uint8_t *p;
    uint32_t operator()(uint32_t i) const { return p[i]; }
};

// The member of a blob, span by span as the device writes it.
static Bytes encode_member(const Blob &b, uint32_t kinds[3])
{
    using namespace dfl;
    const uint64_t len = b.content.size();
    const uint64_t cap_words = (member_bound(len) + 3) / 4 + 2;
    std::unique_ptr<uint32_t[]> words(new uint32_t[cap_words]());
    const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    Serial par;
    {
        BitW<Serial> B(par, words.get(), 0);
        for (int i = 0; i < 10; ++i) B.put(hdr[i], 8);
        B.flush();
    }
    uint64_t P = 80;
    const uint32_t nspan = uint32_t((len + kSpan - 1) / kSpan);
    for (uint32_t sp = 0; sp < nspan; ++sp) {
        const uint32_t slen = uint32_t(len - uint64_t(sp) * kSpan < kSpan ? len - uint64_t(sp) * kSpan : kSpan);
        // an exactly-sized copy of the span: a read past it is a report
        std::unique_ptr<uint8_t[]> data(new uint8_t[slen]);
        memcpy(data.get(), b.content.data() + uint64_t(sp) * kSpan, slen);
        ByteRd rd{data.get()};
        SpanView V{};
        V.len = slen;
        for (uint32_t g = 0; g < kSpanSegs; ++g) {
            const size_t sg = size_t(sp) * kSpanSegs + g;
            V.rec[g] = sg < b.recs.size() ? b.recs[sg].data() : nullptr;
            V.nrec[g] = sg < b.recs.size() ? uint32_t(b.recs[sg].size()) : 0u;
        }
        std::unique_ptr<uint32_t[]> lfreq(new uint32_t[kLitSlots]()), dfreq(new uint32_t[kDistSlots]());
        uint32_t xbits = 0;
        span_hist(par, V, rd, lfreq.get(), dfreq.get(), &xbits);
        std::unique_ptr<uint8_t[]> llen(new uint8_t[kNLit]), dlen(new uint8_t[kNDist]);
        std::unique_ptr<CodeWork> W(new CodeWork);
        std::unique_ptr<HdrWork> H(new HdrWork);
        build_lengths(par, lfreq.get(), kNLit, 15, llen.get(), *W);
        build_lengths(par, dfreq.get(), kNDist, 15, dlen.get(), *W);
        header_tokens(llen.get(), dlen.get(), *H);
        build_lengths(par, H->clfreq, kNCl, 7, H->cllen, *W);
        assign_codes(par, H->cllen, kNCl, H->clcode);
        std::unique_ptr<uint32_t[]> hw(new uint32_t[kHdrWords]());
        const uint32_t hdr_bits = write_header(*H, hw.get());
        CHECK(hdr_bits <= 32 * kHdrWords, "header of %u bits", hdr_bits);
        const uint32_t dyn_bits = 3 + hdr_bits + body_bits(lfreq.get(), dfreq.get(), llen.get(), dlen.get(), xbits);
        const uint32_t fixed_bits = 3 + body_bits(lfreq.get(), dfreq.get(), nullptr, nullptr, xbits);
        uint64_t bits;
        const uint32_t type = choose_block(P, slen, fixed_bits, dyn_bits, bits);
        const bool final = sp + 1 == nspan;
        ++kinds[type];
        if (type == kStored) {
            BitW<Serial> B(par, words.get(), P);
            B.put(final ? 1u : 0u, 3);
            B.flush();
            const uint64_t A = (P + 3 + 7) / 8;
            BitW<Serial> D(par, words.get(), 8 * A);
            D.put(slen, 16);
            D.put(slen ^ 0xFFFFu, 16);
            for (uint32_t i = 0; i < slen; ++i) D.put(data[i], 8);
            D.flush();
            CHECK(D.pos() == P + bits, "stored block: %llu bits planned, %llu written", (unsigned long long)bits,
                  (unsigned long long)(D.pos() - P));
        } else {
            std::unique_ptr<Codes> C(new Codes);
            load_codes(par, *C, type == kDynamic ? llen.get() : nullptr, type == kDynamic ? dlen.get() : nullptr);
            std::unique_ptr<uint32_t[]> sbits(new uint32_t[kStretches]);
            span_count(par, V, rd, *C, sbits.get());
            const uint64_t end = span_pack(par, V, rd, *C, sbits.get(), type, final, hw.get(), hdr_bits, words.get(), P);
            CHECK(end == P + bits, "block of kind %u: %llu bits planned, %llu written", type, (unsigned long long)bits,
                  (unsigned long long)(end - P));
        }
        P += bits;
    }
    const uint64_t body_end = (P + 7) / 8;
    CHECK(body_end + 8 <= member_bound(len), "member of %llu bytes past its bound", (unsigned long long)(body_end + 8));
    Bytes out(body_end + 8);
    for (uint64_t i = 0; i < body_end; ++i) out[i] = uint8_t(words[i >> 2] >> (8 * (i & 3)));
    const uint32_t crc = uint32_t(crc32(0, b.content.data(), unsigned(len)));
    for (int i = 0; i < 4; ++i) {
        out[body_end + i] = uint8_t(crc >> (8 * i));
        out[body_end + 4 + i] = uint8_t(uint32_t(len) >> (8 * i));
    }
    return out;
}

static bool zlib_inflates(const Bytes &m, const Bytes &content)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 31) != Z_OK) return false;
    Bytes out(content.size() + 16);
    z.next_in = const_cast<uint8_t *>(m.data());
    z.avail_in = unsigned(m.size());
    z.next_out = out.data();
    z.avail_out = unsigned(out.size());
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.total_out == content.size() && z.avail_in == 0 &&
                    memcmp(out.data(), content.data(), content.size()) == 0;
    inflateEnd(&z);
    return ok;
}

// Appends a literal run and then a match to the blob's current segment (a new
// segment when the match would not fit in this one).
struct Maker {
    Blob b;
    void lits(uint32_t n, bool random)
    {
        for (uint32_t i = 0; i < n; ++i) b.content.push_back(random ? uint8_t(rnd()) : uint8_t("plakar chunk "[rnd() % 13]));
    }
    void pad_segment()
    {
        while (b.content.size() % dfl::kSeg) b.content.push_back(uint8_t('a' + rnd() % 4));
    }
    void match(uint32_t off, uint32_t len)
    {
        uint32_t p = uint32_t(b.content.size() % dfl::kSeg);
        if (p + len > dfl::kSeg || p == 0) {
            pad_segment();
            lits(40, false);
            p = 40;
        }
        if (off > p) off = p;
        const size_t seg = b.content.size() / dfl::kSeg;
        if (b.recs.size() <= seg) b.recs.resize(seg + 1);
        b.recs[seg].push_back(dfl::Rec{p | off << 16, len});
        for (uint32_t i = 0; i < len; ++i) b.content.push_back(b.content[b.content.size() - off]);
    }
};

static void member_case(const char *name, const Blob &b, FILE *out)
{
    uint32_t kinds[3] = {0, 0, 0};
    const Bytes m = encode_member(b, kinds);
    CHECK(zlib_inflates(m, b.content), "%s: zlib does not inflate the member to the content", name);
    printf("M %s %zu %zu %u %u %u\n", name, m.size(), b.content.size(), kinds[0], kinds[1], kinds[2]);
    if (out) {
        const uint32_t a = uint32_t(m.size()), c = uint32_t(b.content.size());
        fwrite(&a, 4, 1, out);
        fwrite(m.data(), 1, a, out);
        fwrite(&c, 4, 1, out);
        fwrite(b.content.data(), 1, c, out);
    }
}

static void member_cases(FILE *out)
{
    {  // every record length 4..1100 (every residue mod 258, remainders 1 and 2 among them), offsets 1..
        Maker M;
        for (uint32_t L = 4; L <= 1100; ++L) {
            M.lits(rnd() % 4, false);
            M.match(1 + (L * 7) % 300, L);
        }
        member_case("lengths-4-1100", M.b, out);
    }
    {  // back to back, and the longest a segment holds
        Maker M;
        M.lits(1, false);
        for (uint32_t L : {259u, 260u, 258u, 516u, 517u, 518u, 257u, 4u, 5u, 774u, 775u, 776u}) M.match(1, L);
        M.pad_segment();
        M.lits(3, false);
        M.match(3, dfl::kSeg - 3);
        M.lits(5, false);
        M.match(2, 8000);
        member_case("back-to-back", M.b, out);
    }
    {  // literals only: text-like (a code), then random (stored), then a tail
        Maker M;
        M.lits(40000, false);
        M.lits(70000, true);
        M.lits(33000, false);
        M.lits(777, true);
        member_case("literals-coded-and-stored", M.b, out);
    }
    {  // spans that alternate between records and random bytes: stored blocks that start mid-byte
        Maker M;
        for (int k = 0; k < 6; ++k) {
            while (M.b.content.size() % dfl::kSpan < dfl::kSpan - 700) {
                M.lits(1 + rnd() % 9, false);
                M.match(1 + rnd() % 4000, 4 + rnd() % 600);
            }
            while (M.b.content.size() % dfl::kSpan) M.lits(1, false);
            M.lits(dfl::kSpan, true);
        }
        M.lits(19, false);
        member_case("alternating", M.b, out);
    }
    for (uint32_t n : {1u, 2u, 3u, 127u, 128u, 129u, 8191u, 8192u, 8193u, 32767u, 32768u, 32769u}) {
        Maker M;
        M.lits(n, false);
        char name[32];
        snprintf(name, sizeof name, "text-%u", n);
        member_case(name, M.b, out);
        Maker Z;
        Z.b.content.assign(n, 0);
        for (uint32_t s = 0; s * dfl::kSeg < n; ++s) {  // what the match search finds in zeros
            const uint32_t sl = n - s * dfl::kSeg < dfl::kSeg ? n - s * dfl::kSeg : dfl::kSeg;
            Z.b.recs.resize(s + 1);
            if (sl >= 5) Z.b.recs[s].push_back(dfl::Rec{1u | 1u << 16, sl - 1});
        }
        snprintf(name, sizeof name, "zeros-%u", n);
        member_case(name, Z.b, out);
    }
    for (int k = 0; k < 40; ++k) {  // seeded mixes
        Maker M;
        const uint32_t target = 1 + rnd() % 90000;
        while (M.b.content.size() < target) {
            const uint32_t what = rnd() % 10;
            if (what < 6) {
                M.lits(rnd() % 12, rnd() % 5 == 0);
                M.match(1 + rnd() % 8000, 4 + (rnd() % 8 ? rnd() % 40 : rnd() % 2000));
            } else if (what < 9) {
                M.lits(rnd() % 300, false);
            } else {
                M.lits(rnd() % 9000, true);
            }
        }
        char name[32];
        snprintf(name, sizeof name, "seeded-%d", k);
        member_case(name, M.b, out);
    }
}

// ---- 3. the CRC-32's assembly ----------------------------------------------------------
// What k_dfl_size (stretches into a span's register) and k_gz_fin (spans into
// the member's CRC-32) compute, one term after the other.
static uint32_t assembled_crc(const uint8_t *p, uint64_t len)
{
    using namespace dfl;
    uint32_t acc = 0;
    const uint64_t nspan = (len + kSpan - 1) / kSpan;
    for (uint64_t k = 0; k < nspan; ++k) {
        const uint64_t s0 = k * kSpan, done = len < s0 + kSpan ? len : s0 + kSpan;
        const uint32_t slen = uint32_t(done - s0);
        uint32_t span = 0;
        for (uint32_t a = 0; a < slen; a += kStretch) {
            const uint32_t e = a + kStretch < slen ? a + kStretch : slen;
            uint32_t r = 0;
            for (uint32_t i = a; i < e; ++i) r = infw::crc_bits(r, p[s0 + i]);
            if (r) r = infw::crc_mul(r, infw::crc_shift(slen - e));
            span ^= r;
        }
        acc ^= infw::crc_mul(span, infw::crc_shift(len - done));
    }
    return ~(acc ^ infw::crc_mul(0xFFFFFFFFu, infw::crc_shift(len)));
}

static void crc_cases()
{
    for (uint64_t n : {1ull, 127ull, 128ull, 129ull, 32767ull, 32768ull, 32769ull, (2ull << 20) + 1, (4ull << 20) + 5,
                       (8ull << 20) + 3}) {
        std::unique_ptr<uint8_t[]> data(new uint8_t[n]);  // exactly sized: a read past it is a report
        for (uint64_t i = 0; i < n; ++i) data[i] = uint8_t(rnd());
        const uint32_t want = uint32_t(crc32(0, data.get(), unsigned(n))), got = assembled_crc(data.get(), n);
        CHECK(got == want, "CRC-32 of %llu bytes: assembled %08x, zlib %08x", (unsigned long long)n, got, want);
        printf("C %llu %08x\n", (unsigned long long)n, got);
    }
    // the shift alone: a register moved past 2^29 + 3 zero bytes (8 * bytes = 2^32 + 24: the
    // exponent is reduced mod 2^32 - 1, not cut to 32 bits); zlib is fed the zeros 1 MiB at a time
    const uint64_t zeros = (1ull << 29) + 3;
    CHECK(8 * zeros > 0xFFFFFFFFull, "the exponent passes 2^32");
    const uint8_t head[5] = {'s', 'h', 'i', 'f', 't'};
    unsigned long z = crc32(0, head, 5);
    const uint32_t got = ~infw::crc_mul(~uint32_t(z), infw::crc_shift(zeros));  // zlib keeps the register complemented
    std::unique_ptr<uint8_t[]> mib(new uint8_t[1 << 20]());
    for (uint64_t left = zeros; left;) {
        const unsigned k = unsigned(left < (1u << 20) ? left : (1u << 20));
        z = crc32(z, mib.get(), k);
        left -= k;
    }
    CHECK(got == uint32_t(z), "a register moved past %llu zero bytes: %08x, zlib %08x", (unsigned long long)zeros, got,
          uint32_t(z));
    CHECK(infw::crc_shift(zeros) == infw::crc_xpow(25) && infw::crc_shift(zeros) != infw::crc_xpow(24),
          "x^(2^32 + 24) is x^25 mod P, not x^24");
    printf("S %llu %08x\n", (unsigned long long)zeros, got);
}

int main(int argc, char **argv)
{
    FILE *out = nullptr;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--out") && i + 1 < argc) out = fopen(argv[++i], "wb");
    // symbol mapping and splitting, exhaustively
    for (uint32_t l = 3; l <= 258; ++l) {
        uint32_t s, eb, ex;
        dfl::len_sym(l, s, eb, ex);
        const uint32_t c = s - 257, e = c < 8 || c == 28 ? 0 : (c >> 2) - 1;
        const uint32_t back = c < 8 ? 3 + c : c == 28 ? 258 : 3 + ((4 + (c & 3u)) << e) + ex;
        CHECK(s >= 257 && s <= 285 && eb == e && ex < (1u << eb) && back == l, "length %u -> symbol %u", l, s);
    }
    for (uint32_t d = 1; d <= 32768; ++d) {
        uint32_t s, eb, ex;
        dfl::dist_sym(d, s, eb, ex);
        const uint32_t e = s < 4 ? 0 : (s >> 1) - 1;
        const uint32_t back = s < 4 ? 1 + s : 1 + ((2 + (s & 1u)) << e) + ex;
        CHECK(s <= 29 && eb == e && ex < (1u << eb) && back == d, "distance %u -> symbol %u", d, s);
    }
    for (uint32_t L = 4; L <= 9000; ++L) {
        uint32_t sum = 0;
        const uint32_t n = dfl::split_count(L);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t p = dfl::split_piece(L, k);
            CHECK(p >= 3 && p <= 258, "record %u piece %u is %u", L, k, p);
            sum += p;
        }
        CHECK(sum == L, "record %u splits into %u bytes", L, sum);
    }
    for (uint64_t P = 0; P < 64; ++P)
        CHECK(dfl::stored_bits(P, 7) == ((P + 3 + 7) / 8 * 8 - P) + 32 + 56 && (P + dfl::stored_bits(P, 7)) % 8 == 0,
              "stored block at bit %llu", (unsigned long long)P);
    histogram_cases();
    member_cases(out);
    if (out) fclose(out);
    crc_cases();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("ok\n");
    return 0;
}
