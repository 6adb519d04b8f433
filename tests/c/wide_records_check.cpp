// The DEFLATE writer (plakar_amd/csrc/deflate_enc.h) on records that reach
// before their segment, as the wide match search (CDC_LEVEL_WIDE) writes them:
// stand-alone, compiled by tests/test_wide_cpu.py under the address and
// undefined-behaviour sanitizers.  Members are built span by span as the device
// builds them, from hand-made record lists over 2-6 segments; zlib inflates
// each one here, and the test walks them with inflate_ref.
//
//   wide_records_check --out FILE
// prints per case "M name member-bytes content-bytes matches max-distance",
// writes (u32 n, member, u32 k, content) to FILE twice per case, the member
// with dynamic and with fixed blocks, and ends with "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <memory>
#include <vector>

#include "../../plakar_amd/csrc/deflate_enc.h"

using Bytes = std::vector<uint8_t>;

static int g_fail = 0;
#define CHECK(c, ...)                      \
    do {                                   \
        if (!(c)) {                        \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);           \
            printf("\n");                  \
            ++g_fail;                      \
        }                                  \
    } while (0)

static uint32_t g_seed = 12345;
static uint32_t rnd()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

struct Blob {
    Bytes content;
    std::vector<std::vector<dfl::Rec>> recs;  // per 8-KiB segment
    std::vector<uint32_t> hist;               // per segment
};

struct ByteRd {
    const uint8_t *p;
    uint32_t operator()(uint32_t i) const { return p[i]; }
};

struct Collect {  // what a walk yields
    uint32_t lits = 0, matches = 0, max_off = 0, bytes = 0;
    std::vector<uint32_t> offs;
    void lit(uint32_t) { ++lits; ++bytes; }
    void match(uint32_t off, uint32_t len)
    {
        ++matches;
        bytes += len;
        if (off > max_off) max_off = off;
        offs.push_back(off);
    }
};

// The member of a blob, span by span as the device writes it (k_dfl_size,
// k_dfl_emit), every block in the form `type` (fixed or dynamic): each
// block's computed size must be the bits written.
static Bytes encode_member(const Blob &b, uint32_t type)
{
    using namespace dfl;
    const uint64_t len = b.content.size();
    const uint64_t cap_words = (2 * len + 4096) / 4;  // the fixed code on random bytes is longer than the bound of a planned member
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
        std::unique_ptr<uint8_t[]> data(new uint8_t[slen]);  // an exactly-sized copy: a read past the span is a report
        memcpy(data.get(), b.content.data() + uint64_t(sp) * kSpan, slen);
        ByteRd rd{data.get()};
        SpanView V{};
        V.len = slen;
        for (uint32_t g = 0; g < kSpanSegs; ++g) {
            const size_t sg = size_t(sp) * kSpanSegs + g;
            V.rec[g] = sg < b.recs.size() ? b.recs[sg].data() : nullptr;
            V.nrec[g] = sg < b.recs.size() ? uint32_t(b.recs[sg].size()) : 0u;
            V.hist[g] = sg < b.hist.size() ? b.hist[sg] : 0u;
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
        const uint32_t dyn_bits = 3 + hdr_bits + body_bits(lfreq.get(), dfreq.get(), llen.get(), dlen.get(), xbits);
        const uint32_t fixed_bits = 3 + body_bits(lfreq.get(), dfreq.get(), nullptr, nullptr, xbits);
        // the asked form, not the plan's choice: the filler between the records is random, and a stored
        // block would write none of them
        const uint32_t planned = type == kDynamic ? dyn_bits : fixed_bits;
        std::unique_ptr<Codes> C(new Codes);
        load_codes(par, *C, type == kDynamic ? llen.get() : nullptr, type == kDynamic ? dlen.get() : nullptr);
        std::unique_ptr<uint32_t[]> sbits(new uint32_t[kStretches]);
        span_count(par, V, rd, *C, sbits.get());
        const uint64_t end = span_pack(par, V, rd, *C, sbits.get(), type, sp + 1 == nspan, hw.get(), hdr_bits, words.get(), P);
        CHECK(end == P + planned, "span %u as kind %u: %u bits planned, %llu written", sp, type, planned,
              (unsigned long long)(end - P));
        P += planned;
    }
    const uint64_t body_end = (P + 7) / 8;
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

// What every walk of the blob yields, segment by segment.
static Collect collect(const Blob &b)
{
    Collect c;
    for (size_t sg = 0; sg * dfl::kSeg < b.content.size(); ++sg) {
        const uint32_t sl = uint32_t(b.content.size() - sg * dfl::kSeg < dfl::kSeg ? b.content.size() - sg * dfl::kSeg : dfl::kSeg);
        const dfl::Rec *r = sg < b.recs.size() ? b.recs[sg].data() : nullptr;
        const uint32_t n = sg < b.recs.size() ? uint32_t(b.recs[sg].size()) : 0u;
        dfl::walk(r, n, sg < b.hist.size() ? b.hist[sg] : 0u, 0, sl, c);
    }
    return c;
}

// Content and records made together: literals, then records at the running
// position whose bytes are the copy they name (real) or fresh bytes (a record
// the writer must refuse: its bytes are literals whatever it claims).
struct Maker {
    Blob b;
    uint32_t level_hist(size_t seg) const { return uint32_t(seg * dfl::kSeg < dfl::kMaxDist ? seg * dfl::kSeg : dfl::kMaxDist); }
    void lits(uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i) b.content.push_back(uint8_t("plakar wide chunk"[rnd() % 17]));
    }
    void to_segment(size_t seg, uint32_t p)
    {
        CHECK(b.content.size() <= seg * dfl::kSeg + p, "the maker moves forward");
        while (b.content.size() < seg * dfl::kSeg + p) b.content.push_back(uint8_t(rnd()));  // random: nothing compresses by accident
    }
    void rec(uint32_t off, uint32_t len, bool real)
    {
        const size_t seg = b.content.size() / dfl::kSeg;
        const uint32_t p = uint32_t(b.content.size() % dfl::kSeg);
        CHECK(p + len <= dfl::kSeg, "a record's destination stays in its segment");
        if (b.recs.size() <= seg) b.recs.resize(seg + 1);
        b.recs[seg].push_back(dfl::Rec{p | off << 16, len});
        for (uint32_t i = 0; i < len; ++i)
            b.content.push_back(real ? b.content[b.content.size() - off] : uint8_t(rnd()));
    }
    void finish(bool wide)
    {
        const size_t nseg = (b.content.size() + dfl::kSeg - 1) / dfl::kSeg;
        b.recs.resize(nseg);
        b.hist.assign(nseg, 0);
        for (size_t s = 0; wide && s < nseg; ++s) b.hist[s] = level_hist(s);
    }
};

static Bytes member_case(const char *name, const Blob &b, uint32_t want_matches, uint32_t want_max, FILE *out)
{
    const Bytes m = encode_member(b, dfl::kDynamic), fx = encode_member(b, dfl::kFixed);
    CHECK(zlib_inflates(m, b.content), "%s: zlib does not inflate the dynamic member to the content", name);
    CHECK(zlib_inflates(fx, b.content), "%s: zlib does not inflate the fixed member to the content", name);
    const Collect c = collect(b);
    CHECK(c.bytes == b.content.size(), "%s: the walk covers %u of %zu bytes", name, c.bytes, b.content.size());
    CHECK(c.matches == want_matches, "%s: %u matches, %u expected", name, c.matches, want_matches);
    CHECK(c.max_off == want_max, "%s: the longest distance is %u, %u expected", name, c.max_off, want_max);
    printf("M %s %zu %zu %u %u\n", name, m.size(), b.content.size(), c.matches, c.max_off);
    for (const Bytes *w : {&m, &fx}) {
        if (!out) break;
        const uint32_t a = uint32_t(w->size()), k = uint32_t(b.content.size());
        fwrite(&a, 4, 1, out);
        fwrite(w->data(), 1, a, out);
        fwrite(&k, 4, 1, out);
        fwrite(b.content.data(), 1, k, out);
    }
    return m;
}

// The records every case is made of.  `bad`: the two records that reach one byte too far.
static Maker six_segments(bool bad)
{
    using namespace dfl;
    Maker M;
    M.lits(300);                                   // segment 0, hist 0
    M.rec(300, 40, true);                          // offset p + hist exactly, with hist 0 (the level-0 rule's edge)
    M.lits(7);
    M.rec(1, 500, true);                           // a run
    M.to_segment(1, 0);                            // segment 1, hist 8 KiB
    M.rec(1, 300, true);                           // overlapping copy at offset 1 from the segment's first byte
    M.lits(50);
    M.rec(kSeg + 350, 19, true);                   // p = 350: offset p + hist exactly: the blob's first byte
    if (bad) {
        M.lits(3);
        M.rec(kSeg + 372 + 1, 12, false);          // p = 372: offset p + hist + 1: before the blob
    }
    M.to_segment(2, 5);                            // segment 2, hist 16 KiB
    M.rec(2 * kSeg + 5, 4, true);
    M.to_segment(3, 100);                          // segment 3, hist 24 KiB
    M.rec(3 * kSeg + 100, 258, true);              // offset p + hist exactly, 24,676
    M.lits(9);
    M.rec(3 * kSeg, 259, true);
    M.to_segment(4, 0);                            // segment 4, hist 32 KiB
    M.rec(kMaxDist, 700, true);                    // p = 0: offset p + hist = 32,768 exactly, longer than 258
    M.lits(20);
    M.rec(kMaxDist, 1000, true);                   // p = 720: 32,768 is less than p + hist, and the limit
    M.to_segment(5, 100);                          // segment 5, hist 32 KiB
    if (bad) {
        M.rec(kMaxDist + 1, 30, false);            // 32,769: inside p + hist, past DEFLATE's window
        M.lits(4);
    }
    M.rec(kMaxDist, 5, true);
    M.to_segment(5, 4000);
    M.rec(kMaxDist - 1, 258 + 258 + 2, true);      // a last piece of 2: the pair before it is shortened
    M.lits(11);
    return M;
}

int main(int argc, char **argv)
{
    using namespace dfl;
    FILE *out = nullptr;
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--out")) out = fopen(argv[i + 1], "wb");

    {   // every record taken: hist of 0, 8, 16, 24 and 32 KiB
        Maker M = six_segments(false);
        M.finish(true);
        CHECK(M.b.hist.size() == 6 && M.b.hist[1] == 8192 && M.b.hist[3] == 24576 && M.b.hist[4] == 32768 && M.b.hist[5] == 32768,
              "the segments' hist");
        member_case("six-segments", M.b, 11, kMaxDist, out);
    }
    {   // the two records one byte too far come out as literals; the member still inflates
        Maker M = six_segments(true);
        M.finish(true);
        const Collect c = collect(M.b);
        for (uint32_t o : c.offs) CHECK(o != kMaxDist + 1 && o != kSeg + 372 + 1, "a refused record's distance %u was written", o);
        member_case("six-segments-two-refused", M.b, 11, kMaxDist, out);
    }
    {   // hist 0 everywhere: the level-0 rule.  The same records give what the
        // records that rule accepts (offset <= start) give alone.
        Maker M = six_segments(true);
        M.finish(false);
        Blob kept = M.b;
        uint32_t nkept = 0, max_off = 0;
        for (auto &seg : kept.recs) {
            std::vector<Rec> v;
            for (const Rec &r : seg)
                if ((r.x >> 16) - 1u < (r.x & 0xFFFFu) && r.y >= 4) {
                    v.push_back(r);
                    if ((r.x >> 16) > max_off) max_off = r.x >> 16;
                }
            nkept += uint32_t(v.size());
            seg = v;
        }
        CHECK(nkept == 2, "%u records lie inside their segment", nkept);
        const Bytes a = member_case("level-0-rule-all-records", M.b, nkept, max_off, out);
        const Bytes b = member_case("level-0-rule-kept-records", kept, nkept, max_off, out);
        CHECK(a == b, "with hist 0 the records that reach before their segment must be literals");
    }
    {   // two segments: the smallest blob with history
        Maker M;
        M.lits(kSeg - 3);
        M.to_segment(1, 0);
        M.rec(kSeg, 4, true);                      // p = 0: offset hist exactly, the blob's first byte
        M.rec(1, 6, true);
        M.lits(2);
        M.finish(true);
        member_case("two-segments", M.b, 2, kSeg, out);
    }
    if (out) fclose(out);
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("ok\n");
    return 0;
}
