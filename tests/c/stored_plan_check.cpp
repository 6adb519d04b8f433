// Stand-alone check of plakar_amd/csrc/stored_plan.h (host only), built with
// -fsanitize=address,undefined by tests/test_stored_packfile_cpu.py.
//
// The tail split and the index range are compared with a brute-force
// restatement of the layout (snapshot/snapshot.go:249-267, info.go:387-426)
// that is written from the file's front, not from its end, and enumerates
// candidates instead of computing them:
//   * every file length 0..300 with every value of the last byte, both
//     versions around 100, with and without a coded repository;
//   * 10,000 seeded random trailers over larger lengths;
//   * index ranges: every index offset around the footer's start and counts
//     around each compression's expansion bound;
//   * the writer's trailer read back by the tail split.
// The file's bytes sit in exactly-sized heap buffers so that a read past either
// end is a sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stored_plan.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// The layout from the front: the file is [data+index: p][footer code: L][v0 v1 v2 v3][L].
// Accept when some split (p, L) with p + L + 5 == len has the last byte equal to L;
// every L is tried.
struct Brute {
    bool ok;
    uint64_t footer_off;
    uint32_t L, version;
};
static Brute brute_tail(const std::vector<uint8_t> &file, bool coded)
{
    Brute b{false, 0, 0, 0};
    const uint64_t len = file.size();
    for (uint64_t L = 0; L <= 255 && L + 5 <= len; ++L)
        for (uint64_t p = len - L - 5; p + L + 5 == len; ++p) {  // the one data-and-index length that fits this L
            if (file[size_t(len - 1)] != L) continue;
            uint32_t v = 0;
            for (int k = 3; k >= 0; --k) v = v << 8 | file[size_t(p + L + k)];
            if (v != 100) continue;
            if (L == 0 && coded) continue;
            b = Brute{true, p, uint32_t(L), v};
        }
    return b;
}

static uint64_t n_accept = 0, n_reject = 0, n_ranges = 0;

static void check_tail(const std::vector<uint8_t> &file, bool coded)
{
    const uint64_t len = file.size();
    // the last five bytes in a buffer of their own: the planner may read no others
    std::vector<uint8_t> last(file.end() - (len < 5 ? len : 5), file.end());
    stplan::Tail t;
    const int st = stplan::split_tail(last.data(), len, coded, &t);
    const Brute b = brute_tail(file, coded);
    REQUIRE(st == CDC_OK || st == CDC_E_CORRUPT);
    REQUIRE((st == CDC_OK) == b.ok);
    if (b.ok) {
        REQUIRE(t.footer_off == b.footer_off && t.L == b.L && t.version == b.version);
        REQUIRE(t.footer_off + t.L + 5 == len);
        ++n_accept;
    } else {
        ++n_reject;
    }
}

static void put32(uint8_t *p, uint32_t v)
{
    for (int k = 0; k < 4; ++k) p[k] = uint8_t(v >> (8 * k));
}

static uint64_t brute_bound(uint64_t enc, int compress, bool encrypted)
{
    uint64_t frame = enc;
    if (encrypted) {
        if (enc < 60) return 0;
        // records of at most 12 + 65536 + 16 bytes after the 60-byte header
        uint64_t rem = enc - 60;
        frame = 0;
        while (rem) {
            const uint64_t rec = rem < 65564 ? rem : 65564;
            if (rec < 28) return 0;  // no room for a nonce and a tag: Decode refuses the blob
            frame += rec - 28;
            rem -= rec;
        }
    }
    return frame * (compress == CDC_COMPRESS_GZIP ? 1032u : compress == CDC_COMPRESS_LZ4 ? 255u : 1u);
}

static void check_range(uint64_t footer_off, uint32_t L, uint32_t fversion, uint32_t count, uint32_t index_offset,
                        uint64_t footer_len, int compress, bool encrypted)
{
    stplan::Tail t{100, L, footer_off};
    std::vector<uint8_t> footer(size_t(footer_len), 0);
    if (footer_len >= 52) {
        put32(footer.data(), fversion);
        put32(footer.data() + 12, count);
        put32(footer.data() + 16, index_offset);
        for (int k = 0; k < 32; ++k) footer[size_t(20 + k)] = uint8_t(k * 7 + 1);
    }
    cdc_packfile_footer f;
    stplan::IndexRange r;
    const int st = stplan::index_range(footer.data(), footer_len, t, compress, encrypted, &f, &r);
    bool ok = footer_len == 52 && fversion == 100 && index_offset <= footer_off;
    if (ok) ok = 41ull * count <= brute_bound(footer_off - index_offset, compress, encrypted);
    REQUIRE(st == (ok ? CDC_OK : CDC_E_CORRUPT));
    if (ok) {
        REQUIRE(r.off == index_offset && r.off + r.len == footer_off && r.plain == 41ull * count);
        REQUIRE(f.count == count && f.index_offset == index_offset && f.version == 100 && f.index_checksum[31] == 218);
    }
    ++n_ranges;
}

int main()
{
    // every length 0..300, every last byte, versions 99..101, coded or not
    const uint32_t versions[] = {100, 99, 101};
    for (uint64_t len = 0; len <= 300; ++len)
        for (uint32_t last = 0; last < 256; ++last)
            for (uint32_t v : versions)
                for (int coded = 0; coded < 2; ++coded) {
                    std::vector<uint8_t> file(size_t(len), 0xA5);
                    if (len >= 5) put32(file.data() + (len - 5), v);
                    if (len >= 1) file[size_t(len - 1)] = uint8_t(last);
                    check_tail(file, coded != 0);
                }
    // 10,000 random trailers
    for (int it = 0; it < 10000; ++it) {
        const uint64_t len = rnd() % 2000;
        std::vector<uint8_t> file(size_t(len), 0);
        for (auto &b : file) b = uint8_t(rnd());
        if (len >= 5 && rnd() % 4) put32(file.data() + (len - 5), rnd() % 8 ? 100 : 100u | uint32_t(1u << (rnd() % 32)));
        if (len >= 1 && rnd() % 2) file[size_t(len - 1)] = uint8_t(rnd() % (len < 255 ? len + 2 : 256));
        check_tail(file, rnd() % 2 != 0);
    }
    // index ranges
    const int comps[] = {CDC_COMPRESS_NONE, CDC_COMPRESS_LZ4, CDC_COMPRESS_GZIP};
    for (int c : comps)
        for (int enc = 0; enc < 2; ++enc) {
            for (uint64_t footer_off : {0ull, 1ull, 41ull, 59ull, 60ull, 88ull, 89ull, 129ull, 1000ull, 70000ull, 200000ull})
                for (uint64_t back = 0; back <= footer_off + 2 && back <= 300; ++back) {
                    const uint32_t io = back <= footer_off ? uint32_t(footer_off - back) : uint32_t(footer_off + (back - footer_off));
                    const uint64_t bound = brute_bound(footer_off >= io ? footer_off - io : 0, c, enc != 0) / 41;
                    for (int64_t d = -2; d <= 2; ++d) {
                        const int64_t cnt = int64_t(bound) + d;
                        if (cnt < 0 || cnt > 0xFFFFFFFFll) continue;
                        check_range(footer_off, 71, 100, uint32_t(cnt), io, 52, c, enc != 0);
                    }
                    check_range(footer_off, 71, 100, 1u << 31, io, 52, c, enc != 0);
                    check_range(footer_off, 71, 100, 0xFFFFFFFFu, io, 52, c, enc != 0);
                }
            check_range(1000, 71, 101, 0, 0, 52, c, enc != 0);
            check_range(1000, 71, 100, 0, 0, 51, c, enc != 0);
            check_range(1000, 71, 100, 0, 0, 53, c, enc != 0);
            check_range(1000, 71, 100, 0, 0, 0, c, enc != 0);
            // 2^31 rows over a 100-byte index
            check_range(100, 71, 100, 1u << 31, 0, 52, c, enc != 0);
        }
    for (int it = 0; it < 10000; ++it) {
        const uint64_t footer_off = rnd() % 300000;
        const uint32_t io = uint32_t(rnd() % (footer_off + 3));
        check_range(footer_off, uint32_t(rnd() % 256), rnd() % 16 ? 100 : uint32_t(rnd()), uint32_t(rnd() >> (rnd() % 40 + 24)), io,
                    rnd() % 16 ? 52 : rnd() % 100, comps[rnd() % 3], rnd() % 2 != 0);
    }
    // the writer's trailer, read back
    for (uint64_t ef = 0; ef <= 300; ++ef) {
        uint8_t tr[5];
        uint64_t total = 0;
        const uint64_t data = rnd() % 1000, ei = rnd() % 1000;
        const int st = stplan::make_trailer(data, ei, ef, tr, &total);
        REQUIRE(st == (ef < 256 ? CDC_OK : CDC_E_UNSUPPORTED));
        if (st != CDC_OK) continue;
        REQUIRE(total == data + ei + ef + 5);
        stplan::Tail t;
        REQUIRE(stplan::split_tail(tr, total, false, &t) == CDC_OK);
        REQUIRE(t.L == ef && t.footer_off == data + ei && t.version == 100);
    }
    std::printf("%" PRIu64 " accepted, %" PRIu64 " rejected, %" PRIu64 " ranges, ok\n", n_accept, n_reject, n_ranges);
    return 0;
}
