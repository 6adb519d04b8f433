// Stand-alone checker of the check path's host-only code (check_plan.h,
// sha_blocks.h, hybrid_model.h), built by tests/test_check_cpu.py with
// -fsanitize=address,undefined together with the library's host SHA-256
// (cdc_sha256.cpp).
//
//   * run and seam planner: thousands of random segment lists (tiny, huge,
//     empty, repeated, overlapping) over a source in a heap buffer of exactly
//     its size, the seam area in one of exactly the reported size, so that any
//     access past an end is a sanitizer report.  The seam copies are replayed
//     with memcpy, then every object is read back through its runs: the exact
//     message, every run but the last a multiple of 64, every copy and run in
//     bounds, copies ascending and disjoint, the reported seam size the size
//     used.  Each object is then hashed the way k_object_digest walks it
//     (block by block, the run switched when it is used up, padding from
//     sha_blocks.h) and compared with SHA-256 of the message;
//   * block arithmetic: the blocks sha_blocks.h pads against a byte-wise
//     padding (FIPS 180-4, 5.1.1) for totals 0..300 and around 2^29, 2^32 and
//     2^35 bytes, whose 64-bit bit length no GPU test can afford to run;
//   * the split rule: no objects, all equal, one giant, host_min_len, empties.
//
// Prints "<p> plans, <o> objects, <t> totals, ok" and exits 0, or says what
// failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "cdc_internal.h"
#include "check_plan.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
            exit(1);                              \
        }                                         \
    } while (0)

// Block b of a message of `total` bytes as sha_blocks.h pads it; data(p) is
// message byte p.
template <class F>
static void shab_block(uint64_t total, uint64_t b, F data, uint8_t out[64])
{
    const int32_t r = shab::remaining(total, b);
    for (int q = 0; q < 16; ++q) {
        uint32_t w = 0;
        for (int j = 0; j < 4; ++j) {
            const uint64_t p = 64 * b + 4 * uint64_t(q) + uint64_t(j);
            w = (w << 8) | (p < total ? data(p) : 0xEEu);  // past the data: whatever the clamped load brought
        }
        if (shab::has_padding(r)) {
            w = (w & shab::keep_mask(r, q)) | shab::pad_byte(r, q);
            if (shab::has_length(r) && q == 14) w = shab::bits_hi(total);
            if (shab::has_length(r) && q == 15) w = shab::bits_lo(total);
        }
        for (int j = 0; j < 4; ++j) out[4 * q + j] = uint8_t(w >> (24 - 8 * j));
    }
}

// Byte p of the padded message, byte-wise: data, 0x80, zeros, the bit length big-endian.
template <class F>
static uint8_t padded_byte(uint64_t total, uint64_t p, F data)
{
    const uint64_t padded = (total + 9 + 63) / 64 * 64;
    if (p < total) return data(p);
    if (p == total) return 0x80;
    if (p >= padded - 8) {
        const unsigned i = unsigned(p - (padded - 8));  // 0: the most significant byte
        // total * 8 as a 64-bit number, without overflowing: byte i of it
        const unsigned shift = 8 * (7 - i);
        return uint8_t(shift >= 3 ? (total >> (shift - 3)) : (total << (3 - shift)));
    }
    return 0;
}

static uint64_t check_totals()
{
    uint64_t count = 0;
    auto data = [](uint64_t p) { return uint8_t((p * 131u + (p >> 7)) ^ 0x5Au); };
    std::vector<uint64_t> totals;
    for (uint64_t t = 0; t <= 300; ++t) totals.push_back(t);
    for (uint64_t c : {1ull << 29, 1ull << 32, 1ull << 35, (1ull << 61) - 200})
        for (uint64_t d = 0; d <= 130; ++d) {
            totals.push_back(c + d);
            totals.push_back(c - 1 - d);
        }
    for (uint64_t total : totals) {
        const uint64_t padded = (total + 9 + 63) / 64 * 64, nb = shab::blocks(total);
        CHECK(nb == padded / 64, "blocks(%llu) = %llu", (unsigned long long)total, (unsigned long long)nb);
        std::vector<uint64_t> bs;
        for (uint64_t b = nb > 4 ? nb - 4 : 0; b < nb; ++b) bs.push_back(b);
        if (nb > 4) {
            bs.push_back(0);
            bs.push_back(nb / 2);
        }
        for (uint64_t b : bs) {
            uint8_t got[64];
            shab_block(total, b, data, got);
            for (unsigned j = 0; j < 64; ++j)
                CHECK(got[j] == padded_byte(total, 64 * b + j, data), "total %llu block %llu byte %u",
                      (unsigned long long)total, (unsigned long long)b, j);
        }
        if (total <= 300) {  // and through the compression function against the library's one-shot SHA-256
            std::vector<uint8_t> msg(total ? total : 1);  // exactly sized (1 for the empty message)
            for (uint64_t p = 0; p < total; ++p) msg[p] = data(p);
            cdc::Sha256 S;
            S.force_scalar = true;
            for (uint64_t b = 0; b < nb; ++b) {
                uint8_t blk[64];
                shab_block(total, b, data, blk);
                S.blocks(blk, 1);
            }
            uint8_t want[32];
            cdc::sha256(msg.data(), total, want);
            for (int j = 0; j < 8; ++j)
                for (int i = 0; i < 4; ++i)
                    CHECK(uint8_t(S.h[j] >> (24 - 8 * i)) == want[4 * j + i], "digest of %llu bytes", (unsigned long long)total);
        }
        ++count;
    }
    return count;
}

static uint64_t pick_len(uint64_t src_len)
{
    switch (below(8)) {
    case 0: return 0;
    case 1: return below(8);
    case 2: return below(200);
    case 3: return 64 * below(20);
    case 4: return 63 + below(3);
    case 5: return below(src_len + 1);  // huge
    default: return below(2000);
    }
}

static uint64_t g_objects = 0;

static void check_plan_once(unsigned round)
{
    const uint64_t src_len = round % 50 == 0 ? 0 : 1 + below(round % 7 == 0 ? 200000 : 5000);
    uint8_t *src = static_cast<uint8_t *>(malloc(src_len ? src_len : 1));
    for (uint64_t i = 0; i < src_len; ++i) src[i] = uint8_t(rnd());
    const uint64_t n = below(12);
    std::vector<uint64_t> off, len, seg0(1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t ns = below(5) == 0 ? 0 : below(9);
        for (uint64_t s = 0; s < ns; ++s) {
            if (!off.empty() && below(6) == 0) {  // a repeat
                const size_t j = size_t(below(off.size()));
                off.push_back(off[j]);
                len.push_back(len[j]);
                continue;
            }
            const uint64_t l = std::min(pick_len(src_len), src_len);
            off.push_back(below(src_len - l + 1));
            len.push_back(l);
        }
        seg0.push_back(off.size());
    }
    CHECK(cplan::segments_valid(off.data(), len.data(), off.size(), seg0.data(), n, src_len), "valid lists refused");
    cplan::Runs P;
    cplan::plan_runs(off.data(), len.data(), seg0.data(), n, P);
    CHECK(P.run0.size() == n + 1 && P.total.size() == n && P.run0[n] == P.runs.size(), "shape");
    uint8_t *seam = static_cast<uint8_t *>(malloc(P.seam_bytes ? P.seam_bytes : 1));
    memset(seam, 0xA5, P.seam_bytes);
    uint64_t end = 0;
    for (const cplan::Copy &c : P.copies) {
        CHECK(c.len > 0 && c.src_off <= src_len && c.len <= src_len - c.src_off, "copy source out of bounds");
        CHECK(c.dst_off >= end && c.dst_off <= P.seam_bytes && c.len <= P.seam_bytes - c.dst_off, "copy destination");
        memcpy(seam + c.dst_off, src + c.src_off, c.len);
        end = c.dst_off + c.len;
    }
    CHECK(end == P.seam_bytes, "seam area: %llu reported, %llu used", (unsigned long long)P.seam_bytes, (unsigned long long)end);
    for (uint64_t i = 0; i < n; ++i) {
        std::vector<uint8_t> want, got;
        for (uint64_t s = seg0[i]; s < seg0[i + 1]; ++s) want.insert(want.end(), src + off[s], src + off[s] + len[s]);
        CHECK(P.run0[i] < P.run0[i + 1], "an object without a run");
        for (uint64_t r = P.run0[i]; r < P.run0[i + 1]; ++r) {
            const cplan::Run &R = P.runs[r];
            const bool in_seam = (R.src & cplan::kSeam) != 0;
            const uint64_t o = R.src & ~cplan::kSeam, cap = in_seam ? P.seam_bytes : src_len;
            CHECK(o <= cap && R.bytes <= cap - o, "run out of bounds");
            CHECK(r + 1 == P.run0[i + 1] || (R.bytes % 64 == 0 && R.bytes), "run %llu of object %llu holds %llu bytes",
                  (unsigned long long)(r - P.run0[i]), (unsigned long long)i, (unsigned long long)R.bytes);
            const uint8_t *b = (in_seam ? seam : src) + o;
            got.insert(got.end(), b, b + R.bytes);
        }
        CHECK(got == want && P.total[i] == want.size(), "object %llu: the runs do not rebuild the message", (unsigned long long)i);
        // the kernel's walk: block gb of the object from block lb of run r
        cdc::Sha256 S;
        S.force_scalar = true;
        const uint64_t nb = shab::blocks(P.total[i]);
        uint64_t r = P.run0[i], lb = 0;
        for (uint64_t gb = 0; gb < nb; ++gb) {
            const cplan::Run &R = P.runs[r];
            const uint8_t *b = ((R.src & cplan::kSeam) ? seam : src) + (R.src & ~cplan::kSeam);
            uint8_t blk[64];
            // message byte p of this block is byte 64 lb + (p - 64 gb) of the run; read only what the run holds
            auto data = [&](uint64_t p) {
                const uint64_t q = 64 * lb + (p - 64 * gb);
                CHECK(q < R.bytes, "block %llu of object %llu reads past its run", (unsigned long long)gb, (unsigned long long)i);
                return b[q];
            };
            shab_block(P.total[i], gb, data, blk);
            S.blocks(blk, 1);
            ++lb;
            if (gb + 1 < nb && 64 * lb >= R.bytes && r + 1 < P.run0[i + 1]) {
                ++r;
                lb = 0;
            }
        }
        uint8_t d[32];
        cdc::sha256(want.data(), want.size(), d);
        for (int j = 0; j < 8; ++j)
            for (int q = 0; q < 4; ++q) CHECK(uint8_t(S.h[j] >> (24 - 8 * q)) == d[4 * j + q], "object %llu: digest", (unsigned long long)i);
        ++g_objects;
    }
    // lists that must be refused
    if (!off.empty()) {
        std::vector<uint64_t> l2(len), o2(off), s2(seg0);
        const size_t j = size_t(below(off.size()));
        l2[j] = src_len - off[j] + 1 + below(3);
        CHECK(!cplan::segments_valid(off.data(), l2.data(), off.size(), seg0.data(), n, src_len), "a segment past the end");
        o2[j] = src_len + 1 + below(5);
        CHECK(!cplan::segments_valid(o2.data(), len.data(), off.size(), seg0.data(), n, src_len), "an offset past the end");
        l2 = len;
        l2[j] = ~0ull - below(3);  // offset + length wraps
        CHECK(!cplan::segments_valid(off.data(), l2.data(), off.size(), seg0.data(), n, src_len), "a length that wraps");
        s2[n] = off.size() + 1;
        CHECK(!cplan::segments_valid(off.data(), len.data(), off.size(), s2.data(), n, src_len), "a list past nsegs");
        if (n >= 2 && seg0[1] > 0) {
            s2 = seg0;
            s2[0] = seg0[1] + 1;  // descends
            CHECK(!cplan::segments_valid(off.data(), len.data(), off.size(), s2.data(), n, src_len), "a list that descends");
        }
    }
    free(seam);
    free(src);
}

static void check_split()
{
    std::vector<uint8_t> host(3, 7);
    cplan::split(nullptr, 0, 8, 0, 2e9, host);
    CHECK(host.empty(), "no objects");
    cplan::split(nullptr, 0, 8, 5, 2e9, host);
    CHECK(host.empty(), "no objects, host_min_len");
    // all equal: whatever the model says, it says it for the whole tie or a prefix of it, never out of range
    std::vector<uint64_t> eq(100, 65536);
    cplan::split(eq.data(), eq.size(), 8, 0, 2e9, host);
    CHECK(host.size() == 100, "all equal: size");
    for (size_t i = 1; i < host.size(); ++i) CHECK(host[i - 1] >= host[i], "all equal: ties go in list order");
    // one giant among small ones: the giant's chain (2 us per block) would last minutes
    std::vector<uint64_t> g(101, 65536);
    g[37] = 1ull << 32;
    cplan::split(g.data(), g.size(), 8, 0, 2e9, host);
    CHECK(host[37] == 1, "one giant stays on the device");
    size_t on_dev = 0;
    for (uint8_t h : host) on_dev += !h;
    CHECK(on_dev > 0, "one giant takes everything to the host");
    // host_min_len overrides the model
    std::vector<uint64_t> m = {0, 1, 99, 100, 101, 1ull << 40};
    cplan::split(m.data(), m.size(), 8, 100, 2e9, host);
    CHECK(host == std::vector<uint8_t>({0, 0, 0, 1, 1, 1}), "host_min_len 100");
    cplan::split(m.data(), m.size(), 8, ~0ull, 2e9, host);
    CHECK(host == std::vector<uint8_t>(6, 0), "host_min_len 2^64 - 1");
    cplan::split(m.data(), m.size(), 8, 1, 2e9, host);
    CHECK(host == std::vector<uint8_t>(6, 1), "host_min_len 1: the empty object follows the others to the host");
    // empty objects alone are no reason for a launch
    std::vector<uint64_t> z(5, 0);
    cplan::split(z.data(), z.size(), 8, 0, 2e9, host);
    CHECK(host == std::vector<uint8_t>(5, 1), "empties, the model");
    cplan::split(z.data(), z.size(), 8, ~0ull, 2e9, host);
    CHECK(host == std::vector<uint8_t>(5, 1), "empties, forced to the device");
    // a single thread and a slow host keep more on the device than many fast ones
    std::vector<uint64_t> mix;
    for (int i = 0; i < 64; ++i) mix.push_back(uint64_t(1) << (10 + i % 16));
    std::vector<uint8_t> slow, fast;
    cplan::split(mix.data(), mix.size(), 1, 0, 2e8, slow);
    cplan::split(mix.data(), mix.size(), 16, 0, 4e9, fast);
    size_t ns = 0, nf = 0;
    for (uint8_t h : slow) ns += h;
    for (uint8_t h : fast) nf += h;
    CHECK(ns <= nf, "a slower host takes more");
}

int main()
{
    const uint64_t totals = check_totals();
    const unsigned plans = 4000;
    for (unsigned r = 0; r < plans; ++r) check_plan_once(r);
    check_split();
    printf("%u plans, %llu objects, %llu totals, ok\n", plans, (unsigned long long)g_objects, (unsigned long long)totals);
    return 0;
}
