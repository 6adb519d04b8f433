// Stand-alone check of plakar_amd/csrc/grep_plan.h, built with
// -fsanitize=address,undefined by tests/test_grep_cpu.py:
//   * the compiled query's first-byte set, one-byte set, start masks and
//     two-byte prefix bitmap, every bit against a brute force over the
//     patterns, with and without CDC_GREP_IGNORE_CASE;
//   * what the compiler refuses;
//   * the scalar matcher against a naive one that works position by position
//     over the whole text, on 10,000 seeded cases;
//   * the emit records of the matched-line text.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <vector>

#include "grep_plan.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 16);
}

static uint8_t lower(uint8_t b) { return b >= 'A' && b <= 'Z' ? uint8_t(b + 32) : b; }
static bool same(uint8_t text, uint8_t pat, bool ic) { return ic ? lower(text) == lower(pat) : text == pat; }

struct Pats {
    std::vector<std::string> s;
    std::vector<const uint8_t *> p;
    std::vector<uint32_t> n;
    void done()
    {
        p.clear(), n.clear();
        for (auto &x : s) p.push_back(reinterpret_cast<const uint8_t *>(x.data())), n.push_back(uint32_t(x.size()));
    }
};

static uint64_t check_sets(const Pats &P, uint32_t flags)
{
    const bool ic = flags & CDC_GREP_IGNORE_CASE;
    gplan::Query Q;
    CHECK(gplan::compile(P.p.data(), P.n.data(), uint32_t(P.p.size()), flags, Q) == CDC_OK);
    const uint32_t *B = Q.block.data();
    CHECK(B[gplan::kNPat] == P.p.size() && B[gplan::kFlags] == flags && B[gplan::kBlockBytes] == 4 * Q.block.size());
    CHECK(B[gplan::kBlockBytes] <= gplan::kMaxBlockBytes && B[gplan::kBlockBytes] % 4 == 0);
    uint64_t bits = 0;
    for (uint32_t b0 = 0; b0 < 256; ++b0) {
        bool first = false, one = false;
        uint32_t start = 0;
        for (size_t k = 0; k < P.s.size(); ++k)
            if (same(uint8_t(b0), uint8_t(P.s[k][0]), ic)) {
                first = true;
                start |= 1u << k;
                one |= P.s[k].size() == 1;
            }
        CHECK(gplan::get_bit(B + gplan::kFirst, b0) == first);
        CHECK(gplan::get_bit(B + gplan::kOne, b0) == one);
        CHECK(B[gplan::kStart + b0] == start);
        bits += 3;
        for (uint32_t b1 = 0; b1 < 256; ++b1) {
            bool pre = false;
            for (size_t k = 0; k < P.s.size(); ++k)
                pre |= P.s[k].size() >= 2 && same(uint8_t(b0), uint8_t(P.s[k][0]), ic) && same(uint8_t(b1), uint8_t(P.s[k][1]), ic);
            CHECK(gplan::get_bit(B + gplan::kPrefix, b0 | b1 << 8) == pre);
            ++bits;
        }
    }
    for (size_t k = 0; k < P.s.size(); ++k) {
        CHECK(Q.len(uint32_t(k)) == P.s[k].size());
        for (size_t j = 0; j < P.s[k].size(); ++j)
            CHECK(Q.bytes(uint32_t(k))[j] == (ic ? lower(uint8_t(P.s[k][j])) : uint8_t(P.s[k][j])));
    }
    return bits;
}

struct Line {
    uint64_t off = 0;
    uint32_t mask = 0, col = 0xFFFFFFFFu;
    uint64_t nocc = 0;
};

// position by position over the whole text: an occurrence cannot hold a newline, so it lies in the line of its first byte
static std::vector<cdc_grep_hit> naive(const Pats &P, bool ic, const std::string &T, uint64_t base, uint32_t text)
{
    std::map<uint32_t, Line> lines;
    uint32_t line = 1;
    uint64_t start = 0;
    for (uint64_t i = 0; i < T.size(); ++i) {
        for (size_t k = 0; k < P.s.size(); ++k) {
            const std::string &p = P.s[k];
            if (i + p.size() > T.size()) continue;
            bool eq = true;
            for (size_t j = 0; j < p.size() && eq; ++j) eq = same(uint8_t(T[i + j]), uint8_t(p[j]), ic);
            if (!eq) continue;
            Line &L = lines[line];
            L.off = start;
            L.mask |= 1u << k;
            L.col = std::min<uint32_t>(L.col, uint32_t(i - start));
            ++L.nocc;
        }
        if (T[i] == '\n') ++line, start = i + 1;
    }
    std::vector<cdc_grep_hit> out;
    for (auto &kv : lines) {
        uint64_t e = kv.second.off;
        while (e < T.size() && T[e] != '\n') ++e;
        out.push_back(cdc_grep_hit{text, kv.first, base + kv.second.off, uint32_t(e - kv.second.off), kv.second.col, kv.second.mask,
                                   uint32_t(kv.second.nocc)});
    }
    return out;
}

int main()
{
    // ---- the sets
    uint64_t bits = 0;
    const char *sets[][6] = {{"a", nullptr}, {"Ab", "aB", "Z", nullptr}, {"@[", "`{", "\xc9x", "\xe9", nullptr},
                             {"hello", "HeLLo", "h", "zz", "Zq", nullptr}, {"m\xffn", "M", "9z", "9Z", nullptr}};
    for (auto &set : sets) {
        Pats P;
        for (int k = 0; set[k]; ++k) P.s.push_back(set[k]);
        P.s.push_back(std::string("\0q", 2));  // 0x00 is ordinary
        P.done();
        bits += check_sets(P, 0) + check_sets(P, CDC_GREP_IGNORE_CASE);
    }
    {   // 32 patterns of 256 bytes: the largest block
        Pats P;
        for (int k = 0; k < 32; ++k) P.s.push_back(std::string(256, char('A' + k % 26)));
        P.done();
        bits += check_sets(P, 0) + check_sets(P, CDC_GREP_IGNORE_CASE);
        gplan::Query Q;
        CHECK(gplan::compile(P.p.data(), P.n.data(), 32, 0, Q) == CDC_OK && Q.block[gplan::kBlockBytes] == gplan::kMaxBlockBytes);
    }
    // ---- what is refused
    int refused = 0;
    {
        Pats P;
        P.s = {"ab", "c"};
        P.done();
        gplan::Query Q;
        CHECK(gplan::compile(P.p.data(), P.n.data(), 2, 0, Q) == CDC_OK);
        CHECK(gplan::compile(P.p.data(), P.n.data(), 0, 0, Q) == CDC_E_INVALID); ++refused;
        CHECK(gplan::compile(nullptr, P.n.data(), 2, 0, Q) == CDC_E_INVALID); ++refused;
        CHECK(gplan::compile(P.p.data(), nullptr, 2, 0, Q) == CDC_E_INVALID); ++refused;
        CHECK(gplan::compile(P.p.data(), P.n.data(), 2, 2, Q) == CDC_E_INVALID); ++refused;
        uint32_t n0[2] = {0, 1}, n257[2] = {2, 257};
        std::string big(257, 'x');
        const uint8_t *pb[2] = {P.p[0], reinterpret_cast<const uint8_t *>(big.data())};
        CHECK(gplan::compile(P.p.data(), n0, 2, 0, Q) == CDC_E_INVALID); ++refused;
        CHECK(gplan::compile(pb, n257, 2, 0, Q) == CDC_E_INVALID); ++refused;
        n257[1] = 256;
        CHECK(gplan::compile(pb, n257, 2, 0, Q) == CDC_OK);
        Pats N;
        N.s = {"ab", "c\nd"};
        N.done();
        CHECK(gplan::compile(N.p.data(), N.n.data(), 2, 0, Q) == CDC_E_INVALID); ++refused;
        N.s = {"ab", std::string("c\0d", 3)};
        N.done();
        CHECK(gplan::compile(N.p.data(), N.n.data(), 2, 0, Q) == CDC_OK);
        Pats M;
        for (int k = 0; k < 33; ++k) M.s.push_back("p");
        M.done();
        CHECK(gplan::compile(M.p.data(), M.n.data(), 33, 0, Q) == CDC_E_INVALID); ++refused;
        CHECK(gplan::compile(M.p.data(), M.n.data(), 32, 0, Q) == CDC_OK);
    }
    // ---- the matcher
    const char alphabet[] = {'a', 'b', 'A', 'B', ' ', '\r', '\n', '\n', '\xc9', '\xe9', '\0', '@', '`'};
    uint64_t cases = 0, hits_seen = 0;
    for (int c = 0; c < 10000; ++c) {
        std::string T(rnd() % 120, 'a');
        for (auto &ch : T) ch = alphabet[rnd() % sizeof(alphabet)];
        Pats P;
        const uint32_t np = 1 + rnd() % (c % 50 == 0 ? 32 : 4);
        for (uint32_t k = 0; k < np; ++k) {
            std::string p;
            const uint32_t m = 1 + rnd() % 4;
            if (!T.empty() && rnd() % 3) {
                const size_t at = rnd() % T.size();
                p = T.substr(at, m);
            }
            for (auto &ch : p)
                if (ch == '\n') ch = 'b';
            while (p.size() < 1) p.push_back(alphabet[rnd() % 6]);
            if (rnd() % 4 == 0) p[0] = char(p[0] ^ 0x20);
            if (p.find('\n') != std::string::npos) p = "ab";
            P.s.push_back(p);
        }
        P.done();
        const bool ic = rnd() & 1;
        gplan::Query Q;
        CHECK(gplan::compile(P.p.data(), P.n.data(), np, ic ? CDC_GREP_IGNORE_CASE : 0, Q) == CDC_OK);
        const uint64_t base = uint64_t(rnd()) << 12;
        std::vector<cdc_grep_hit> got;
        int binary = -1;
        gplan::match_text(Q, reinterpret_cast<const uint8_t *>(T.data()), T.size(), base, uint32_t(c), got, &binary);
        const std::vector<cdc_grep_hit> want = naive(P, ic, T, base, uint32_t(c));
        CHECK(got.size() == want.size());
        for (size_t i = 0; i < got.size(); ++i) CHECK(memcmp(&got[i], &want[i], sizeof(cdc_grep_hit)) == 0);
        CHECK(binary == (T.find('\0') != std::string::npos));
        uint64_t nl = 0;
        for (char ch : T) nl += ch == '\n';
        CHECK(gplan::grep_lines(reinterpret_cast<const uint8_t *>(T.data()), T.size()) == nl + (!T.empty() && T.back() != '\n'));
        hits_seen += got.size();
        ++cases;
    }
    CHECK(hits_seen > 5000);
    // ---- the emit records
    int emits = 0;
    {
        static_assert(sizeof(cdc_grep_hit) == 32, "");
        const cdc_grep_hit H[3] = {{0, 1, 100, 5, 0, 1, 1}, {0, 7, 200, 0, 0, 1, 1}, {1, 2, 4096, 40, 3, 1, 2}};
        std::vector<cdc_emit_rec> R;
        CHECK(gplan::emit_records(H, 3, 16, 1000, R) == 6 + 1 + 17 && R.size() == 3); ++emits;
        CHECK(R[0].src_off == 100 && R[0].dst_off == 1000 && R[0].len == 5 && R[0].flags == CDC_EMIT_NEWLINE); ++emits;
        CHECK(R[1].src_off == 200 && R[1].dst_off == 1006 && R[1].len == 0 && R[1].flags == CDC_EMIT_NEWLINE); ++emits;
        CHECK(R[2].src_off == 4096 && R[2].dst_off == 1007 && R[2].len == 16 && R[2].flags == CDC_EMIT_NEWLINE); ++emits;
        R.clear();
        CHECK(gplan::emit_records(H, 0, 16, 0, R) == 0 && R.empty()); ++emits;
        CHECK(gplan::emit_records(H, 3, 1, 0, R) == 2 + 1 + 2 && R[2].dst_off == 3 && R[2].len == 1); ++emits;
    }
    printf("%llu bits, %d refusals, %llu matcher cases, %d emit checks, ok\n", (unsigned long long)bits, refused,
           (unsigned long long)cases, emits);
    return 0;
}
