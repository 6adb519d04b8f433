// Host-only pieces of the search path (include/plakar_cdc.h, "grep"), shared by
// the library (cdc_grep.hip, cdc_grep.cpp) and the stand-alone sanitizer
// program tests/c/grep_plan_check.cpp:
//
//   * the query compiler: it validates 1..32 fixed strings of 1..256 bytes,
//     folds them under CDC_GREP_IGNORE_CASE (ASCII letters only) and lays what
//     k_grep_scan filters with into one flat block of dwords, uploaded once per
//     query: a 256-bit first-byte set, a 256-bit set of the one-byte patterns,
//     for every byte the patterns that start with it, a 64-Kbit bitmap of the
//     two-byte prefixes of the patterns of 2 bytes or more, and the packed
//     pattern bytes.  Under ignore-case the sets hold both cases of a letter
//     (the kernel filters the raw bytes) and the packed bytes are folded (the
//     kernel folds a text byte before it compares);
//   * a scalar matcher over one text with exactly the device's semantics, for
//     the CPU tests and nothing else;
//   * the emit records of the matched-line text (cdc_diff_emit_device runs them).
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "plakar_cdc.h"

namespace gplan {

constexpr uint32_t kMaxPatterns = 32, kMaxPatternLen = 256;
// The block, in dwords.
constexpr uint32_t kNPat = 0, kFlags = 1, kPatBytes = 2, kBlockBytes = 3;
constexpr uint32_t kFirst = 4;               // 8: bit b set, some pattern starts with byte b
constexpr uint32_t kOne = 12;                // 8: bit b set, a one-byte pattern is byte b
constexpr uint32_t kLen = 20;                // 32: the patterns' lengths
constexpr uint32_t kOff = 52;                // 32: their places in the packed bytes
constexpr uint32_t kStart = 84;              // 256: bit k of entry b set, pattern k starts with byte b
constexpr uint32_t kPrefix = kStart + 256;   // 2048: bit (b0 | b1 << 8) set, a pattern of 2 bytes or more starts b0 b1
constexpr uint32_t kBytes = kPrefix + 2048;  // the packed pattern bytes (folded under ignore-case)
constexpr uint32_t kMaxBlockBytes = 4 * kBytes + kMaxPatterns * kMaxPatternLen;

inline uint8_t fold(uint8_t b) { return uint8_t(b - 'A') < 26 ? uint8_t(b | 0x20) : b; }
inline bool is_letter(uint8_t b) { return uint8_t((b | 0x20) - 'a') < 26; }

struct Query {
    std::vector<uint32_t> block;  // block[kBlockBytes] bytes of it are uploaded
    uint32_t npatterns() const { return block[kNPat]; }
    bool ignore_case() const { return (block[kFlags] & CDC_GREP_IGNORE_CASE) != 0; }
    uint32_t len(uint32_t k) const { return block[kLen + k]; }
    const uint8_t *bytes(uint32_t k) const { return reinterpret_cast<const uint8_t *>(&block[kBytes]) + block[kOff + k]; }
};

// The arguments alone: CDC_OK or CDC_E_INVALID.
inline int validate(const uint8_t *const *patterns, const uint32_t *pattern_len, uint32_t npatterns, uint32_t flags)
{
    if (npatterns < 1 || npatterns > kMaxPatterns || !patterns || !pattern_len || (flags & ~uint32_t(CDC_GREP_IGNORE_CASE)))
        return CDC_E_INVALID;
    for (uint32_t k = 0; k < npatterns; ++k) {
        if (pattern_len[k] < 1 || pattern_len[k] > kMaxPatternLen || !patterns[k]) return CDC_E_INVALID;
        if (memchr(patterns[k], '\n', pattern_len[k])) return CDC_E_INVALID;
    }
    return CDC_OK;
}

inline void set_bit(uint32_t *w, uint32_t i) { w[i >> 5] |= 1u << (i & 31); }
inline bool get_bit(const uint32_t *w, uint32_t i) { return (w[i >> 5] >> (i & 31)) & 1u; }

inline int compile(const uint8_t *const *patterns, const uint32_t *pattern_len, uint32_t npatterns, uint32_t flags, Query &Q)
{
    const int s = validate(patterns, pattern_len, npatterns, flags);
    if (s != CDC_OK) return s;
    const bool ic = (flags & CDC_GREP_IGNORE_CASE) != 0;
    uint32_t total = 0;
    for (uint32_t k = 0; k < npatterns; ++k) total += pattern_len[k];
    const uint32_t padded = (total + 3u) & ~3u;
    Q.block.assign(kBytes + padded / 4, 0);
    uint32_t *B = Q.block.data();
    B[kNPat] = npatterns;
    B[kFlags] = flags;
    B[kPatBytes] = padded;
    B[kBlockBytes] = 4 * kBytes + padded;
    uint8_t *packed = reinterpret_cast<uint8_t *>(B + kBytes);
    uint32_t at = 0;
    for (uint32_t k = 0; k < npatterns; ++k) {
        const uint32_t m = pattern_len[k];
        B[kLen + k] = m;
        B[kOff + k] = at;
        for (uint32_t j = 0; j < m; ++j) packed[at + j] = ic ? fold(patterns[k][j]) : patterns[k][j];
        // both cases of a letter under ignore-case: the filter sees raw text bytes
        uint8_t c0[2] = {packed[at], packed[at]}, c1[2] = {0, 0};
        uint32_t n0 = 1, n1 = 1;
        if (ic && is_letter(c0[0])) c0[1] = uint8_t(c0[0] ^ 0x20), n0 = 2;
        if (m >= 2) {
            c1[0] = c1[1] = packed[at + 1];
            if (ic && is_letter(c1[0])) c1[1] = uint8_t(c1[0] ^ 0x20), n1 = 2;
        }
        for (uint32_t i = 0; i < n0; ++i) {
            set_bit(B + kFirst, c0[i]);
            B[kStart + c0[i]] |= 1u << k;
            if (m == 1) set_bit(B + kOne, c0[i]);
            for (uint32_t j = 0; m >= 2 && j < n1; ++j) set_bit(B + kPrefix, uint32_t(c0[i]) | uint32_t(c1[j]) << 8);
        }
        at += m;
    }
    return CDC_OK;
}

// The lines of a text by grep's count: its newlines, and one more when it is
// not empty and does not end in one.
inline uint64_t grep_lines(const uint8_t *p, uint64_t n)
{
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; ++i) k += p[i] == '\n';
    return k + (n && p[n - 1] != '\n');
}

// The matching lines of the text [p, p + n), which lies at `base` of its buffer,
// in line order, all of them (no limit).  *binary (may be NULL): a 0x00 in it.
inline void match_text(const Query &Q, const uint8_t *p, uint64_t n, uint64_t base, uint32_t text, std::vector<cdc_grep_hit> &hits,
                       int *binary)
{
    const bool ic = Q.ignore_case();
    if (binary) *binary = n && memchr(p, 0, n) != nullptr;
    uint64_t lo = 0;
    uint32_t line = 1;
    while (lo < n) {
        const uint8_t *e = static_cast<const uint8_t *>(memchr(p + lo, '\n', n - lo));
        const uint64_t hi = e ? uint64_t(e - p) : n, len = hi - lo;
        cdc_grep_hit H{text, line, base + lo, uint32_t(len), 0xFFFFFFFFu, 0, 0};
        uint64_t nocc = 0;
        for (uint32_t k = 0; k < Q.npatterns(); ++k) {
            const uint32_t m = Q.len(k);
            const uint8_t *pat = Q.bytes(k);
            for (uint64_t i = 0; i + m <= len; ++i) {
                uint32_t j = 0;
                while (j < m && (ic ? fold(p[lo + i + j]) : p[lo + i + j]) == pat[j]) ++j;
                if (j < m) continue;
                H.mask |= 1u << k;
                H.col = std::min<uint32_t>(H.col, uint32_t(i));
                ++nocc;
            }
        }
        if (H.mask) {
            H.nocc = uint32_t(std::min<uint64_t>(nocc, 0xFFFFFFFFull));
            hits.push_back(H);
        }
        lo = hi + 1;
        ++line;
    }
}

// The matched-line text: per hit, the line's first min(len, max_line_bytes)
// bytes and a newline, in hit order from dst_base on.  hits[i].off is the
// line's place in the plaintext buffer.  Returns the bytes of the text.
inline uint64_t emit_records(const cdc_grep_hit *hits, uint64_t n, uint32_t max_line_bytes, uint64_t dst_base,
                             std::vector<cdc_emit_rec> &recs)
{
    uint64_t at = dst_base;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t len = std::min(hits[i].len, max_line_bytes);
        recs.push_back(cdc_emit_rec{hits[i].off, at, len, CDC_EMIT_NEWLINE});
        at += uint64_t(len) + 1;
    }
    return at - dst_base;
}

}  // namespace gplan
