// Host-only pieces of the diff path, shared by the library (cdc_diff.cpp) and
// the stand-alone sanitizer program tests/c/diff_plan_check.cpp:
//
//   * the matcher of `plakar diff` (cmd/plakar/subcommands/diff/diff.go:152-196
//     calls go-difflib's UnifiedDiff, a port of Python's difflib): difflib's
//     SequenceMatcher over 32-bit line ids, with no junk function and autojunk
//     on, its matching blocks, opcodes and grouped opcodes;
//   * the unified-diff text as an emit plan: records that name where every
//     output line comes from (a line of the plaintext image, or a literal the
//     host wrote: the header and the @@ lines), executed by
//     cdc_diff_emit_device;
//   * exact line ids from hashes: leaders proposed from a hash map, and the
//     re-leading of the lines a byte comparison flagged.
//
// No HIP, no library state: everything is a function of its arguments.  The
// matcher's worst case is quadratic, as the reference's is; there is no
// cut-off.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "plakar_cdc.h"

namespace dplan {

enum : uint32_t { kEqual = CDC_DIFF_EQUAL, kReplace = CDC_DIFF_REPLACE, kDelete = CDC_DIFF_DELETE, kInsert = CDC_DIFF_INSERT };

struct Match {
    uint32_t a, b, size;
};

// difflib.SequenceMatcher(None, a, b) with autojunk=True.
class Matcher {
public:
    Matcher(const uint32_t *a, size_t na, const uint32_t *b, size_t nb) : a_(a), b_(b), na_(na), nb_(nb) { chain_b(); }

    // get_matching_blocks(): the blocks in order, adjacent ones collapsed, the
    // (na, nb, 0) sentinel last.
    std::vector<Match> matching_blocks()
    {
        struct Q {
            size_t alo, ahi, blo, bhi;
        };
        std::vector<Q> queue{Q{0, na_, 0, nb_}};
        std::vector<Match> found;
        prev_.assign(nb_ + 1, 0);
        cur_.assign(nb_ + 1, 0);
        while (!queue.empty()) {
            const Q q = queue.back();
            queue.pop_back();
            const Match m = find_longest_match(q.alo, q.ahi, q.blo, q.bhi);
            if (!m.size) continue;
            found.push_back(m);
            if (q.alo < m.a && q.blo < m.b) queue.push_back(Q{q.alo, m.a, q.blo, m.b});
            if (m.a + m.size < q.ahi && m.b + m.size < q.bhi) queue.push_back(Q{size_t(m.a) + m.size, q.ahi, size_t(m.b) + m.size, q.bhi});
        }
        std::sort(found.begin(), found.end(), [](const Match &x, const Match &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
        std::vector<Match> out;
        uint32_t i1 = 0, j1 = 0, k1 = 0;
        for (const Match &m : found) {
            if (i1 + k1 == m.a && j1 + k1 == m.b) {
                k1 += m.size;
            } else {
                if (k1) out.push_back(Match{i1, j1, k1});
                i1 = m.a, j1 = m.b, k1 = m.size;
            }
        }
        if (k1) out.push_back(Match{i1, j1, k1});
        out.push_back(Match{uint32_t(na_), uint32_t(nb_), 0});
        return out;
    }

    // find_longest_match: the longest block in a[alo:ahi] and b[blo:bhi] over
    // the elements b2j kept, the earliest in a and then in b among equals,
    // extended over the popular elements on both sides.  There is no junk, so
    // the second pair of extension loops (over junk elements) never runs.
    Match find_longest_match(size_t alo, size_t ahi, size_t blo, size_t bhi)
    {
        size_t besti = alo, bestj = blo, bestsize = 0;
        touched_prev_.clear();
        for (size_t i = alo; i < ahi; ++i) {
            touched_cur_.clear();
            const auto it = slot_.find(a_[i]);
            if (it != slot_.end()) {
                const uint32_t s = it->second;
                for (uint32_t p = start_[s]; p < start_[s + 1]; ++p) {
                    const size_t j = pos_[p];
                    if (j < blo) continue;
                    if (j >= bhi) break;
                    const uint32_t k = prev_[j] + 1;  // prev_[j] is j2len[j - 1]
                    cur_[j + 1] = k;
                    touched_cur_.push_back(uint32_t(j + 1));
                    if (k > bestsize) besti = i + 1 - k, bestj = j + 1 - k, bestsize = k;
                }
            }
            for (uint32_t t : touched_prev_) prev_[t] = 0;
            prev_.swap(cur_);
            touched_prev_.swap(touched_cur_);
        }
        for (uint32_t t : touched_prev_) prev_[t] = 0;
        touched_prev_.clear();
        while (besti > alo && bestj > blo && a_[besti - 1] == b_[bestj - 1]) --besti, --bestj, ++bestsize;
        while (besti + bestsize < ahi && bestj + bestsize < bhi && a_[besti + bestsize] == b_[bestj + bestsize]) ++bestsize;
        return Match{uint32_t(besti), uint32_t(bestj), uint32_t(bestsize)};
    }

private:
    // b2j: for every element of b the ascending list of its places; with 200
    // elements or more, those that occur more than len(b) // 100 + 1 times
    // (the popular ones) are left out.
    void chain_b()
    {
        slot_.reserve(nb_ * 2);
        std::vector<uint32_t> cnt;
        std::vector<uint32_t> which(nb_);
        for (size_t j = 0; j < nb_; ++j) {
            const auto r = slot_.emplace(b_[j], uint32_t(cnt.size()));
            if (r.second) cnt.push_back(0);
            which[j] = r.first->second;
            ++cnt[which[j]];
        }
        if (nb_ >= 200) {
            const size_t ntest = nb_ / 100 + 1;
            for (uint32_t &c : cnt)
                if (c > ntest) c = 0;  // popular: an empty list
        }
        start_.assign(cnt.size() + 1, 0);
        for (size_t s = 0; s < cnt.size(); ++s) start_[s + 1] = start_[s] + cnt[s];
        pos_.resize(start_.back());
        std::vector<uint32_t> fill(start_.begin(), start_.end() - 1);
        for (size_t j = 0; j < nb_; ++j)
            if (cnt[which[j]]) pos_[fill[which[j]]++] = uint32_t(j);
    }

    const uint32_t *a_, *b_;
    size_t na_, nb_;
    std::unordered_map<uint32_t, uint32_t> slot_;
    std::vector<uint32_t> start_, pos_;
    std::vector<uint32_t> prev_, cur_, touched_prev_, touched_cur_;
};

// get_opcodes()
static inline std::vector<cdc_diff_op> opcodes(const std::vector<Match> &blocks)
{
    std::vector<cdc_diff_op> out;
    uint32_t i = 0, j = 0;
    for (const Match &m : blocks) {
        uint32_t tag = kEqual;
        if (i < m.a && j < m.b)
            tag = kReplace;
        else if (i < m.a)
            tag = kDelete;
        else if (j < m.b)
            tag = kInsert;
        if (tag != kEqual) out.push_back(cdc_diff_op{tag, 0, i, m.a, j, m.b});
        i = m.a + m.size, j = m.b + m.size;
        if (m.size) out.push_back(cdc_diff_op{kEqual, 0, m.a, i, m.b, j});
    }
    return out;
}

// get_grouped_opcodes(n): the groups back to back, `group` numbering them.
static inline std::vector<cdc_diff_op> grouped_opcodes(std::vector<cdc_diff_op> codes, uint32_t n)
{
    std::vector<cdc_diff_op> out;
    if (codes.empty()) codes.push_back(cdc_diff_op{kEqual, 0, 0, 1, 0, 1});
    auto lo = [n](uint32_t x, uint32_t y) { return std::max<uint64_t>(x, y > n ? y - n : 0); };  // max(x, y - n)
    auto hi = [n](uint32_t x, uint32_t y) { return uint32_t(std::min<uint64_t>(x, uint64_t(y) + n)); };  // min(x, y + n)
    if (codes.front().tag == kEqual) {
        cdc_diff_op &c = codes.front();
        c.i1 = uint32_t(lo(c.i1, c.i2)), c.j1 = uint32_t(lo(c.j1, c.j2));
    }
    if (codes.back().tag == kEqual) {
        cdc_diff_op &c = codes.back();
        c.i2 = hi(c.i2, c.i1), c.j2 = hi(c.j2, c.j1);
    }
    const uint64_t nn = uint64_t(n) + n;
    std::vector<cdc_diff_op> group;
    uint32_t gid = 0;
    auto flush = [&](bool always) {
        if (always || (!group.empty() && !(group.size() == 1 && group[0].tag == kEqual))) {
            for (cdc_diff_op &g : group) {
                g.group = gid;
                out.push_back(g);
            }
            ++gid;
        }
        group.clear();
    };
    for (const cdc_diff_op &c0 : codes) {
        cdc_diff_op c = c0;
        if (c.tag == kEqual && uint64_t(c.i2) - c.i1 > nn) {
            group.push_back(cdc_diff_op{kEqual, 0, c.i1, hi(c.i2, c.i1), c.j1, hi(c.j2, c.j1)});
            flush(true);  // difflib yields here without looking at the group
            c.i1 = uint32_t(lo(c.i1, c.i2)), c.j1 = uint32_t(lo(c.j1, c.j2));
        }
        group.push_back(c);
    }
    flush(false);
    return out;
}

// The whole script of one pair.
static inline std::vector<cdc_diff_op> script(const uint32_t *a, size_t na, const uint32_t *b, size_t nb, uint32_t context)
{
    Matcher m(a, na, b, nb);
    return grouped_opcodes(opcodes(m.matching_blocks()), context);
}

// ---- the emit plan ----------------------------------------------------------------
struct Plan {
    std::vector<cdc_emit_rec> recs;
    std::string lit;       // the literal area: "--- from\n+++ to\n" and the @@ lines
    uint64_t out_bytes = 0;
    uint64_t hunks = 0;
};

// difflib._format_range_unified
static inline std::string format_range(uint32_t start, uint32_t stop)
{
    const uint32_t length = stop - start;
    char buf[40];
    if (length == 1)
        snprintf(buf, sizeof(buf), "%u", start + 1);
    else if (length == 0)
        snprintf(buf, sizeof(buf), "%u,0", start);
    else
        snprintf(buf, sizeof(buf), "%u,%u", start + 1, length);
    return buf;
}

// unified_diff(..., lineterm="\n") without dates over the grouped opcodes: the
// records in output order, dst_off ascending from dst_base, literals placed
// from lit_base in the literal area.  a_lines / b_lines give every line's
// place in the plaintext source.
static inline void emit_plan(const cdc_diff_op *ops, size_t nops, const cdc_line_rec *a_lines, const cdc_line_rec *b_lines,
                             const char *from_name, const char *to_name, uint64_t dst_base, uint64_t lit_base, Plan &P)
{
    P.recs.clear();
    P.lit.clear();
    P.hunks = 0;
    uint64_t dst = dst_base;
    auto literal = [&](const std::string &s) {
        P.recs.push_back(cdc_emit_rec{lit_base + P.lit.size(), dst, uint32_t(s.size()), CDC_EMIT_LITERAL});
        P.lit += s;
        dst += s.size();
    };
    auto line = [&](const cdc_line_rec &L, char prefix) {
        P.recs.push_back(cdc_emit_rec{L.off, dst, L.len, CDC_EMIT_PREFIX | CDC_EMIT_NEWLINE | uint32_t(uint8_t(prefix))});
        dst += uint64_t(L.len) + 2;
    };
    for (size_t g0 = 0; g0 < nops;) {
        size_t g1 = g0;
        while (g1 < nops && ops[g1].group == ops[g0].group) ++g1;
        if (!P.hunks) literal(std::string("--- ") + (from_name ? from_name : "") + "\n+++ " + (to_name ? to_name : "") + "\n");
        ++P.hunks;
        const cdc_diff_op &first = ops[g0], &last = ops[g1 - 1];
        literal("@@ -" + format_range(first.i1, last.i2) + " +" + format_range(first.j1, last.j2) + " @@\n");
        for (size_t k = g0; k < g1; ++k) {
            const cdc_diff_op &c = ops[k];
            if (c.tag == kEqual) {
                for (uint32_t i = c.i1; i < c.i2; ++i) line(a_lines[i], ' ');
                continue;
            }
            if (c.tag == kReplace || c.tag == kDelete)
                for (uint32_t i = c.i1; i < c.i2; ++i) line(a_lines[i], '-');
            if (c.tag == kReplace || c.tag == kInsert)
                for (uint32_t j = c.j1; j < c.j2; ++j) line(b_lines[j], '+');
        }
        g0 = g1;
    }
    P.out_bytes = dst - dst_base;
}

// What a record writes at dst_off: the prefix byte, len bytes, the newline.
static inline uint64_t rec_out_bytes(const cdc_emit_rec &r)
{
    return uint64_t(r.len) + ((r.flags & CDC_EMIT_PREFIX) ? 1 : 0) + ((r.flags & CDC_EMIT_NEWLINE) ? 1 : 0);
}

// ---- exact line ids ---------------------------------------------------------------
// id[i] = the smallest j <= i whose line has the same bytes, over one pair's
// lines (A's, then B's).  The hashes only propose: every line whose candidate
// is not itself is compared byte for byte on the device, and a line the
// comparison flags moves to the next leader of its hash's chain, or becomes a
// leader at its end.  Lines are visited in index order in every round and all
// walk a chain at one step per round, so a line meets the first line with its
// bytes in the round that line becomes a leader.
struct Key {
    uint64_t h[2];
    bool operator==(const Key &o) const { return h[0] == o.h[0] && h[1] == o.h[1]; }
};
struct KeyHash {
    size_t operator()(const Key &k) const { return size_t(k.h[0] ^ (k.h[1] * 0x9E3779B97F4A7C15ull)); }
};
// The first hash_bits bits of the 128 (0 or 128 and more: all of them).
static inline Key mask_key(const uint64_t h[2], int hash_bits)
{
    Key k{{h[0], h[1]}};
    if (hash_bits <= 0 || hash_bits >= 128) return k;
    if (hash_bits <= 64) {
        k.h[1] = 0;
        if (hash_bits < 64) k.h[0] &= (1ull << hash_bits) - 1;
    } else {
        k.h[1] &= (1ull << (hash_bits - 64)) - 1;
    }
    return k;
}

class Ids {
public:
    static constexpr uint32_t kNone = 0xFFFFFFFFu;
    // lines: the pair's records (A's then B's); cand[i] = the first line with i's key.
    void propose(const cdc_line_rec *lines, size_t n, int hash_bits)
    {
        cand.assign(n, 0);
        next_.assign(n, kNone);
        head_.clear();
        head_.reserve(n * 2);
        for (size_t i = 0; i < n; ++i) cand[i] = head_.emplace(mask_key(lines[i].hash, hash_bits), uint32_t(i)).first->second;
    }
    // Line i's comparison with cand[i] failed: its next candidate, itself at the chain's end.
    void relead(size_t i)
    {
        const uint32_t nx = next_[cand[i]];
        if (nx != kNone) {
            cand[i] = nx;
            return;
        }
        next_[cand[i]] = uint32_t(i);  // cand[i] was the chain's tail
        cand[i] = uint32_t(i);
    }
    std::vector<uint32_t> cand;  // after the last round: the ids

private:
    std::vector<uint32_t> next_;                        // a leader's successor in its key's chain
    std::unordered_map<Key, uint32_t, KeyHash> head_;   // key -> the first line with it
};

}  // namespace dplan
