// Stand-alone checker of the diff path's host-only code (diff_plan.h), built by
// tests/test_diff_cpu.py with -fsanitize=address,undefined.
//
//   * the matcher: for every case (empty sides, equal sequences, single
//     changes at the start, middle and end, two changes 2n and 2n + 1 apart
//     for n in 0, 1, 3, a popular id at len(b) 199, 200 and 201, every third
//     line "}", 200 seeded random pairs of 0-400 ids from alphabets of 2-50)
//     and n in 0, 1, 3 the grouped opcodes must be a script: ops of a group
//     back to back, equal ops over equal ids, no two changes adjacent inside
//     a group, the stretches between groups equal in a and b, every group
//     with a change and at most n lines of context at its ends;
//   * the emit planner: the records of each script laid into heap buffers of
//     exactly the reported sizes (any access past an end is a sanitizer
//     report), executed with memcpy and compared with a rendering of the same
//     opcodes written here with snprintf; destinations ascending and disjoint;
//   * exact ids: lines with hashes cut to 0-6 bits, the flagged lines found
//     with memcmp as k_line_verify does, against the first-occurrence ids of
//     a map over the bytes.
//
// Prints "<c> cases, <o> ops, <r> records, <v> rounds, ok" and exits 0, or
// says what failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "diff_plan.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                           \
    do {                                                           \
        if (!(cond)) {                                             \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                          \
            fprintf(stderr, "\n");                                 \
            exit(1);                                               \
        }                                                          \
    } while (0)

typedef std::vector<uint32_t> Seq;
struct Case {
    std::string name;
    Seq a, b;
};

static Seq range(uint32_t lo, uint32_t n)
{
    Seq s(n);
    for (uint32_t i = 0; i < n; ++i) s[i] = lo + i;
    return s;
}

static std::vector<Case> cases()
{
    std::vector<Case> c;
    c.push_back({"both empty", {}, {}});
    c.push_back({"a empty", {}, {1, 2, 3}});
    c.push_back({"b empty", {1, 2, 3}, {}});
    c.push_back({"equal", range(0, 40), range(0, 40)});
    c.push_back({"one each, equal", {7}, {7}});
    c.push_back({"one each, different", {7}, {8}});
    const Seq base = range(100, 40);
    for (uint32_t at : {0u, 20u, 39u}) {
        Seq r = base, ins = base, del = base;
        r[at] = 999;
        ins.insert(ins.begin() + at + (at == 39), 999);
        del.erase(del.begin() + at);
        c.push_back({"replace", base, r});
        c.push_back({"insert", base, ins});
        c.push_back({"delete", base, del});
    }
    const Seq lng = range(1000, 100);
    for (uint32_t n : {0u, 1u, 3u})
        for (uint32_t gap : {2 * n, 2 * n + 1}) {
            Seq r = lng;
            r[30] = 5;
            r[30 + gap + 1] = 6;
            c.push_back({"two changes", lng, r});
        }
    for (uint32_t nb : {199u, 200u, 201u}) {
        Seq b = range(10, nb);
        for (uint32_t at : {5u, 60u, 120u, 180u}) b[at] = 1;
        Seq a = {1, 11, 12, 1, 13};
        a.insert(a.end(), b.begin() + 40, b.begin() + 90);
        a.push_back(1), a.push_back(1);
        a.insert(a.end(), b.begin() + 130, b.begin() + 170);
        c.push_back({"popular", a, b});
    }
    {
        Seq a(3000);
        for (uint32_t i = 0; i < 3000; ++i) a[i] = i % 3 == 2 ? 0 : 10 + i;
        Seq b = a;
        b.erase(b.begin() + 1500, b.begin() + 1506);
        b[700] = 5;
        const uint32_t add[3] = {6, 0, 7};
        b.insert(b.begin() + 2222, add, add + 3);
        c.push_back({"every third line", a, b});
    }
    for (int t = 0; t < 200; ++t) {
        const uint32_t k = 2 + uint32_t(below(49));
        Seq a(below(401)), b(below(401));
        for (uint32_t &x : a) x = uint32_t(below(k));
        for (uint32_t &x : b) x = uint32_t(below(k));
        c.push_back({"random", a, b});
    }
    return c;
}

static void check_script(const Case &C, uint32_t n, const std::vector<cdc_diff_op> &ops)
{
    const Seq &a = C.a, &b = C.b;
    uint32_t pi = 0, pj = 0;  // the end of the group before
    for (size_t g0 = 0; g0 < ops.size();) {
        size_t g1 = g0;
        while (g1 < ops.size() && ops[g1].group == ops[g0].group) ++g1;
        CHECK(g0 == 0 || ops[g0].group == ops[g0 - 1].group + 1, "%s: group numbers", C.name.c_str());
        const cdc_diff_op &f = ops[g0], &l = ops[g1 - 1];
        CHECK(f.i1 >= pi && f.j1 >= pj && f.i1 - pi == f.j1 - pj, "%s: the stretch before a group", C.name.c_str());
        for (uint32_t k = 0; k < f.i1 - pi; ++k) CHECK(a[pi + k] == b[pj + k], "%s: unequal ids outside the groups", C.name.c_str());
        bool change = false;
        for (size_t k = g0; k < g1; ++k) {
            const cdc_diff_op &c = ops[k];
            CHECK(c.tag <= dplan::kInsert && c.i1 <= c.i2 && c.i2 <= a.size() && c.j1 <= c.j2 && c.j2 <= b.size(), "%s: op bounds",
                  C.name.c_str());
            if (k > g0) CHECK(c.i1 == ops[k - 1].i2 && c.j1 == ops[k - 1].j2, "%s: ops not back to back", C.name.c_str());
            if (k > g0) CHECK((c.tag == dplan::kEqual) != (ops[k - 1].tag == dplan::kEqual), "%s: two ops of a kind", C.name.c_str());
            if (c.tag == dplan::kEqual) {
                CHECK(c.i2 - c.i1 == c.j2 - c.j1, "%s: equal op sizes", C.name.c_str());
                for (uint32_t t = 0; t < c.i2 - c.i1; ++t) CHECK(a[c.i1 + t] == b[c.j1 + t], "%s: equal op over unequal ids", C.name.c_str());
                if (k == g0 || k == g1 - 1) CHECK(c.i2 - c.i1 <= n, "%s: more context than n", C.name.c_str());
                else CHECK(c.i2 - c.i1 <= 2 * n, "%s: a stretch that should split the group", C.name.c_str());
            } else {
                change = true;
                CHECK((c.tag == dplan::kReplace) == (c.i1 < c.i2 && c.j1 < c.j2), "%s: replace", C.name.c_str());
                CHECK((c.tag == dplan::kDelete) == (c.i1 < c.i2 && c.j1 == c.j2), "%s: delete", C.name.c_str());
                CHECK((c.tag == dplan::kInsert) == (c.i1 == c.i2 && c.j1 < c.j2), "%s: insert", C.name.c_str());
            }
        }
        CHECK(change, "%s: a group without a change", C.name.c_str());
        pi = l.i2, pj = l.j2;
        g0 = g1;
    }
    CHECK(a.size() - pi == b.size() - pj, "%s: the stretch after the last group", C.name.c_str());
    for (size_t k = 0; k < a.size() - pi; ++k) CHECK(a[pi + k] == b[pj + k], "%s: unequal ids after the last group", C.name.c_str());
}

// the text of the ids as lines "L<id>", with (off, len) records into one heap buffer of exactly its size
struct Text {
    uint8_t *plain;
    size_t size;
    std::vector<cdc_line_rec> a, b;
};
static Text make_text(const Case &C)
{
    std::string s;
    Text T{};
    for (int side = 0; side < 2; ++side)
        for (uint32_t id : side ? C.b : C.a) {
            char buf[24];
            const int n = id % 7 == 0 ? 0 : snprintf(buf, sizeof(buf), "L%u", id);  // some lines are empty
            cdc_line_rec r{};
            r.off = s.size(), r.len = uint32_t(n);
            (side ? T.b : T.a).push_back(r);
            s.append(buf, size_t(n));
            s.push_back('\n');
        }
    T.size = s.size();
    T.plain = static_cast<uint8_t *>(malloc(T.size ? T.size : 1));
    memcpy(T.plain, s.data(), T.size);
    return T;
}

static std::string render(const std::vector<cdc_diff_op> &ops, const Text &T)
{
    std::string out;
    auto rng = [](uint32_t start, uint32_t stop) {
        char buf[40];
        const uint32_t len = stop - start;
        if (len == 1) snprintf(buf, sizeof(buf), "%u", start + 1);
        else if (len == 0) snprintf(buf, sizeof(buf), "%u,0", start);
        else snprintf(buf, sizeof(buf), "%u,%u", start + 1, len);
        return std::string(buf);
    };
    auto line = [&](char p, const cdc_line_rec &r) {
        out.push_back(p);
        out.append(reinterpret_cast<const char *>(T.plain) + r.off, r.len);
        out.push_back('\n');
    };
    for (size_t g0 = 0; g0 < ops.size();) {
        size_t g1 = g0;
        while (g1 < ops.size() && ops[g1].group == ops[g0].group) ++g1;
        if (g0 == 0) out += "--- old name\n+++ new name\n";
        out += "@@ -" + rng(ops[g0].i1, ops[g1 - 1].i2) + " +" + rng(ops[g0].j1, ops[g1 - 1].j2) + " @@\n";
        for (size_t k = g0; k < g1; ++k) {
            const cdc_diff_op &c = ops[k];
            if (c.tag == dplan::kEqual) {
                for (uint32_t i = c.i1; i < c.i2; ++i) line(' ', T.a[i]);
                continue;
            }
            for (uint32_t i = c.i1; i < c.i2; ++i) line('-', T.a[i]);
            for (uint32_t j = c.j1; j < c.j2; ++j) line('+', T.b[j]);
        }
        g0 = g1;
    }
    return out;
}

static size_t check_plan(const Case &C, const std::vector<cdc_diff_op> &ops, const Text &T)
{
    dplan::Plan P;
    const uint64_t dst_base = below(100), lit_base = below(100);
    dplan::emit_plan(ops.data(), ops.size(), T.a.data(), T.b.data(), "old name", "new name", dst_base, lit_base, P);
    const std::string want = render(ops, T);
    CHECK(P.out_bytes == want.size(), "%s: out_bytes %llu, rendering %zu", C.name.c_str(), (unsigned long long)P.out_bytes, want.size());
    uint8_t *out = static_cast<uint8_t *>(malloc(P.out_bytes ? P.out_bytes : 1));
    uint8_t *lit = static_cast<uint8_t *>(malloc(P.lit.size() ? P.lit.size() : 1));
    memcpy(lit, P.lit.data(), P.lit.size());
    uint64_t end = dst_base;
    for (const cdc_emit_rec &r : P.recs) {
        CHECK(r.dst_off == end, "%s: destinations not back to back", C.name.c_str());
        const bool is_lit = r.flags & CDC_EMIT_LITERAL;
        const uint64_t so = is_lit ? r.src_off - lit_base : r.src_off;
        CHECK(r.src_off >= (is_lit ? lit_base : 0) && so + r.len <= (is_lit ? P.lit.size() : T.size), "%s: source range", C.name.c_str());
        CHECK(r.dst_off - dst_base + dplan::rec_out_bytes(r) <= P.out_bytes, "%s: destination range", C.name.c_str());
        uint8_t *d = out + (r.dst_off - dst_base);
        if (r.flags & CDC_EMIT_PREFIX) *d++ = uint8_t(r.flags);
        memcpy(d, (is_lit ? lit : T.plain) + so, r.len);
        if (r.flags & CDC_EMIT_NEWLINE) d[r.len] = '\n';
        end = r.dst_off + dplan::rec_out_bytes(r);
    }
    CHECK(end - dst_base == P.out_bytes, "%s: the records do not fill the output", C.name.c_str());
    CHECK(memcmp(out, want.data(), want.size()) == 0, "%s: the executed plan is not the rendering", C.name.c_str());
    uint64_t groups = ops.empty() ? 0 : ops.back().group + 1;
    CHECK(P.hunks == groups, "%s: hunks", C.name.c_str());
    free(out);
    free(lit);
    return P.recs.size();
}

// exact ids from cut hashes: the device's comparison replaced by memcmp
static uint32_t check_ids(const Case &C, const Text &T, int hash_bits)
{
    std::vector<cdc_line_rec> L(T.a);
    L.insert(L.end(), T.b.begin(), T.b.end());
    std::map<std::string, uint32_t> first;
    std::vector<uint32_t> want(L.size());
    for (size_t i = 0; i < L.size(); ++i) {
        const std::string s(reinterpret_cast<const char *>(T.plain) + L[i].off, L[i].len);
        want[i] = first.emplace(s, uint32_t(i)).first->second;
        uint64_t h = 1469598103934665603ull;  // equal lines, equal hashes
        for (char ch : s) h = (h ^ uint8_t(ch)) * 1099511628211ull;
        L[i].hash[0] = h ^ (h >> 29), L[i].hash[1] = h * 0x9E3779B97F4A7C15ull;
    }
    dplan::Ids I;
    I.propose(L.data(), L.size(), hash_bits);
    std::vector<size_t> todo, next;
    for (size_t i = 0; i < L.size(); ++i)
        if (I.cand[i] != i) todo.push_back(i);
    uint32_t rounds = 0;
    for (bool firstround = true; !todo.empty(); firstround = false) {
        next.clear();
        for (size_t i : todo) {
            if (!firstround) I.relead(i);
            while (I.cand[i] != i && L[I.cand[i]].len != L[i].len) I.relead(i);
            if (I.cand[i] != i) next.push_back(i);
        }
        if (next.empty()) break;
        ++rounds;
        CHECK(rounds <= L.size() + 1, "%s: the rounds do not end", C.name.c_str());
        todo.clear();
        for (size_t i : next)
            if (memcmp(T.plain + L[i].off, T.plain + L[I.cand[i]].off, L[i].len) != 0) todo.push_back(i);
    }
    for (size_t i = 0; i < L.size(); ++i)
        CHECK(I.cand[i] == want[i], "%s: id of line %zu is %u, not %u (hash_bits %d)", C.name.c_str(), i, I.cand[i], want[i], hash_bits);
    return rounds;
}

int main()
{
    const std::vector<Case> all = cases();
    size_t nops = 0, nrecs = 0, nrounds = 0;
    for (size_t ci = 0; ci < all.size(); ++ci) {
        const Case &C = all[ci];
        const Text T = make_text(C);
        for (uint32_t n : {0u, 1u, 3u}) {
            const std::vector<cdc_diff_op> ops = dplan::script(C.a.data(), C.a.size(), C.b.data(), C.b.size(), n);
            check_script(C, n, ops);
            nrecs += check_plan(C, ops, T);
            nops += ops.size();
        }
        nrounds += check_ids(C, T, int(ci % 7));  // 0: all 128 bits
        free(T.plain);
    }
    // the range format's three forms
    CHECK(dplan::format_range(4, 5) == "5" && dplan::format_range(4, 4) == "4,0" && dplan::format_range(4, 9) == "5,5" &&
              dplan::format_range(0, 0) == "0,0",
          "format_range");
    printf("%zu cases, %zu ops, %zu records, %zu rounds, ok\n", all.size(), nops, nrecs, nrounds);
    return 0;
}
