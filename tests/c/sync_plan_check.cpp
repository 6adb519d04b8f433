// Stand-alone check of the sync planner (plakar_amd/csrc/sync_plan.h), built
// with -fsanitize=address,undefined by tests/test_sync_pipeline_cpu.py: the
// 33-byte search against a linear scan (first, last and absent keys, empty and
// one-record lists), the sortedness test, and seeded random row lists
// (duplicate rows, one checksum under two types, known and wanted subsets,
// zero-length rows, rows larger than the budget) against a brute-force
// restatement of the filter and the cut; then the packers' split.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "sync_plan.h"

using namespace splan;

static int g_fail = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            ++g_fail;                                                  \
        }                                                              \
    } while (0)

static bool linear(const std::vector<Key> &v, const Key &k)
{
    for (const Key &x : v)
        if (x == k) return true;
    return false;
}

static std::vector<uint8_t> flat(std::vector<Key> v)
{
    std::sort(v.begin(), v.end(), [](const Key &a, const Key &b) { return memcmp(a.b, b.b, kKeyBytes) < 0; });
    std::vector<uint8_t> out;
    for (const Key &k : v) out.insert(out.end(), k.b, k.b + kKeyBytes);
    return out;
}

static Key make_key(uint8_t type, uint32_t id)
{
    Key k;
    memset(k.b, 0, sizeof(k.b));
    k.b[0] = type;
    // the id in the checksum's LAST bytes: keys that differ late, so a search that compared a prefix only would fail
    k.b[29] = uint8_t(id >> 24), k.b[30] = uint8_t(id >> 16), k.b[31] = uint8_t(id >> 8), k.b[32] = uint8_t(id);
    k.b[1] = uint8_t(id * 131);
    return k;
}

static void check_search()
{
    EXPECT(sorted33(nullptr, 0));
    EXPECT(!contains33(nullptr, 0, make_key(1, 1).b));
    for (uint32_t n : {1u, 2u, 3u, 7u, 64u, 1000u}) {
        std::vector<Key> keys;
        for (uint32_t i = 0; i < n; ++i) keys.push_back(make_key(uint8_t(1 + i % 5), 2 * i + 2));
        const std::vector<uint8_t> recs = flat(keys);
        EXPECT(sorted33(recs.data(), n));
        // every key present, the first and the last of the sorted list among them
        for (uint32_t i = 0; i < n; ++i) EXPECT(contains33(recs.data(), n, keys[i].b));
        EXPECT(contains33(recs.data(), n, recs.data()));
        EXPECT(contains33(recs.data(), n, recs.data() + kKeyBytes * (n - 1)));
        // absent: between the records, below the first, above the last, the same checksum under another type
        for (uint32_t i = 0; i <= n; ++i) {
            const Key a = make_key(uint8_t(1 + i % 5), 2 * i + 1);
            EXPECT(contains33(recs.data(), n, a.b) == linear(keys, a));
        }
        Key lo, hi;
        memset(lo.b, 0, sizeof(lo.b));
        memset(hi.b, 0xff, sizeof(hi.b));
        EXPECT(!contains33(recs.data(), n, lo.b) && !contains33(recs.data(), n, hi.b));
        Key other = keys[0];
        other.b[0] = 9;
        EXPECT(!contains33(recs.data(), n, other.b));
        if (n >= 2) {  // out of order
            std::vector<uint8_t> bad = recs;
            std::swap_ranges(bad.begin(), bad.begin() + kKeyBytes, bad.begin() + kKeyBytes * (n - 1));
            EXPECT(!sorted33(bad.data(), n));
        }
    }
}

// The filter and the cut, restated without a search structure.
struct Ref {
    std::vector<Item> items;
    std::vector<Batch> batches;
    uint64_t skipped = 0;
};
static Ref brute(const std::vector<std::vector<cdc_packfile_row>> &packs, const std::vector<Key> &known,
                 const std::vector<Key> *wanted, uint64_t budget)
{
    Ref R;
    std::vector<Key> taken;
    uint64_t first = 0, count = 0, bytes = 0;
    for (size_t p = 0; p < packs.size(); ++p)
        for (size_t r = 0; r < packs[p].size(); ++r) {
            const Key k = key_of(packs[p][r]);
            if (wanted && !linear(*wanted, k)) continue;
            if (linear(known, k) || linear(taken, k)) {
                ++R.skipped;
                continue;
            }
            taken.push_back(k);
            if (count && bytes + packs[p][r].length > budget) {
                R.batches.push_back(Batch{first, count, bytes});
                first += count;
                count = bytes = 0;
            }
            R.items.push_back(Item{uint32_t(p), uint32_t(r)});
            ++count;
            bytes += packs[p][r].length;
        }
    if (count) R.batches.push_back(Batch{first, count, bytes});
    return R;
}

static int check_plans()
{
    std::mt19937_64 rng(20240607);
    int lists = 0;
    for (int round = 0; round < 400; ++round) {
        const uint64_t budget = (round % 7 == 0) ? 1 : 1000 + rng() % 100000;
        const uint32_t ids = 1 + uint32_t(rng() % 60);
        std::vector<std::vector<cdc_packfile_row>> packs(1 + rng() % 4);
        std::vector<Key> all;
        for (auto &rows : packs) {
            const size_t n = rng() % 80;  // an empty packfile now and then
            for (size_t i = 0; i < n; ++i) {
                // few ids and few types: duplicate rows, and one checksum under two types
                const Key k = make_key(uint8_t(1 + rng() % 3), uint32_t(rng() % ids));
                cdc_packfile_row r;
                memset(&r, 0, sizeof(r));
                r.type = k.b[0];
                memcpy(r.checksum, k.b + 1, 32);
                const uint64_t pick = rng() % 10;
                r.length = pick == 0 ? 0 : pick == 1 ? uint32_t(budget + 1 + rng() % 5000) : uint32_t(rng() % (budget / 3 + 2));
                r.offset = uint32_t(rng());
                rows.push_back(r);
                all.push_back(k);
            }
        }
        std::vector<Key> known, wanted;
        for (const Key &k : all) {
            if (rng() % 5 == 0) known.push_back(k);
            if (rng() % 2 == 0) wanted.push_back(k);
        }
        wanted.push_back(make_key(7, 12345));  // a pair no packfile holds
        const bool use_wanted = round % 3 != 0;
        const std::vector<uint8_t> kf = flat(known), wf = flat(wanted);
        std::vector<Pack> in;
        for (auto &rows : packs) in.push_back(Pack{rows.data(), rows.size()});
        Plan P;
        plan(in.data(), in.size(), kf.data(), known.size(), use_wanted ? wf.data() : nullptr, wanted.size(), budget, P);
        const Ref R = brute(packs, known, use_wanted ? &wanted : nullptr, budget);
        EXPECT(P.skipped == R.skipped);
        EXPECT(P.items.size() == R.items.size() && P.batches.size() == R.batches.size());
        if (P.items.size() != R.items.size() || P.batches.size() != R.batches.size()) continue;
        // every eligible row exactly once, in order
        for (size_t i = 0; i < P.items.size(); ++i)
            EXPECT(P.items[i].pack == R.items[i].pack && P.items[i].row == R.items[i].row);
        uint64_t next = 0, bytes = 0;
        for (size_t b = 0; b < P.batches.size(); ++b) {
            const Batch &B = P.batches[b];
            EXPECT(B.first == next && B.count >= 1);
            EXPECT(B.first == R.batches[b].first && B.count == R.batches[b].count && B.bytes == R.batches[b].bytes);
            uint64_t sum = 0;
            for (uint64_t i = B.first; i < B.first + B.count; ++i) sum += packs[P.items[i].pack][P.items[i].row].length;
            EXPECT(sum == B.bytes);
            EXPECT(B.bytes <= budget || B.count == 1);  // over the budget only alone
            next += B.count;
            bytes += B.bytes;
        }
        EXPECT(next == P.items.size() && bytes == P.bytes);
        ++lists;
    }
    // a budget of 0 is a budget of 1; no packfile at all is an empty plan
    Plan P;
    plan(nullptr, 0, nullptr, 0, nullptr, 0, 0, P);
    EXPECT(P.items.empty() && P.batches.empty() && P.skipped == 0);
    return lists;
}

static int check_split()
{
    std::mt19937_64 rng(77);
    int n_ok = 0;
    std::vector<uint32_t> bounds;
    for (int round = 0; round < 300; ++round) {
        const uint32_t n = uint32_t(rng() % 50);
        const uint32_t parts = round % 9 == 0 ? 1 : 1 + uint32_t(rng() % 12);
        std::vector<uint64_t> off(size_t(n) + 1);
        off[0] = rng() % 1000;  // offsets need not start at 0
        for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + (rng() % 4 == 0 ? 0 : rng() % (round % 2 ? 100000 : 1ull << 40));
        split(off.data(), n, parts, bounds);
        EXPECT(bounds.size() == size_t(parts) + 1 && bounds[0] == 0 && bounds[parts] == n);
        const uint64_t total = off[n] - off[0];
        for (uint32_t p = 0; p < parts; ++p) {
            EXPECT(bounds[p] <= bounds[p + 1]);
            // no range but the last holds more than its share plus one blob
            if (p + 1 < parts && bounds[p + 1] > bounds[p]) {
                const uint64_t start = off[bounds[p + 1] - 1] - off[0];  // the range's last blob starts below the next share
                EXPECT(start <= total / parts * (p + 1) + total % parts * (p + 1) / parts);
            }
        }
        ++n_ok;
    }
    split(std::vector<uint64_t>{5}.data(), 0, 0, bounds);  // no blob, and 0 parts means 1
    EXPECT(bounds.size() == 2 && bounds[0] == 0 && bounds[1] == 0);
    return n_ok;
}

int main()
{
    check_search();
    const int lists = check_plans();
    const int splits = check_split();
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("%d row lists, %d splits, ok\n", lists, splits);
    return 0;
}
