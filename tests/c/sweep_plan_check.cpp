// Stand-alone check of the host-only pieces of maintenance,
// built with -fsanitize=address,undefined by tests/test_maintenance_cpu.py:
//
//   swplan::verdict        the thresholds, against 128-bit arithmetic
//   swplan::group_repack   the grouping sort of the repack rows, against a
//                          brute-force restatement
//   splan::serialize_deleted   a state with deleted snapshots, read back with
//                          splan::read and by hand
//
// Prints "<v> verdicts, <g> groupings, <w> writer checks, ok" and exits 0, or
// the line of the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "state_plan.h"
#include "sweep_plan.h"

#define REQUIRE(c)                                                  \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                           \
        }                                                           \
    } while (0)

static uint64_t g_verdicts = 0, g_groupings = 0, g_writer = 0;

static int32_t wide_verdict(uint64_t rows, uint64_t bytes, uint64_t extent, uint32_t permille)
{
    if (!rows) return CDC_SWEEP_DROP;
    return (unsigned __int128)bytes * 1000 < (unsigned __int128)extent * permille ? CDC_SWEEP_REPACK : CDC_SWEEP_KEEP;
}

static void verdict_is(uint64_t rows, uint64_t bytes, uint64_t extent, uint32_t permille, int32_t want)
{
    ++g_verdicts;
    REQUIRE(swplan::verdict(rows, bytes, extent, permille) == want);
    REQUIRE(wide_verdict(rows, bytes, extent, permille) == want);
}

static void check_verdicts()
{
    // exactly at live * 1000 == extent * permille, and one byte either side
    verdict_is(3, 500, 1000, 500, CDC_SWEEP_KEEP);
    verdict_is(3, 499, 1000, 500, CDC_SWEEP_REPACK);
    verdict_is(3, 501, 1000, 500, CDC_SWEEP_KEEP);
    verdict_is(1, 250, 1000, 250, CDC_SWEEP_KEEP);
    verdict_is(1, 249, 1000, 250, CDC_SWEEP_REPACK);
    verdict_is(1, 1, 3, 333, CDC_SWEEP_KEEP);     // 1000 >= 999
    verdict_is(1, 1, 3, 334, CDC_SWEEP_REPACK);   // 1000 < 1002
    // nothing live is DROP whatever the rest says
    verdict_is(0, 0, 1000, 500, CDC_SWEEP_DROP);
    verdict_is(0, 0, 0, 0, CDC_SWEEP_DROP);
    verdict_is(0, 900, 1000, 1000, CDC_SWEEP_DROP);
    // permille 0 never repacks
    verdict_is(1, 0, 1000, 0, CDC_SWEEP_KEEP);
    verdict_is(1, 1, UINT64_MAX, 0, CDC_SWEEP_KEEP);
    // permille 1000 repacks every packfile that is not entirely live
    verdict_is(2, 1000, 1000, 1000, CDC_SWEEP_KEEP);
    verdict_is(2, 999, 1000, 1000, CDC_SWEEP_REPACK);
    verdict_is(1, 0, 1, 1000, CDC_SWEEP_REPACK);
    // an extent past 2^32: 0xFFFFFFF0 + 0x20, added as u64
    const uint64_t far = uint64_t(0xFFFFFFF0u) + 0x20;
    REQUIRE(far == 0x100000010ull);
    verdict_is(1, far / 2, far, 500, CDC_SWEEP_KEEP);
    verdict_is(1, far / 2 - 1, far, 500, CDC_SWEEP_REPACK);
    verdict_is(1, 0x20, far, 500, CDC_SWEEP_REPACK);
    verdict_is(1, 0x20, far, 0, CDC_SWEEP_KEEP);
    // products past 2^64 on either side
    verdict_is(1, UINT64_MAX, UINT64_MAX, 1000, CDC_SWEEP_KEEP);
    verdict_is(1, UINT64_MAX - 1, UINT64_MAX, 1000, CDC_SWEEP_REPACK);
    verdict_is(1, UINT64_MAX / 2, UINT64_MAX, 500, CDC_SWEEP_REPACK);  // (2^64 - 1) / 2 rounds down
    verdict_is(1, UINT64_MAX / 2 + 1, UINT64_MAX, 500, CDC_SWEEP_KEEP);
    std::mt19937_64 rng(7);
    for (int i = 0; i < 20000; ++i) {
        const int sh = int(rng() % 64);
        const uint64_t extent = rng() >> sh, bytes = extent ? (rng() >> sh) % extent + (rng() % 8 == 0) : 0;
        const uint32_t permille = uint32_t(rng() % 1001);
        const uint64_t rows = rng() % 3;
        verdict_is(rows, bytes, extent, permille, wide_verdict(rows, bytes, extent, permille));
        if (permille && extent < (UINT64_MAX / 1000)) {  // on the threshold itself, where it is a whole number
            const uint64_t at = extent * permille;
            if (at % 1000 == 0) {
                verdict_is(1, at / 1000, extent, permille, CDC_SWEEP_KEEP);
                if (at) verdict_is(1, at / 1000 - 1, extent, permille, CDC_SWEEP_REPACK);
            }
        }
    }
}

static void fill_sum(uint8_t *out, uint32_t tag, uint32_t i)
{
    for (int k = 0; k < 32; ++k) out[k] = uint8_t(tag * 131 + i * 31 + k * 7 + (i >> 8));
}

static void check_grouping()
{
    std::mt19937_64 rng(11);
    for (int round = 0; round < 200; ++round) {
        const uint64_t npacks = 1 + rng() % 9, n = round == 0 ? 0 : rng() % 300;
        std::vector<cdc_sweep_pack> packs(npacks, cdc_sweep_pack{});
        for (uint64_t i = 0; i < npacks; ++i) {
            fill_sum(packs[i].packfile, 1, uint32_t(i));
            packs[i].row_first = packs[i].row_count = 77;  // overwritten
        }
        std::vector<cdc_state_row> rows(n, cdc_state_row{});
        for (uint64_t i = 0; i < n; ++i) {
            fill_sum(rows[i].checksum, 2, uint32_t(i));
            std::memcpy(rows[i].packfile, packs[rng() % npacks].packfile, 32);
            rows[i].offset = uint32_t(rng() % 40) * (rng() % 2 ? 1u : 0x08000000u);  // ties, and offsets past 2^31
            rows[i].length = uint32_t(i);  // the order given, to check that ties keep it
        }
        // brute force: for each pack in order, its rows by (offset, position given)
        std::vector<cdc_state_row> want;
        std::vector<uint64_t> first(npacks, 0), count(npacks, 0);
        for (uint64_t p = 0; p < npacks; ++p) {
            std::vector<cdc_state_row> mine;
            for (const cdc_state_row &r : rows)
                if (!std::memcmp(r.packfile, packs[p].packfile, 32)) mine.push_back(r);
            for (size_t a = 1; a < mine.size(); ++a)  // insertion sort: stable
                for (size_t b = a; b > 0 && mine[b - 1].offset > mine[b].offset; --b) std::swap(mine[b - 1], mine[b]);
            first[p] = mine.empty() ? 0 : want.size(), count[p] = mine.size();
            want.insert(want.end(), mine.begin(), mine.end());
        }
        REQUIRE(swplan::group_repack(rows.data(), n, packs.data(), npacks) == CDC_OK);
        REQUIRE(want.size() == n && (n == 0 || !std::memcmp(want.data(), rows.data(), n * sizeof(cdc_state_row))));
        uint64_t at = 0;
        for (uint64_t p = 0; p < npacks; ++p) {
            REQUIRE(packs[p].row_first == first[p] && packs[p].row_count == count[p]);
            if (count[p]) REQUIRE(packs[p].row_first == at);  // the slices tile the list
            at += count[p];
            for (uint64_t k = 1; k < count[p]; ++k) REQUIRE(rows[first[p] + k - 1].offset <= rows[first[p] + k].offset);
        }
        REQUIRE(at == n);
        ++g_groupings;
    }
    // a row whose packfile is not in the list: refused, nothing moved
    std::vector<cdc_sweep_pack> packs(1, cdc_sweep_pack{});
    std::vector<cdc_state_row> rows(2, cdc_state_row{});
    rows[1].packfile[0] = 1, rows[0].offset = 9;
    const std::vector<cdc_state_row> before = rows;
    REQUIRE(swplan::group_repack(rows.data(), 2, packs.data(), 1) == CDC_E_INVALID);
    REQUIRE(!std::memcmp(before.data(), rows.data(), 2 * sizeof(cdc_state_row)));
    ++g_groupings;
}

static void check_writer()
{
    // 3 rows (one repeats a key and is dropped), 3 deletions: one of a checksum a row
    // names (it keeps the row's id), one new, and the new one again with a later time
    std::vector<cdc_state_row> rows(3, cdc_state_row{});
    for (uint32_t i = 0; i < 3; ++i) {
        fill_sum(rows[i].checksum, 3, i == 2 ? 0 : i);
        fill_sum(rows[i].packfile, 4, 0);
        rows[i].offset = 10 * i, rows[i].length = 5, rows[i].type = 0;
    }
    uint8_t gone[3 * 32];
    fill_sum(gone, 5, 0);               // new: id 3 (pack 0, blob 1, blob 2 came first)
    fill_sum(gone + 32, 3, 1);          // rows[1]'s checksum: id 2
    fill_sum(gone + 64, 5, 0);          // again
    const int64_t times[3] = {100, -7, 300};
    uint8_t ext[32];
    fill_sum(ext, 6, 0);
    uint64_t len = 0, len2 = 0;
    REQUIRE(splan::serialize_deleted(rows.data(), 3, gone, times, 3, 42, 1, ext, 1, nullptr, 0, &len) == CDC_E_NOSPACE);
    REQUIRE(len == splan::kMinBytes + 32 + 2 * 16 + 4 * 40 + 2 * 24);
    std::vector<uint8_t> out(len);
    REQUIRE(splan::serialize_deleted(rows.data(), 3, gone, times, 3, 42, 1, ext, 1, out.data(), len - 1, &len2) == CDC_E_NOSPACE);
    REQUIRE(splan::serialize_deleted(rows.data(), 3, gone, times, 3, 42, 1, ext, 1, out.data(), len, &len2) == CDC_OK && len2 == len);
    ++g_writer;
    splan::Layout L;
    REQUIRE(splan::read(out.data(), len, &L) == CDC_OK);
    REQUIRE(L.version == splan::kVersion && L.timestamp == 42 && L.aggregate == 1 && L.extends.count == 1 && L.end == len);
    REQUIRE(L.sec[splan::kSecDeleted].count == 2 && L.sec[splan::kSecIds].count == 4);
    REQUIRE(L.sec[splan::section_of_type(0)].count == 2);
    const uint8_t *d = out.data() + L.sec[splan::kSecDeleted].off;
    REQUIRE(splan::rd64(d) == 2 && int64_t(splan::rd64(d + 8)) == -7);      // ascending id: rows[1]'s checksum first
    REQUIRE(splan::rd64(d + 16) == 3 && splan::rd64(d + 24) == 300);        // the last time given stays
    const uint8_t *ids = out.data() + L.sec[splan::kSecIds].off;
    REQUIRE(splan::rd64(ids + 40 * 3) == 3 && !std::memcmp(ids + 40 * 3 + 8, gone, 32));
    REQUIRE(splan::rd64(ids + 40 * 2) == 2 && !std::memcmp(ids + 40 * 2 + 8, gone + 32, 32));
    ++g_writer;
    // without deletions the bytes are serialize's
    uint64_t a = 0, b = 0;
    REQUIRE(splan::serialize(rows.data(), 3, 42, 0, nullptr, 0, nullptr, 0, &a) == CDC_E_NOSPACE);
    std::vector<uint8_t> x(a), y(a);
    REQUIRE(splan::serialize(rows.data(), 3, 42, 0, nullptr, 0, x.data(), a, &a) == CDC_OK);
    REQUIRE(splan::serialize_deleted(rows.data(), 3, nullptr, nullptr, 0, 42, 0, nullptr, 0, y.data(), a, &b) == CDC_OK);
    REQUIRE(a == b && x == y && a == splan::kMinBytes + 3 * 40 + 2 * 24);
    ++g_writer;
    // deletions alone: what `rm` stores
    REQUIRE(splan::serialize_deleted(nullptr, 0, gone, times, 1, 1, 0, nullptr, 0, nullptr, 0, &a) == CDC_E_NOSPACE);
    REQUIRE(a == splan::kMinBytes + 16 + 40);
    std::vector<uint8_t> z(a);
    REQUIRE(splan::serialize_deleted(nullptr, 0, gone, times, 1, 1, 0, nullptr, 0, z.data(), a, &b) == CDC_OK && b == a);
    REQUIRE(splan::read(z.data(), a, &L) == CDC_OK && L.sec[splan::kSecDeleted].count == 1 && L.sec[splan::kSecIds].count == 1);
    // every truncation of it is rejected, and read stays inside the bytes given (the sanitizer watches)
    for (uint64_t cut = 0; cut < a; ++cut) {
        std::vector<uint8_t> part(z.begin(), z.begin() + cut);
        REQUIRE(splan::read(part.data(), cut, &L) == CDC_E_CORRUPT);
    }
    ++g_writer;
}

int main()
{
    check_verdicts();
    check_grouping();
    check_writer();
    std::printf("%llu verdicts, %llu groupings, %llu writer checks, ok\n", (unsigned long long)g_verdicts,
                (unsigned long long)g_groupings, (unsigned long long)g_writer);
    return 0;
}
