// Stand-alone check of plakar_amd/csrc/state_plan.h (host only), built with
// -fsanitize=address,undefined by tests/test_state_cpu.py.
//
// The reader is compared with a brute-force restatement of DeserializeStream
// (repository/state/state.go:235-378) that walks the stream front to back and
// holds every count against the remaining bytes by a 128-bit multiplication
// (the planner divides), over
//   * every truncation length 0..len of a state with two records in every
//     section (and two extends);
//   * each of the 12 counts set to 2^61, 2^64 - 1, remaining / record size + 1
//     and remaining / record size;
//   * 10,000 seeded random mutations of that state, half of them inside a count;
//   * the writer's output for rows with repeats, read back and decoded into
//     the maps SetPackfileForBlob would hold.
// The state's bytes sit in exactly-sized heap buffers so that a read past
// either end is a sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "state_plan.h"

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

static void put(std::vector<uint8_t> &v, uint64_t x, int bytes)
{
    for (int k = 0; k < bytes; ++k) v.push_back(uint8_t(x >> (8 * k)));
}
static uint64_t get(const std::vector<uint8_t> &v, uint64_t at, int bytes)
{
    uint64_t x = 0;
    for (int k = bytes - 1; k >= 0; --k) x = x << 8 | v[size_t(at + k)];
    return x;
}
static void put_sum(std::vector<uint8_t> &v, uint8_t tag)
{
    for (int k = 0; k < 32; ++k) v.push_back(uint8_t(tag + 3 * k));
}

// record sizes in stream order: extends, deleted, ids, nine location maps
static const uint64_t kRec[12] = {32, 16, 40, 24, 24, 24, 24, 24, 24, 24, 24, 24};

struct Brute {
    bool ok;
    uint64_t off[12], count[12], end;
    uint32_t version;
    uint64_t timestamp;
    uint32_t aggregate;
};
static Brute brute_read(const std::vector<uint8_t> &s)
{
    Brute b{};
    const unsigned __int128 len = s.size();
    unsigned __int128 pos = 0;
    if (pos + 4 > len) return b;
    b.version = uint32_t(get(s, 0, 4)), pos += 4;
    if (pos + 8 > len) return b;
    b.timestamp = get(s, 4, 8), pos += 8;
    if (pos + 1 > len) return b;
    b.aggregate = s[12] == 1, pos += 1;
    for (int k = 0; k < 12; ++k) {
        if (pos + 8 > len) return b;
        const uint64_t n = get(s, uint64_t(pos), 8);
        pos += 8;
        if (pos + (unsigned __int128)n * kRec[k] > len) return b;
        b.off[k] = uint64_t(pos), b.count[k] = n;
        pos += (unsigned __int128)n * kRec[k];
    }
    b.end = uint64_t(pos);
    b.ok = true;
    return b;
}

static uint64_t n_accept = 0, n_reject = 0;

static void check(const std::vector<uint8_t> &s)
{
    // an exactly-sized copy: one byte past it is the sanitizer's
    uint8_t *buf = static_cast<uint8_t *>(std::malloc(s.size() ? s.size() : 1));
    REQUIRE(buf);
    if (!s.empty()) std::memcpy(buf, s.data(), s.size());
    splan::Layout L;
    const int st = splan::read(s.empty() ? nullptr : buf, s.size(), &L);
    std::free(buf);
    const Brute b = brute_read(s);
    REQUIRE(st == CDC_OK || st == CDC_E_CORRUPT);
    REQUIRE((st == CDC_OK) == b.ok);
    if (!b.ok) {
        splan::Layout Z;
        std::memset(&Z, 0, sizeof(Z));
        REQUIRE(std::memcmp(&L, &Z, sizeof(Z)) == 0);
        ++n_reject;
        return;
    }
    REQUIRE(L.version == b.version && L.timestamp == b.timestamp && L.aggregate == b.aggregate && L.end == b.end);
    REQUIRE(L.extends.off == b.off[0] && L.extends.count == b.count[0]);
    for (uint32_t k = 0; k < splan::kSections; ++k) {
        REQUIRE(L.sec[k].off == b.off[k + 1] && L.sec[k].count == b.count[k + 1]);
        REQUIRE(L.sec[k].off + L.sec[k].count * splan::record_bytes(k) <= s.size());
    }
    ++n_accept;
}

// Two records in every section; where[k] = the offset of count k.
static std::vector<uint8_t> base_state(uint64_t where[12])
{
    std::vector<uint8_t> s;
    put(s, 100, 4), put(s, 1700000000123456789ull, 8), put(s, 1, 1);
    where[0] = s.size(), put(s, 2, 8), put_sum(s, 200), put_sum(s, 201);
    where[1] = s.size(), put(s, 2, 8);
    for (int k = 0; k < 2; ++k) put(s, uint64_t(k), 8), put(s, 555 + k, 8);
    where[2] = s.size(), put(s, 2, 8);
    for (int k = 1; k >= 0; --k) put(s, uint64_t(k), 8), put_sum(s, uint8_t(10 + k));
    for (int t = 0; t < 9; ++t) {
        where[3 + t] = s.size(), put(s, 2, 8);
        for (int k = 0; k < 2; ++k) put(s, uint64_t(k), 8), put(s, uint64_t(1 - k), 8), put(s, 1000 * t + k, 4), put(s, 77 + k, 4);
    }
    return s;
}

static void check_writer()
{
    // rows with a repeated (type, blob), a blob under two types, a packfile that is also a blob
    struct R {
        uint8_t type, blob, pack;
        uint32_t off, len;
    };
    const R in[] = {{1, 50, 90, 0, 10},  {1, 51, 90, 10, 20}, {1, 50, 91, 5, 6},   {2, 50, 91, 30, 7},
                    {0, 60, 92, 1, 2},   {8, 61, 92, 3, 4},   {1, 90, 93, 40, 50}, {7, 62, 90, 9, 9},
                    {6, 51, 93, 8, 1},   {1, 51, 93, 99, 99}};
    const uint64_t n = sizeof(in) / sizeof(in[0]);
    std::vector<cdc_state_row> rows(n);
    // what SetPackfileForBlob leaves, restated over std::map
    std::map<std::string, uint64_t> ids;
    std::map<std::pair<int, uint64_t>, std::tuple<uint64_t, uint32_t, uint32_t>> want;
    auto sum_of = [](uint8_t tag) {
        std::vector<uint8_t> v;
        put_sum(v, tag);
        return std::string(v.begin(), v.end());
    };
    for (uint64_t i = 0; i < n; ++i) {
        std::memset(&rows[i], 0, sizeof(rows[i]));
        const std::string b = sum_of(in[i].blob), p = sum_of(in[i].pack);
        std::memcpy(rows[i].checksum, b.data(), 32), std::memcpy(rows[i].packfile, p.data(), 32);
        rows[i].type = in[i].type, rows[i].offset = in[i].off, rows[i].length = in[i].len;
        const uint64_t pid = ids.emplace(p, ids.size()).first->second, bid = ids.emplace(b, ids.size()).first->second;
        want.emplace(std::make_pair(int(in[i].type), bid), std::make_tuple(pid, in[i].off, in[i].len));
    }
    std::vector<uint8_t> ext;
    put_sum(ext, 1), put_sum(ext, 2), put_sum(ext, 3);
    uint64_t len = 0;
    REQUIRE(splan::serialize(rows.data(), n, -5, 1, ext.data(), 3, nullptr, 0, &len) == CDC_E_NOSPACE);
    REQUIRE(len == 109 + 32 * 3 + 40 * ids.size() + 24 * want.size());
    std::vector<uint8_t> out(len);
    uint64_t len2 = 0;
    REQUIRE(splan::serialize(rows.data(), n, -5, 1, ext.data(), 3, out.data(), len - 1, &len2) == CDC_E_NOSPACE);
    REQUIRE(splan::serialize(rows.data(), n, -5, 1, ext.data(), 3, out.data(), len, &len2) == CDC_OK && len2 == len);
    check(out);
    splan::Layout L;
    REQUIRE(splan::read(out.data(), len, &L) == CDC_OK && L.end == len);
    REQUIRE(L.version == 100 && int64_t(L.timestamp) == -5 && L.aggregate == 1 && L.extends.count == 3);
    REQUIRE(std::memcmp(out.data() + L.extends.off, ext.data(), 96) == 0);
    REQUIRE(L.sec[splan::kSecDeleted].count == 0 && L.sec[splan::kSecIds].count == ids.size());
    for (uint64_t k = 0; k < ids.size(); ++k) {  // ascending, dense, the checksum the id was given for
        const uint64_t at = L.sec[splan::kSecIds].off + 40 * k;
        REQUIRE(get(out, at, 8) == k);
        REQUIRE(ids.at(std::string(out.begin() + at + 8, out.begin() + at + 40)) == k);
    }
    std::map<std::pair<int, uint64_t>, std::tuple<uint64_t, uint32_t, uint32_t>> got;
    for (uint32_t s = splan::kSecFirstType; s < splan::kSections; ++s) {
        const int type = int(splan::type_of_section(s));
        REQUIRE(splan::section_of_type(uint32_t(type)) == s);
        uint64_t prev = 0;
        for (uint64_t k = 0; k < L.sec[s].count; ++k) {
            const uint64_t at = L.sec[s].off + 24 * k, id = get(out, at, 8);
            REQUIRE(k == 0 || id > prev);
            prev = id;
            REQUIRE(got.emplace(std::make_pair(type, id), std::make_tuple(get(out, at + 8, 8), uint32_t(get(out, at + 16, 4)),
                                                                           uint32_t(get(out, at + 20, 4)))).second);
        }
    }
    REQUIRE(got == want);
    // SerializeStream's order: Chunks first, Snapshots seventh
    const int order[9] = {1, 2, 3, 4, 5, 6, 0, 7, 8};
    for (int k = 0; k < 9; ++k) REQUIRE(splan::type_of_section(splan::kSecFirstType + k) == uint32_t(order[k]));
    // a type the reference panics on, and the empty state
    rows[0].type = 9;
    REQUIRE(splan::serialize(rows.data(), n, 0, 0, nullptr, 0, out.data(), len, &len2) == CDC_E_INVALID);
    REQUIRE(splan::serialize(nullptr, 0, 0, 0, nullptr, 0, out.data(), len, &len2) == CDC_OK && len2 == splan::kMinBytes);
    out.resize(len2);
    check(out);
}

int main()
{
    uint64_t where[12];
    const std::vector<uint8_t> base = base_state(where);
    REQUIRE(base.size() == 109 + 32 * 2 + 16 * 2 + 40 * 2 + 24 * 18);

    // every truncation
    uint64_t n_trunc_ok = 0;
    for (uint64_t L = 0; L <= base.size(); ++L) {
        const uint64_t before = n_accept;
        check(std::vector<uint8_t>(base.begin(), base.begin() + L));
        n_trunc_ok += n_accept - before;
    }
    REQUIRE(n_trunc_ok == 1);  // only the whole state
    {   // bytes after the last section are ignored; the smallest state is 109 bytes of zero counts
        std::vector<uint8_t> s = base;
        s.insert(s.end(), 7, 0xEE);
        const uint64_t before = n_accept;
        check(s);
        REQUIRE(n_accept == before + 1);
        std::vector<uint8_t> z(109, 0);
        check(z);
        REQUIRE(n_accept == before + 2);
        z.pop_back();
        check(z);
        REQUIRE(n_accept == before + 2);
    }

    // the counts
    uint64_t n_counts = 0;
    for (int k = 0; k < 12; ++k) {
        const uint64_t remaining = base.size() - (where[k] + 8);
        const uint64_t vals[4] = {1ull << 61, UINT64_MAX, remaining / kRec[k] + 1, remaining / kRec[k]};
        for (int v = 0; v < 4; ++v) {
            std::vector<uint8_t> s = base;
            for (int b = 0; b < 8; ++b) s[size_t(where[k] + b)] = uint8_t(vals[v] >> (8 * b));
            const uint64_t before = n_accept;
            check(s);
            if (v < 3) REQUIRE(n_accept == before);  // none of these fits
            ++n_counts;
        }
    }

    // random mutations
    for (int it = 0; it < 10000; ++it) {
        std::vector<uint8_t> s = base;
        const int edits = 1 + int(rnd() % 3);
        for (int e = 0; e < edits; ++e) {
            uint64_t at = rnd() % s.size();
            if (rnd() & 1) at = where[rnd() % 12] + rnd() % 8;
            s[size_t(at)] = (rnd() & 3) ? uint8_t(rnd()) : uint8_t(rnd() % 4);
        }
        if (rnd() % 4 == 0) s.resize(size_t(rnd() % (s.size() + 1)));
        check(s);
    }

    check_writer();
    std::printf("%" PRIu64 " accepted, %" PRIu64 " rejected, %" PRIu64 " truncations, %" PRIu64 " counts, writer ok\n", n_accept,
                n_reject, uint64_t(base.size() + 1), n_counts);
    return 0;
}
