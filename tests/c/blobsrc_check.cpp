// Stand-alone checker of the readers' host-only layer (cdc_blobsrc.h,
// cdc_hostutil.h), built by tests/test_blobsrc_cpu.py with
// -fsanitize=address,undefined together with cdc_blobsrc.cpp and the
// library's host SHA-256 (cdc_sha256.cpp).
//
//   * gather: packfiles serialised here (the layout restore_plan.h reads),
//     registered from memory and by path in turn; seeded random span lists
//     with empty spans, clipped spans and repeated packfiles land byte for
//     byte where a plain loop puts them, in a heap arena of exactly the total,
//     at 1, 2 and 8 threads;
//   * lost files: one by-path packfile deleted and one cut short after
//     registration give CDC_E_IO for exactly their blobs, every other blob's
//     bytes intact;
//   * descriptors: as many entries under /proc/self/fd after every gather as
//     before it, a skipped read (no arena) included;
//   * resolve: -1 for a full match and for no chunks, else the first miss;
//   * Handoff: a waiter returns true once its counter is reached, an abort
//     wakes a blocked waiter with false, the first abort's status stays.
//
// Prints "<g> gathers, <l> lost blobs, <r> resolves, handoff ok, ok" and exits
// 0, or says what failed and exits 1.
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <thread>
#include <vector>

#include "cdc_blobsrc.h"
#include "cdc_hostutil.h"
#include "restore_plan.h"

static uint64_t g_seed = 0x243F6A8885A308D3ull;
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

static void put32(std::vector<uint8_t> &v, uint32_t x)
{
    for (int i = 0; i < 4; ++i) v.push_back(uint8_t(x >> (8 * i)));
}
static void put64(std::vector<uint8_t> &v, uint64_t x)
{
    for (int i = 0; i < 8; ++i) v.push_back(uint8_t(x >> (8 * i)));
}

// A packfile of `count` rows: random data, then the index rows (type,
// checksum, offset, length), then the footer over the index's SHA-256.
static std::vector<uint8_t> make_packfile(uint32_t count)
{
    std::vector<uint8_t> idx, out;
    for (uint32_t r = 0; r < count; ++r) {
        const uint32_t len = below(5) == 0 ? 0 : uint32_t(1 + below(3000));
        idx.push_back(below(8) == 0 ? uint8_t(rplan::kTypeChunk + 1) : uint8_t(rplan::kTypeChunk));
        for (int i = 0; i < 32; ++i) idx.push_back(uint8_t(rnd()));
        put32(idx, uint32_t(out.size()));
        put32(idx, len);
        for (uint32_t i = 0; i < len; ++i) out.push_back(uint8_t(rnd()));
    }
    const uint32_t data_len = uint32_t(out.size());
    uint8_t h[32];
    cdc::sha256(idx.data(), idx.size(), h);
    out.insert(out.end(), idx.begin(), idx.end());
    put32(out, 100);
    put64(out, 11);
    put32(out, count);
    put32(out, data_len);
    out.insert(out.end(), h, h + 32);
    return out;
}

static int open_fds()
{
    DIR *d = opendir("/proc/self/fd");
    CHECK(d, "opendir /proc/self/fd");
    int n = 0;
    while (readdir(d)) ++n;
    closedir(d);
    return n;
}

struct Gathered {
    std::vector<uint64_t> eoff, elen;
    std::vector<int32_t> pre;
    uint64_t total;
    uint8_t *arena;  // exactly `total` bytes on the heap: a byte past it is a sanitizer report
};

static Gathered gather(const cdc::Locator &loc, const std::vector<cdc::Span> &spans, int threads, bool skip)
{
    Gathered G;
    G.total = cdc::lay_out(spans.data(), spans.size(), G.eoff, G.elen);
    G.pre.assign(spans.size(), 77);
    G.arena = skip ? nullptr : static_cast<uint8_t *>(malloc(G.total ? G.total : 1));
    if (G.arena) memset(G.arena, 0xEE, G.total);
    const int before = open_fds();
    cdc::read_spans(loc, spans.data(), spans.size(), G.eoff.data(), G.arena, threads, G.pre.data());
    CHECK(open_fds() == before, "a gather of %zu spans left descriptors open", spans.size());
    return G;
}

int main()
{
    char dir[] = "/tmp/blobsrc_check.XXXXXX";
    CHECK(mkdtemp(dir), "mkdtemp");
    const int kPacks = 7;
    std::vector<std::vector<uint8_t>> bytes;
    std::vector<std::string> paths(kPacks);
    cdc::Locator loc;
    for (int p = 0; p < kPacks; ++p) {
        bytes.push_back(make_packfile(uint32_t(5 + below(60))));
        if (p % 2 == 0) {
            CHECK(loc.add_memory(bytes[p].data(), bytes[p].size()) == CDC_OK, "add_memory %d", p);
        } else {
            paths[p] = std::string(dir) + "/pack" + std::to_string(p);
            FILE *f = fopen(paths[p].c_str(), "wb");
            CHECK(f && fwrite(bytes[p].data(), 1, bytes[p].size(), f) == bytes[p].size() && fclose(f) == 0, "write %d", p);
            CHECK(loc.add_path(paths[p].c_str()) == CDC_OK, "add_path %d", p);
        }
    }
    const uint32_t nblobs = uint32_t(loc.locs.size());
    CHECK(nblobs > 50 && loc.packs.size() == size_t(kPacks), "%u blobs", nblobs);

    // ---- gathers against a plain loop
    int gathers = 0;
    for (int trial = 0; trial < 150; ++trial) {
        std::vector<cdc::Span> spans(below(90));
        const uint32_t only = below(4) == 0 ? uint32_t(below(kPacks)) : ~0u;  // sometimes one packfile over and over
        for (cdc::Span &S : spans) {
            do S = cdc::span_of(loc, uint32_t(below(nblobs)));
            while (only != ~0u && S.pack != only && below(50));
            if (below(6) == 0) S.length = below(S.length + 1);  // clipped, as a prefix read's
        }
        std::vector<uint8_t> want;
        for (const cdc::Span &S : spans)
            want.insert(want.end(), bytes[S.pack].begin() + S.offset, bytes[S.pack].begin() + S.offset + S.length);
        for (int threads : {1, 2, 8}) {
            Gathered G = gather(loc, spans, threads, false);
            CHECK(G.total == want.size(), "trial %d: total %llu", trial, (unsigned long long)G.total);
            for (size_t b = 0; b < spans.size(); ++b)
                CHECK(G.pre[b] == CDC_OK && G.elen[b] == spans[b].length && (b == 0 || G.eoff[b] == G.eoff[b - 1] + G.elen[b - 1]),
                      "trial %d span %zu", trial, b);
            CHECK(want.empty() || memcmp(G.arena, want.data(), want.size()) == 0, "trial %d, %d threads: bytes differ", trial, threads);
            free(G.arena);
            ++gathers;
        }
        Gathered G = gather(loc, spans, 4, true);  // the caller found no room: nothing is read, nothing stays open
        for (size_t b = 0; b < spans.size(); ++b) CHECK(G.pre[b] == CDC_OK, "skipped read, span %zu", b);
        ++gathers;
    }

    // ---- one by-path packfile deleted, one cut short
    const uint32_t gone = 1, cut_pack = 3;
    std::vector<uint64_t> ends;
    for (const cdc::Locator::Loc &L : loc.locs)
        if (L.pack == cut_pack && L.length) ends.push_back(uint64_t(L.offset) + L.length);
    CHECK(ends.size() > 2, "packfile %u has blobs", cut_pack);
    const uint64_t cut = ends[ends.size() / 2] - 1;  // inside a blob
    CHECK(unlink(paths[gone].c_str()) == 0 && truncate(paths[cut_pack].c_str(), off_t(cut)) == 0, "unlink, truncate");
    int lost = 0;
    for (int threads : {1, 2, 8}) {
        std::vector<cdc::Span> spans;
        for (uint32_t id = 0; id < nblobs; ++id) spans.push_back(cdc::span_of(loc, id));
        for (size_t i = spans.size(); i > 1; --i) std::swap(spans[i - 1], spans[below(i)]);
        Gathered G = gather(loc, spans, threads, false);
        for (size_t b = 0; b < spans.size(); ++b) {
            const cdc::Span &S = spans[b];
            const bool bad = S.pack == gone || (S.pack == cut_pack && S.length && S.offset + S.length > cut);
            CHECK(G.pre[b] == (bad ? CDC_E_IO : CDC_OK), "%d threads: span %zu of packfile %u has status %d", threads, b, S.pack,
                  G.pre[b]);
            if (!bad)
                CHECK(!S.length || memcmp(G.arena + G.eoff[b], bytes[S.pack].data() + S.offset, S.length) == 0, "span %zu: bytes differ", b);
            lost += bad;
        }
        free(G.arena);
        ++gathers;
    }
    CHECK(lost > 10, "%d lost blobs", lost);

    // ---- resolve
    int resolves = 0;
    for (int trial = 0; trial < 300; ++trial) {
        const uint64_t n = below(40);
        std::vector<uint8_t> sums(n * 32 + 1);
        std::vector<uint32_t> want(n), ids(n + 1, 0xABABABABu);
        for (uint64_t c = 0; c < n; ++c) {
            want[c] = uint32_t(below(nblobs));
            memcpy(&sums[c * 32], loc.sums[want[c]].b, 32);
        }
        CHECK(cdc::resolve(loc, sums.data(), n, ids.data()) == -1, "trial %d: a full match", trial);
        CHECK((n == 0 || memcmp(ids.data(), want.data(), n * 4) == 0) && ids[n] == 0xABABABABu, "trial %d: ids", trial);
        if (n) {
            const uint64_t first = below(n), second = first + below(n - first);
            sums[first * 32 + 5] ^= 0x40;
            sums[second * 32 + 9] ^= 0x01;
            CHECK(cdc::resolve(loc, sums.data(), n, ids.data()) == int64_t(first), "trial %d: the first miss", trial);
        }
        ++resolves;
    }
    CHECK(cdc::resolve(loc, nullptr, 0, nullptr) == -1, "no chunks");

    // ---- Handoff
    {
        cdc::Handoff H;
        int counter = 0;
        bool got = false;
        std::thread waiter([&] { got = H.wait_for(counter, 2); });
        H.advance(counter);
        H.advance(counter);
        waiter.join();
        CHECK(got && counter == 2 && !H.failed(), "a waiter returns true once the counter is reached");
        bool got2 = true;
        std::thread blocked([&] { got2 = H.wait_for(counter, 100); });
        H.abort_run(-5);
        H.abort_run(-7);
        blocked.join();
        CHECK(!got2 && H.failed() && H.fail == -5, "an abort wakes the waiter, the first status stays: %d", H.fail);
        CHECK(!H.wait_for(counter, 0), "a failed run ends every wait");
    }

    for (const std::string &p : paths)
        if (!p.empty()) unlink(p.c_str());
    rmdir(dir);
    printf("%d gathers, %d lost blobs, %d resolves, handoff ok, ok\n", gathers, lost, resolves);
    return 0;
}
