// CPU safety net of prefix Decode's stop mode (lz4w::next_seq_stop in
// plakar_amd/csrc/lz4_walk.h, infw::inflate_body_stop in inflate_walk.h: the
// headers the prefix kernels take every bound from), built with
//   g++ -fsanitize=address,undefined
// and linked with the system's zlib only.  Every stream is copied into a heap
// buffer of exactly its size and every prefix is decoded into a heap buffer of
// exactly `cut` bytes, so one byte read or written out of range is a sanitizer
// report.
//
//   prefix_host_fuzz [--blocks FILE]...
//
// Streams of a few KiB: raw DEFLATE bodies made here with zlib (dynamic codes
// at levels 1, 6 and 9, the fixed code, stored blocks, Z_RLE) and LZ4 blocks
// made here by a small greedy writer, over text-like, zero, random and mixed
// content; a --blocks file adds LZ4 blocks, each as a little-endian u32 length
// and the bytes (the test suite passes the blocks its GPU tests decode).
// For every stream, every cut from 0 to the decoded length (blocks over 8 KiB:
// 300 cuts at each end and a seeded sample):
//   - the stop walk answers ok with exactly `cut` bytes, equal to the full
//     output's prefix; stopped is true below the length and false at it, where
//     the walk has also found the stream's end as the full walk does;
//   - the same over the stream cut short (its last byte, its second half, all
//     but a quarter): either a fault, or again exactly the right prefix.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../plakar_amd/csrc/inflate_walk.h"
#include "../../plakar_amd/csrc/lz4_walk.h"

#if __has_include(<zlib.h>)
#include <zlib.h>
#else
extern "C" {  // zlib's ABI (1.2.x, LP64) where its header is not installed
typedef struct z_stream_s {
    const unsigned char *next_in;
    unsigned avail_in;
    unsigned long total_in;
    unsigned char *next_out;
    unsigned avail_out;
    unsigned long total_out;
    const char *msg;
    void *state, *zalloc, *zfree, *opaque;
    int data_type;
    unsigned long adler, reserved;
} z_stream;
const char *zlibVersion(void);
int deflateInit2_(z_stream *, int, int, int, int, int, const char *, int);
int deflate(z_stream *, int);
int deflateEnd(z_stream *);
unsigned long deflateBound(z_stream *, unsigned long);
}
#define Z_FINISH 4
#define Z_STREAM_END 1
#define Z_OK 0
#define Z_DEFLATED 8
#define Z_RLE 3
#define Z_FIXED 4
#define Z_DEFAULT_STRATEGY 0
#define deflateInit2(s, l, m, w, ml, st) deflateInit2_((s), (l), (m), (w), (ml), (st), zlibVersion(), int(sizeof(z_stream)))
#endif

typedef std::vector<uint8_t> Bytes;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 16);
}

struct PtrRd {
    const uint8_t *p;
    uint32_t operator()(uint32_t i) const { return p[i]; }
};

// A heap block of exactly n bytes, a copy of p[0, n) when p is given (the
// sanitizer guards a zero-sized block too).
static std::unique_ptr<uint8_t[]> exact(const uint8_t *p, size_t n)
{
    std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
    if (n && p) memcpy(b.get(), p, n);
    return b;
}

static unsigned long g_cuts, g_short_ok, g_short_bad;
static int g_bad;

static void fail(const char *what, const char *name, size_t cut)
{
    fprintf(stderr, "FAIL %s: %s at cut %zu\n", name, what, cut);
    ++g_bad;
}

// ---- content ---------------------------------------------------------------------------
static Bytes content(int kind, size_t n)
{
    Bytes b(n);
    static const char *words[] = {"restore ", "snapshot ", "chunk ", "packfile ", "the ", "of ", "range ", "\n"};
    if (kind == 0) {  // text-like: the cuts fall inside matches
        size_t i = 0;
        while (i < n) {
            const char *w = words[rnd() % 8];
            for (; *w && i < n; ++w) b[i++] = uint8_t(*w);
        }
    } else if (kind == 1) {  // zeros: one distance-1 match runs through every cut
        memset(b.data(), 0, n);
    } else if (kind == 2) {  // random: literals, stored blocks
        for (size_t i = 0; i < n; ++i) b[i] = uint8_t(rnd());
    } else {  // a mix of the three
        size_t i = 0;
        while (i < n) {
            const size_t m = 1 + rnd() % 600;
            const Bytes part = content(int(rnd() % 3), m);
            for (size_t k = 0; k < m && i < n; ++k) b[i++] = part[k];
        }
    }
    return b;
}

// ---- DEFLATE ---------------------------------------------------------------------------
static Bytes zlib_deflate(const Bytes &in, int level, int strategy)
{
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) exit(2);
    Bytes out(deflateBound(&z, in.size()) + 16);
    z.next_in = const_cast<unsigned char *>(in.data());
    z.avail_in = unsigned(in.size());
    z.next_out = out.data();
    z.avail_out = unsigned(out.size());
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) exit(2);
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

static infw::Tables g_fixed, g_dyn;

// The stop walk of in[0, t) for `cut` bytes into a buffer of exactly `cut`.
// whole: t is the stream's own length, so the answer is known.
static void deflate_cut(const char *name, const Bytes &in, size_t t, const Bytes &want, size_t cut, bool whole)
{
    auto src = exact(in.data(), t);
    auto dst = exact(nullptr, cut);
    PtrRd rd{src.get()};
    infw::MemSink<PtrRd> sink{dst.get(), rd};
    infw::Serial par;
    uint32_t opos = 0, end = 0;
    bool stopped = false;
    const int st = infw::inflate_body_stop(rd, uint32_t(t), 0, sink, uint32_t(cut), g_dyn, g_fixed, par, opos, end, stopped);
    ++g_cuts;
    if (!whole && st != infw::kOk) {
        ++g_short_bad;
        return;
    }
    if (!whole) ++g_short_ok;
    if (st != infw::kOk) return fail("the stop walk refused a good stream", name, cut);
    // (what is left of a stream cut short may itself end properly, before the cut)
    if (whole || stopped ? opos != cut : opos > cut) return fail("not exactly the bytes asked for", name, cut);
    if (opos && memcmp(dst.get(), want.data(), opos)) return fail("the prefix differs", name, cut);
    if (whole && stopped != (cut < want.size())) return fail("stopped is wrong", name, cut);
    if (whole && !stopped && end != t) return fail("the stream's end is wrong", name, cut);
}

static void deflate_stream(const char *name, const Bytes &plain, int level, int strategy)
{
    const Bytes z = zlib_deflate(plain, level, strategy);
    {  // the full walk first: the stop mode is held against it
        auto src = exact(z.data(), z.size());
        auto dst = exact(nullptr, plain.size());
        PtrRd rd{src.get()};
        infw::MemSink<PtrRd> sink{dst.get(), rd};
        infw::Serial par;
        uint32_t opos = 0, end = 0;
        if (infw::inflate_body(rd, uint32_t(z.size()), 0, sink, uint32_t(plain.size()), g_dyn, g_fixed, par, opos,
                               end) != infw::kOk ||
            opos != plain.size() || memcmp(dst.get(), plain.data(), plain.size()))
            return fail("the full walk", name, 0);
    }
    for (size_t cut = 0; cut <= plain.size(); ++cut) deflate_cut(name, z, z.size(), plain, cut, true);
    // one byte past what the stream holds: everything is out, then the end, not stopped
    {
        auto src = exact(z.data(), z.size());
        auto dst = exact(nullptr, plain.size() + 1);
        PtrRd rd{src.get()};
        infw::MemSink<PtrRd> sink{dst.get(), rd};
        infw::Serial par;
        uint32_t opos = 0, end = 0;
        bool stopped = true;
        if (infw::inflate_body_stop(rd, uint32_t(z.size()), 0, sink, uint32_t(plain.size() + 1), g_dyn, g_fixed, par,
                                    opos, end, stopped) != infw::kOk ||
            stopped || opos != plain.size())
            fail("a stream shorter than the cut", name, plain.size() + 1);
    }
    const size_t shorts[3] = {z.size() - 1, z.size() / 2, z.size() / 4};
    for (size_t t : shorts) {
        const unsigned long ok0 = g_short_ok;
        for (size_t cut = 0; cut < plain.size(); cut += (cut < 600 ? 1 : 7)) deflate_cut(name, z, t, plain, cut, false);
        if (g_short_ok == ok0) fail("no prefix at all of a stream cut short (cut 0 reads nothing)", name, t);
    }
}

// ---- LZ4 -------------------------------------------------------------------------------
// A greedy block writer (4-byte hash, one candidate), within the format's end
// rules: the last match starts 12 bytes before the end at the latest and the
// last 5 bytes are literals.
static void put_len(Bytes &o, size_t v)
{
    for (; v >= 255; v -= 255) o.push_back(255);
    o.push_back(uint8_t(v));
}

static Bytes lz4_block(const Bytes &in)
{
    Bytes o;
    const size_t n = in.size();
    std::vector<int64_t> head(1 << 12, -1);
    size_t anchor = 0, i = 0;
    auto emit = [&](size_t lit, size_t off, size_t ml) {
        const size_t mcode = ml ? ml - 4 : 0;
        o.push_back(uint8_t((lit >= 15 ? 15 : lit) << 4 | (ml ? (mcode >= 15 ? 15 : mcode) : 0)));
        if (lit >= 15) put_len(o, lit - 15);
        o.insert(o.end(), in.begin() + long(anchor), in.begin() + long(anchor + lit));
        if (ml) {
            o.push_back(uint8_t(off));
            o.push_back(uint8_t(off >> 8));
            if (mcode >= 15) put_len(o, mcode - 15);
        }
    };
    while (n >= 13 && i + 12 <= n) {
        uint32_t w;
        memcpy(&w, &in[i], 4);
        const uint32_t h = (w * 2654435761u) >> 20;
        const int64_t c = head[h];
        head[h] = int64_t(i);
        if (c >= 0 && i - size_t(c) <= 65535 && !memcmp(&in[size_t(c)], &in[i], 4)) {
            size_t ml = 4;
            while (i + ml < n - 5 && in[size_t(c) + ml] == in[i + ml]) ++ml;
            emit(i - anchor, i - size_t(c), ml);
            i += ml;
            anchor = i;
        } else {
            ++i;
        }
    }
    emit(n - anchor, 0, 0);
    return o;
}

static void lz4_cut(const char *name, const Bytes &in, size_t t, const Bytes &want, size_t cut, bool whole)
{
    auto src = exact(in.data(), t);
    auto dst = exact(nullptr, cut);
    PtrRd rd{src.get()};
    bool stopped = false;
    const int64_t d = lz4w::decode_block_stop(rd, uint32_t(t), dst.get(), uint32_t(want.size()), uint32_t(cut), stopped);
    ++g_cuts;
    if (!whole && d < 0) {
        ++g_short_bad;
        return;
    }
    if (!whole) ++g_short_ok;
    if (d < 0) return fail("the stop walk refused a good block", name, cut);
    // (what is left of a block cut short may itself be a block that ends before the cut)
    if (whole || stopped ? size_t(d) != cut : size_t(d) > cut) return fail("not exactly the bytes asked for", name, cut);
    if (d && memcmp(dst.get(), want.data(), size_t(d))) return fail("the prefix differs", name, cut);
    if (whole && stopped != (cut < want.size())) return fail("stopped is wrong", name, cut);
}

static void lz4_stream(const char *name, const Bytes &blk)
{
    Bytes plain;
    {
        auto src = exact(blk.data(), blk.size());
        PtrRd rd{src.get()};
        const int64_t size = lz4w::decode_block(rd, uint32_t(blk.size()), static_cast<uint8_t *>(nullptr), 4u << 20);
        if (size < 0) return;  // not a good block: the full walk's own tests cover those
        plain.resize(size_t(size));
        auto dst = exact(nullptr, plain.size());
        if (lz4w::decode_block(rd, uint32_t(blk.size()), dst.get(), uint32_t(size)) != size)
            return fail("the full walk", name, 0);
        if (size) memcpy(plain.data(), dst.get(), plain.size());
    }
    const size_t n = plain.size();
    if (n <= 8192) {
        for (size_t cut = 0; cut <= n; ++cut) lz4_cut(name, blk, blk.size(), plain, cut, true);
    } else {
        for (size_t cut = 0; cut <= 300; ++cut) lz4_cut(name, blk, blk.size(), plain, cut, true);
        for (size_t cut = n - 300; cut <= n; ++cut) lz4_cut(name, blk, blk.size(), plain, cut, true);
        for (int k = 0; k < 100; ++k) lz4_cut(name, blk, blk.size(), plain, rnd() % (n + 1), true);
    }
    if (blk.size() < 2) return;
    const size_t shorts[3] = {blk.size() - 1, blk.size() / 2, blk.size() / 4};
    for (size_t t : shorts) {
        const unsigned long ok0 = g_short_ok;
        const size_t step = n > 8192 ? 997 : 7;
        for (size_t cut = 0; cut < n; cut += (cut < (n > 8192 ? 64 : 600) ? 1 : step)) lz4_cut(name, blk, t, plain, cut, false);
        if (g_short_ok == ok0) fail("no prefix at all of a block cut short (cut 0 reads nothing)", name, t);
    }
}

static void load_blocks(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    uint32_t len;
    int k = 0;
    while (fread(&len, 4, 1, f) == 1) {
        Bytes b(len);
        if (len && fread(b.data(), 1, len, f) != len) exit(2);
        char name[64];
        snprintf(name, sizeof(name), "file block %d", k++);
        lz4_stream(name, b);
    }
    fclose(f);
}

int main(int argc, char **argv)
{
    infw::Serial par;
    infw::build_fixed(par, g_fixed);
    static const char *kinds[4] = {"text", "zeros", "random", "mix"};
    static const size_t sizes[3] = {1, 777, 3100};
    for (int kind = 0; kind < 4; ++kind)
        for (size_t n : sizes) {
            const Bytes plain = content(kind, n);
            char name[96];
            const struct { int level, strategy; const char *what; } modes[6] = {
                {1, Z_DEFAULT_STRATEGY, "level 1"}, {6, Z_DEFAULT_STRATEGY, "level 6"}, {9, Z_DEFAULT_STRATEGY, "level 9"},
                {6, Z_FIXED, "fixed"},              {0, Z_DEFAULT_STRATEGY, "stored"},  {6, Z_RLE, "rle"}};
            for (const auto &m : modes) {
                snprintf(name, sizeof(name), "deflate %s %zu %s", kinds[kind], n, m.what);
                deflate_stream(name, plain, m.level, m.strategy);
            }
            snprintf(name, sizeof(name), "lz4 %s %zu", kinds[kind], n);
            lz4_stream(name, lz4_block(plain));
        }
    {  // literal and match lengths that take extension bytes, the cut inside them
        Bytes p = content(2, 400);
        p.resize(1500, 0x5A);
        const Bytes tail = content(0, 300);
        p.insert(p.end(), tail.begin(), tail.end());
        lz4_stream("lz4 long runs", lz4_block(p));
    }
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--blocks") && i + 1 < argc) load_blocks(argv[++i]);
    printf("prefix_host_fuzz: %lu cuts, %lu short ok, %lu short refused, %s\n", g_cuts, g_short_ok, g_short_bad,
           g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
