// CPU safety net of Decode's gzip / DEFLATE walker (plakar_amd/csrc/
// inflate_walk.h, the header the device kernels take every bound from), built
// with
//   g++ -fsanitize=address,undefined
// and linked with the system's zlib only.  Every input is copied into a heap
// buffer of exactly its size and decoded into a heap buffer of exactly the
// size that was planned for it (a raw body: what a counting walk reported; a
// member: its ISIZE claim, as k_gz_size plans it), so one byte read or written
// out of range is a sanitizer report.  The walker must never accept what zlib
// rejects, and where both accept, the bytes are equal.
//
//   inflate_host_fuzz [--mutations N] [--streams FILE]...
//
// Built-in fixtures (made here with zlib from a fixed seed): raw DEFLATE
// bodies of 0.8-20 KB of text-like, mixed and random content, written with
// dynamic codes (levels 1, 6, 9), the fixed code (Z_FIXED), stored blocks
// (level 0), Z_RLE and Z_HUFFMAN_ONLY.  Then N (default 20,000) single-bit
// mutations of them.  A --streams file holds gzip members, each as a
// little-endian u32 length and the bytes (the test suite passes every stream
// its GPU tests use); each is walked as the device walks it (claim, inflate
// into the claim, CRC-32 by 64 slices, trailer) and reported on a line
//   S <index> <status> <size> <crc32 of the output>
// for the test to hold against its Python restatement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../plakar_amd/csrc/inflate_walk.h"

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
int inflateInit2_(z_stream *, int, const char *, int);
int inflate(z_stream *, int);
int inflateEnd(z_stream *);
int deflateInit2_(z_stream *, int, int, int, int, int, const char *, int);
int deflate(z_stream *, int);
int deflateEnd(z_stream *);
unsigned long deflateBound(z_stream *, unsigned long);
unsigned long crc32(unsigned long, const unsigned char *, unsigned);
}
#define Z_FINISH 4
#define Z_STREAM_END 1
#define Z_OK 0
#define Z_DEFLATED 8
#define Z_HUFFMAN_ONLY 2
#define Z_RLE 3
#define Z_FIXED 4
#define Z_DEFAULT_STRATEGY 0
#define inflateInit2(s, w) inflateInit2_((s), (w), zlibVersion(), int(sizeof(z_stream)))
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

static infw::Tables g_fixed;
static uint32_t g_crc_table[256];
static unsigned long g_accepted, g_rejected;

// zlib's verdict: window bits -15 (raw) or 31 (gzip).  True and `out` when the
// stream ends properly inside the input; used: the input bytes it took.
static bool zlib_inflate(const uint8_t *src, size_t n, int wbits, Bytes &out, size_t &used)
{
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, wbits) != Z_OK) exit(2);
    out.assign(1 << 16, 0);
    z.next_in = const_cast<unsigned char *>(src);
    z.avail_in = unsigned(n);
    int r;
    for (;;) {
        z.next_out = out.data() + z.total_out;
        z.avail_out = unsigned(out.size() - z.total_out);
        r = inflate(&z, Z_FINISH);
        if (r == Z_STREAM_END) break;
        if (z.avail_out != 0 || out.size() > (64u << 20)) break;  // an error, or the input ended
        out.resize(out.size() * 2);
    }
    out.resize(z.total_out);
    used = z.total_in;
    inflateEnd(&z);
    return r == Z_STREAM_END;
}

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

// The CRC-32 as k_gz_emit's wave computes it: 64 slices, then six folds.
static uint32_t crc_by_slices(const uint8_t *p, uint64_t n)
{
    if (n == 0) return 0;
    uint32_t reg[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
        uint64_t lo, hi;
        infw::crc_slice(n, lane, lo, hi, reg[lane]);
        for (uint64_t i = lo; i < hi; ++i) reg[lane] = g_crc_table[(reg[lane] ^ p[i]) & 255u] ^ (reg[lane] >> 8);
    }
    uint32_t M = infw::crc_xpow(8u * infw::crc_slice_len(n));
    for (uint32_t d = 1; d < 64; d <<= 1) {
        for (uint32_t lane = 0; lane + d < 64; lane += 2 * d) reg[lane] = infw::crc_mul(reg[lane], M) ^ reg[lane + d];
        M = infw::crc_mul(M, M);
    }
    return reg[0] ^ 0xFFFFFFFFu;
}

// A raw DEFLATE body.  0: fine; 1: a wrong acceptance.
static int check_raw(const Bytes &in, const char *what)
{
    const uint32_t n = uint32_t(in.size());
    uint8_t *src = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(src, in.data(), n);
    PtrRd rd{src};
    infw::Serial par;
    infw::Tables *dyn = new infw::Tables;
    infw::CountSink cs;
    uint32_t size = 0, end = 0;
    int bad = 0;
    const int st = infw::inflate_body(rd, n, 0, cs, 1u << 28, *dyn, g_fixed, par, size, end);
    if (st != infw::kOk) {
        ++g_rejected;
    } else {
        ++g_accepted;
        uint8_t *out = static_cast<uint8_t *>(malloc(size ? size : 1));
        infw::MemSink<PtrRd> ms{out, rd};
        uint32_t again = 0, end2 = 0;
        const int st2 = infw::inflate_body(rd, n, 0, ms, size, *dyn, g_fixed, par, again, end2);
        Bytes ref;
        size_t used = 0;
        const bool zok = zlib_inflate(src, n, -15, ref, used);
        const bool same = st2 == infw::kOk && again == size && end2 == end && zok && used == end && ref.size() == size &&
                          memcmp(out, ref.data(), size) == 0;
        if (!same) {
            fprintf(stderr, "%s: accepted %u bytes as %u (emit %d, %u), zlib says %d, %zu bytes, used %zu of %u\n", what, n,
                    size, st2, again, int(zok), ref.size(), used, end);
            bad = 1;
        }
        free(out);
    }
    delete dyn;
    free(src);
    return bad;
}

// A gzip member, as the device walks it.  status: 0, -13 (corrupt), -2
// (unsupported); out: the bytes when 0.
static int walk_member(const Bytes &in, Bytes &res)
{
    const uint32_t n = uint32_t(in.size());
    uint8_t *src = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(src, in.data(), n);
    PtrRd rd{src};
    res.clear();
    uint32_t hlen = 0, claim = 0;
    int st = infw::member_claim(rd, n, hlen, claim);
    if (st == infw::kOk && n) {
        uint8_t *out = static_cast<uint8_t *>(malloc(claim ? claim : 1));
        infw::MemSink<PtrRd> ms{out, rd};
        infw::Serial par;
        infw::Tables *dyn = new infw::Tables;
        uint32_t opos = 0, end = 0, h2 = 0;
        st = infw::member_header(rd, n, h2);
        if (st == infw::kOk) st = infw::inflate_body(rd, n, h2, ms, claim, *dyn, g_fixed, par, opos, end);
        if (st == infw::kOk) st = infw::member_trailer(rd, n, end, opos, crc_by_slices(out, opos));
        if (st == infw::kOk && opos != claim) st = infw::kCorrupt;
        if (st == infw::kOk) res.assign(out, out + opos);
        delete dyn;
        free(out);
    }
    free(src);
    return st == infw::kOk ? 0 : st == infw::kUnsupported ? -2 : -13;
}

static Bytes content(uint32_t n, int kind)
{
    static const char *words[] = {"plakar", "snapshot", "chunk", "the", "of", "packfile", "restore", "a", "device", "blob"};
    Bytes c;
    while (c.size() < n) {
        const int k = kind == 2 ? int(rnd() % 3) : kind;
        if (k == 0) {  // text-like
            const char *w = words[rnd() % 10];
            c.insert(c.end(), w, w + strlen(w));
            c.push_back(' ');
        } else if (k == 1) {  // random
            for (int i = 0; i < 64; ++i) c.push_back(uint8_t(rnd()));
        } else {  // a run
            c.insert(c.end(), 1 + rnd() % 300, uint8_t(rnd() % 4));
        }
    }
    c.resize(n);
    return c;
}

int main(int argc, char **argv)
{
    unsigned long mutations = 20000;
    std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--mutations") && i + 1 < argc) mutations = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--streams") && i + 1 < argc) files.push_back(argv[++i]);
        else {
            fprintf(stderr, "usage: %s [--mutations N] [--streams FILE]...\n", argv[0]);
            return 2;
        }
    }
    infw::Serial par;
    infw::build_fixed(par, g_fixed);
    for (uint32_t i = 0; i < 256; ++i) g_crc_table[i] = infw::crc_bits(0, i);
    int bad = 0;
    {  // the sliced CRC-32 against zlib's, over the lengths where slices change shape
        Bytes c = content(70000, 1);
        for (uint32_t n = 0; n <= 70000 && !bad; n += (n < 700 ? 1 : 977)) {
            if (crc_by_slices(c.data(), n) != uint32_t(crc32(0, c.data(), n))) {
                fprintf(stderr, "crc_by_slices differs from zlib at %u bytes\n", n);
                bad = 1;
            }
        }
    }
    std::vector<Bytes> bodies, contents;
    struct Spec {
        uint32_t n;
        int kind, level, strategy;
    };
    const Spec specs[] = {
        {800, 0, 6, Z_DEFAULT_STRATEGY},   {4000, 0, 9, Z_DEFAULT_STRATEGY}, {20000, 2, 6, Z_DEFAULT_STRATEGY},
        {9000, 2, 1, Z_DEFAULT_STRATEGY},  {3000, 0, 6, Z_FIXED},            {12000, 2, 6, Z_FIXED},
        {1500, 2, 0, Z_DEFAULT_STRATEGY},  {5000, 2, 6, Z_RLE},              {2500, 0, 6, Z_HUFFMAN_ONLY},
        {6000, 1, 6, Z_DEFAULT_STRATEGY},
    };
    for (const Spec &s : specs) {
        contents.push_back(content(s.n, s.kind));
        bodies.push_back(zlib_deflate(contents.back(), s.level, s.strategy));
    }
    {  // random bytes (they end up stored), then text
        Bytes c = content(1500, 1), t = content(3000, 0);
        c.insert(c.end(), t.begin(), t.end());
        contents.push_back(c);
        bodies.push_back(zlib_deflate(c, 6, Z_DEFAULT_STRATEGY));
    }
    for (size_t i = 0; i < bodies.size(); ++i) {
        const unsigned long before = g_accepted;
        bad |= check_raw(bodies[i], "fixture");
        if (g_accepted == before) {
            fprintf(stderr, "fixture %zu was rejected\n", i);
            bad = 1;
        }
    }
    for (unsigned long k = 0; k < mutations && !bad; ++k) {
        const size_t f = k % bodies.size();
        Bytes m = bodies[f];
        // half of the flips land in the first 64 bytes, where the block header and the code lengths are
        const size_t at = (rnd() & 1) ? rnd() % (m.size() < 64 ? m.size() : 64) : rnd() % m.size();
        m[at] ^= uint8_t(1u << (rnd() % 8));
        bad |= check_raw(m, "mutation");
    }
    for (const std::string &path : files) {
        FILE *fp = fopen(path.c_str(), "rb");
        if (!fp) {
            fprintf(stderr, "cannot open %s\n", path.c_str());
            return 2;
        }
        uint8_t h[4];
        unsigned long idx = 0;
        while (fread(h, 1, 4, fp) == 4) {
            const uint32_t n = uint32_t(h[0]) | uint32_t(h[1]) << 8 | uint32_t(h[2]) << 16 | uint32_t(h[3]) << 24;
            Bytes b(n), out;
            if (n && fread(b.data(), 1, n, fp) != n) {
                fprintf(stderr, "%s: short record\n", path.c_str());
                fclose(fp);
                return 2;
            }
            const int st = walk_member(b, out);
            if (st == 0 && n) {
                Bytes ref;
                size_t used = 0;
                if (!zlib_inflate(b.data(), n, 31, ref, used) || used != n || ref != out) {
                    fprintf(stderr, "%s: stream %lu accepted, zlib does not agree\n", path.c_str(), idx);
                    bad = 1;
                }
            }
            printf("S %lu %d %zu %08x\n", idx, st, out.size(), unsigned(crc32(0, out.data(), unsigned(out.size()))));
            ++idx;
        }
        fclose(fp);
    }
    printf("inflate_host_fuzz: %lu accepted, %lu rejected, %s\n", g_accepted, g_rejected, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
