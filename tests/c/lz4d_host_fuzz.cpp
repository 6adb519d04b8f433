// CPU safety net of Decode's LZ4 block walker (plakar_amd/csrc/lz4_walk.h, the
// header the device kernels take every bound from), built with
//   g++ -fsanitize=address,undefined
// and linked with the system's liblz4 only.  Every input is copied into a heap
// buffer of exactly its size and decoded into a heap buffer of exactly the
// size the walker's sizing pass reported, so one byte read or written out of
// range is a sanitizer report.  Whenever the walker accepts an input, its
// output must equal LZ4_decompress_safe's, or the content the input was made
// from.
//
//   lz4d_host_fuzz [--mutations N] [--blocks FILE]...
//
// Built-in fixtures (made here from a fixed seed): a 68,640-byte block with a
// 40,960-byte literal run, a 20,480-byte match at offset 40,960 and the
// overlapping matches (offset 1, 4,999) and (offset 3, 2,097); a match at
// offset 65,535; hand-made blocks whose length extensions end in a 0 byte or
// take a full 255 step (literal runs of 15 and 270, matches of 19 and 274).
// Then N (default 20,000) mutations of them: bit flips, truncations and edits
// of length fields.  A --blocks file holds more blocks, each as a
// little-endian u32 length and the bytes (the test suite passes the blocks its
// GPU tests use); those are checked the same way, with no original to fall
// back on.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../plakar_amd/csrc/lz4_walk.h"

extern "C" {
int LZ4_decompress_safe(const char *src, char *dst, int compressedSize, int dstCapacity);
int LZ4_compress_default(const char *src, char *dst, int srcSize, int dstCapacity);
int LZ4_compressBound(int inputSize);
}

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

static const uint32_t kOutMax = 4u << 20;  // BD 7
static unsigned long g_accepted, g_rejected;

// 0: fine (rejected, or accepted with the right bytes); 1: a wrong acceptance.
static int check(const Bytes &in, const Bytes *orig, const char *what)
{
    const uint32_t n = uint32_t(in.size());
    uint8_t *src = static_cast<uint8_t *>(malloc(n ? n : 1));
    memcpy(src, in.data(), n);
    PtrRd rd{src};
    int bad = 0;
    const int64_t size = lz4w::decode_block(rd, n, nullptr, kOutMax);
    if (size < 0) {
        ++g_rejected;
    } else {
        ++g_accepted;
        uint8_t *out = static_cast<uint8_t *>(malloc(size ? size_t(size) : 1));
        const int64_t again = lz4w::decode_block(rd, n, out, uint32_t(size));
        char *ref = static_cast<char *>(malloc(size_t(size) + 64));
        const int r = LZ4_decompress_safe(reinterpret_cast<const char *>(src), ref, int(n), int(size) + 64);
        const bool same_ref = again == size && r == size && memcmp(out, ref, size_t(size)) == 0;
        const bool same_orig = again == size && orig && orig->size() == size_t(size) &&
                               memcmp(out, orig->data(), size_t(size)) == 0;
        if (!same_ref && !same_orig) {
            fprintf(stderr, "%s: accepted %u bytes as %lld (emit %lld), liblz4 says %d\n", what, n, (long long)size,
                    (long long)again, r);
            bad = 1;
        }
        free(ref);
        free(out);
    }
    free(src);
    return bad;
}

static Bytes compress(const Bytes &b)
{
    Bytes c(size_t(LZ4_compressBound(int(b.size()))));
    const int n = LZ4_compress_default(reinterpret_cast<const char *>(b.data()), reinterpret_cast<char *>(c.data()),
                                       int(b.size()), int(c.size()));
    if (n <= 0) {
        fprintf(stderr, "LZ4_compress_default failed\n");
        exit(2);
    }
    c.resize(size_t(n));
    return c;
}

static void put_len(Bytes &o, uint32_t v)  // the extension bytes of a nibble that was 15
{
    v -= 15;
    for (; v >= 255; v -= 255) o.push_back(255);
    o.push_back(uint8_t(v));
}

struct SeqSpec {
    uint32_t lits, off, mlen;
};

// A block of the given sequences (literals are fresh random bytes) and a last
// run of `tail` literals; content: what it decodes to.
static Bytes make_block(const std::vector<SeqSpec> &seqs, uint32_t tail, Bytes &content)
{
    Bytes o;
    content.clear();
    auto lits = [&](uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t b = uint8_t(rnd());
            o.push_back(b);
            content.push_back(b);
        }
    };
    for (const SeqSpec &s : seqs) {
        const uint32_t m = s.mlen - 4;
        o.push_back(uint8_t((s.lits >= 15 ? 15 : s.lits) << 4 | (m >= 15 ? 15 : m)));
        if (s.lits >= 15) put_len(o, s.lits);
        lits(s.lits);
        o.push_back(uint8_t(s.off));
        o.push_back(uint8_t(s.off >> 8));
        if (m >= 15) put_len(o, m);
        const size_t pos = content.size();
        for (uint32_t i = 0; i < s.mlen; ++i) content.push_back(content[pos - s.off + i % s.off]);
    }
    o.push_back(uint8_t((tail >= 15 ? 15 : tail) << 4));
    if (tail >= 15) put_len(o, tail);
    lits(tail);
    return o;
}

static Bytes mutate(const Bytes &b)
{
    Bytes m = b;
    switch (rnd() % 4) {
    case 0:  // bit flips
        for (uint32_t k = 1 + rnd() % 3; k; --k) m[rnd() % m.size()] ^= uint8_t(1u << (rnd() % 8));
        break;
    case 1:  // truncation
        m.resize(rnd() % m.size());
        break;
    case 2: {  // a length field: a token's nibbles or a neighbour of the block's start or end
        const size_t span = m.size() < 64 ? m.size() : 64;
        const size_t at = (rnd() & 1) ? rnd() % span : m.size() - 1 - rnd() % span;
        static const uint8_t v[] = {0x00, 0x0F, 0xF0, 0xFF, 0x10, 0x01};
        m[at] = v[rnd() % 6];
        break;
    }
    default: {  // an offset or extension byte anywhere: 0, 255 or +-1
        const size_t at = rnd() % m.size();
        const uint32_t how = rnd() % 4;
        m[at] = how == 0 ? 0 : how == 1 ? 255 : how == 2 ? uint8_t(m[at] + 1) : uint8_t(m[at] - 1);
        break;
    }
    }
    return m;
}

int main(int argc, char **argv)
{
    unsigned long mutations = 20000;
    std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--mutations") && i + 1 < argc) mutations = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--blocks") && i + 1 < argc) files.push_back(argv[++i]);
        else {
            fprintf(stderr, "usage: %s [--mutations N] [--blocks FILE]...\n", argv[0]);
            return 2;
        }
    }
    std::vector<Bytes> blocks, contents;
    {  // the block fixture
        Bytes c(40960);
        for (auto &x : c) x = uint8_t(rnd());
        const Bytes head(c.begin(), c.begin() + 20480);  // a copy: no insert from the vector into itself
        c.insert(c.end(), head.begin(), head.end());
        c.insert(c.end(), 5000, 0x07);
        for (int i = 0; i < 700; ++i) c.insert(c.end(), {'a', 'b', 'c'});
        for (int i = 0; i < 100; ++i) c.push_back(uint8_t(rnd()));
        blocks.push_back(compress(c));
        contents.push_back(c);
    }
    {  // offset 65,535
        Bytes c(65535);
        for (auto &x : c) x = uint8_t(rnd());
        const Bytes head(c.begin(), c.begin() + 4096);
        c.insert(c.end(), head.begin(), head.end());
        blocks.push_back(compress(c));
        contents.push_back(c);
    }
    {  // extension terminators
        Bytes c;
        blocks.push_back(make_block({{15, 7, 19}, {270, 100, 274}, {0, 1, 19}, {3, 2, 274}}, 15, c));
        contents.push_back(c);
        blocks.push_back(make_block({{270, 270, 4}, {15, 15, 18}, {14, 1, 273}}, 270, c));
        contents.push_back(c);
    }
    int bad = 0;
    for (size_t i = 0; i < blocks.size(); ++i) {
        const unsigned long before = g_accepted;
        bad |= check(blocks[i], nullptr, "fixture");  // against liblz4 alone
        if (g_accepted == before) {
            fprintf(stderr, "fixture %zu was rejected\n", i);
            bad = 1;
        }
        Bytes out(contents[i].size());
        PtrRd rd{blocks[i].data()};
        if (lz4w::decode_block(rd, uint32_t(blocks[i].size()), out.data(), uint32_t(out.size())) !=
                int64_t(out.size()) || out != contents[i]) {
            fprintf(stderr, "fixture %zu does not decode to its content\n", i);
            bad = 1;
        }
    }
    for (unsigned long k = 0; k < mutations && !bad; ++k) {
        const size_t f = k % blocks.size();
        bad |= check(mutate(blocks[f]), &contents[f], "mutation");
    }
    for (const std::string &path : files) {
        FILE *fp = fopen(path.c_str(), "rb");
        if (!fp) {
            fprintf(stderr, "cannot open %s\n", path.c_str());
            return 2;
        }
        uint8_t h[4];
        while (fread(h, 1, 4, fp) == 4) {
            const uint32_t n = uint32_t(h[0]) | uint32_t(h[1]) << 8 | uint32_t(h[2]) << 16 | uint32_t(h[3]) << 24;
            Bytes b(n);
            if (n && fread(b.data(), 1, n, fp) != n) {
                fprintf(stderr, "%s: short record\n", path.c_str());
                fclose(fp);
                return 2;
            }
            bad |= check(b, nullptr, path.c_str());
        }
        fclose(fp);
    }
    printf("lz4d_host_fuzz: %lu accepted, %lu rejected, %s\n", g_accepted, g_rejected, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
