// What a set of gzip members is made of, counted with the walker the device
// uses (plakar_amd/csrc/inflate_walk.h) and a sink that only counts: literals,
// matches and their bytes, stored bytes, blocks, and the member with the most
// symbols (the chain that a kernel of one wave per member waits for).
// tools/decode_bench.py --gzip divides k_gz_emit's time by these.
//
//   inflate_count FILE      (per member: little-endian u32 length, the bytes)
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../plakar_amd/csrc/inflate_walk.h"

struct PtrRd {
    const uint8_t *p;
    uint32_t operator()(uint32_t i) const { return p[i]; }
};

struct Counter {
    uint64_t lits = 0, matches = 0, match_bytes = 0, stored_bytes = 0, blocks = 0;
    void lit(uint32_t, uint32_t) { ++lits; }
    void match(uint32_t, uint32_t, uint32_t len)
    {
        ++matches;
        match_bytes += len;
    }
    void stored(uint32_t, uint32_t, uint32_t len) { stored_bytes += len; }
    void flush() { ++blocks; }
};

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    static infw::Tables fixed, dyn;
    infw::Serial par;
    infw::build_fixed(par, fixed);
    Counter c;
    uint64_t members = 0, failed = 0, out_bytes = 0;
    uint64_t top_lits = 0, top_matches = 0, top_bytes = 0;  // the member with the most symbols: the longest chain
    uint8_t h[4];
    std::vector<uint8_t> b;
    while (fread(h, 1, 4, fp) == 4) {
        const uint32_t n = uint32_t(h[0]) | uint32_t(h[1]) << 8 | uint32_t(h[2]) << 16 | uint32_t(h[3]) << 24;
        b.resize(n);
        if (n && fread(b.data(), 1, n, fp) != n) return 2;
        PtrRd rd{b.data()};
        uint32_t hlen = 0, claim = 0, opos = 0, end = 0;
        ++members;
        const uint64_t l0 = c.lits, m0 = c.matches;
        if (infw::member_claim(rd, n, hlen, claim) != infw::kOk ||
            (n && infw::inflate_body(rd, n, hlen, c, claim, dyn, fixed, par, opos, end) != infw::kOk) || opos != claim)
            ++failed;
        out_bytes += opos;
        if (c.lits - l0 + c.matches - m0 > top_lits + top_matches) {
            top_lits = c.lits - l0;
            top_matches = c.matches - m0;
            top_bytes = opos;
        }
    }
    fclose(fp);
    printf("{\"members\": %llu, \"failed\": %llu, \"out_bytes\": %llu, \"literals\": %llu, \"matches\": %llu, "
           "\"match_bytes\": %llu, \"stored_bytes\": %llu, \"blocks\": %llu, \"longest_literals\": %llu, "
           "\"longest_matches\": %llu, \"longest_out_bytes\": %llu}\n",
           (unsigned long long)members, (unsigned long long)failed, (unsigned long long)out_bytes,
           (unsigned long long)c.lits, (unsigned long long)c.matches, (unsigned long long)c.match_bytes,
           (unsigned long long)c.stored_bytes, (unsigned long long)c.blocks, (unsigned long long)top_lits,
           (unsigned long long)top_matches, (unsigned long long)top_bytes);
    return failed ? 1 : 0;
}
