// The host-side rules of the streamed gzip member (cdc_gzip_stream_piece),
// compiled from the library's own headers under the address and
// undefined-behaviour sanitizers (tests/test_archive_cpu.py builds and runs it):
//
//   J  the joiner and the final block (dfl::stream_end) after a block that
//      ends at each of the eight bits of a byte: two pieces written with
//      deflate_enc.h's bit writer, the raw DEFLATE stream handed to the test
//      (zlib inflates it there);
//   K  the running CRC-32 as the writer keeps it (register of the stream so
//      far, moved past a piece by crc_shift / crc_mul, plus the piece's own
//      register from 0) for second parts of 0, 1, 65,537 and 2^32 + 5 zero
//      bytes (the last in three pieces) and one of 65,537 other bytes;
//   B  the piece bound against the worst a piece can take: every span stored,
//      from every starting bit.
//
//   gzip_stream_check --out FILE     records: u32 n, stream, u32 k, content
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../plakar_amd/csrc/deflate_enc.h"
#include "../../plakar_amd/csrc/inflate_walk.h"

static void die(const char *what)
{
    printf("FAIL %s\n", what);
    exit(1);
}

// A fixed-Huffman block of literals, BFINAL clear, at bit `at` of the zeroed words; the bit after it.
static uint64_t fixed_block(uint32_t *words, uint64_t at, const std::vector<uint8_t> &lits)
{
    dfl::Serial one;
    dfl::BitW<dfl::Serial> B(one, words, at);
    B.put(dfl::kFixed << 1, 3);
    for (uint8_t c : lits) {
        if (c < 144) B.put(dfl::bit_reverse(0x30u + c, 8), 8);
        else B.put(dfl::bit_reverse(0x190u + (c - 144u), 9), 9);
    }
    B.put(0, 7);  // end of block
    B.flush();
    return B.pos();
}

// One piece: the block, then the joiner (and the final block); its bytes.
static std::vector<uint8_t> piece(const std::vector<uint8_t> &lits, bool final, uint32_t want_end_bit)
{
    uint32_t words[16] = {0};
    const uint64_t E = fixed_block(words, 0, lits);
    if ((E & 7u) != want_end_bit) die("the block does not end at the bit the case names");
    std::vector<uint8_t> out(64, 0xA5);
    for (uint64_t i = 0; i < (E + 7) / 8; ++i) out[i] = uint8_t(words[i >> 2] >> ((i & 3u) * 8u));
    const uint32_t sh = uint32_t(E & 7u);
    uint8_t *o = out.data() + (E >> 3);
    const uint32_t edge = sh ? *o : 0u;
    const uint32_t n = dfl::stream_end(o, edge | 0xFFFFFF00u, sh, final);  // bits past the byte are not taken
    if (n != (sh + dfl::joiner_bits(E)) / 8 + (final ? dfl::kFinalBytes : 0)) die("stream_end's length");
    const uint64_t total = (E >> 3) + n;
    if (total * 8 != E + dfl::joiner_bits(E) + (final ? 8 * dfl::kFinalBytes : 0)) die("the piece is not whole bytes");
    for (size_t i = total; i < out.size(); ++i)
        if (out[i] != 0xA5) die("stream_end wrote past its length");
    out.resize(total);
    return out;
}

static void put_rec(FILE *f, const std::vector<uint8_t> &a, const std::vector<uint8_t> &b)
{
    const uint32_t n = uint32_t(a.size()), k = uint32_t(b.size());
    fwrite(&n, 4, 1, f);
    fwrite(a.data(), 1, n, f);
    fwrite(&k, 4, 1, f);
    fwrite(b.data(), 1, k, f);
}

static uint32_t reg_of(const uint8_t *p, size_t n, uint32_t reg)
{
    for (size_t i = 0; i < n; ++i) reg = infw::crc_bits(reg, p[i]);
    return reg;
}

int main(int argc, char **argv)
{
    const char *path = nullptr;
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--out")) path = argv[i + 1];
    if (!path) die("usage: --out FILE");
    FILE *f = fopen(path, "wb");
    if (!f) die("cannot write the output");

    // J: a block of 8 literals, b of them >= 144, is 74 + b bits: it ends at bit (2 + b) % 8
    for (uint32_t b = 0; b < 8; ++b) {
        std::vector<uint8_t> first, second = {'t', 'a', 'r', 200, 201};
        for (uint32_t i = 0; i < 8; ++i) first.push_back(uint8_t(i < b ? 150 + 9 * i : 40 + 5 * i));
        const uint32_t end_bit = (2 + b) % 8;
        // the second piece ends at bit (3 + 8 * 3 + 9 * 2 + 7) % 8 = 4
        std::vector<uint8_t> s = piece(first, false, end_bit), t = piece(second, true, 4);
        printf("J %u %zu %zu\n", end_bit, s.size(), t.size());
        s.insert(s.end(), t.begin(), t.end());
        first.insert(first.end(), second.begin(), second.end());
        put_rec(f, s, first);
        // the same block alone, closed at once
        std::vector<uint8_t> one = piece(std::vector<uint8_t>(first.begin(), first.begin() + 8), true, end_bit);
        put_rec(f, one, std::vector<uint8_t>(first.begin(), first.begin() + 8));
    }
    fclose(f);

    // K: the writer's update, reg' = reg * x^(8 len) + (the piece's register from 0)
    const uint8_t head[] = {'a', 'r', 'c', 'h', 'i', 'v', 'e'};
    const uint32_t r0 = reg_of(head, sizeof(head), 0xFFFFFFFFu);
    {
        std::vector<uint8_t> z(65537, 0);
        if (reg_of(z.data(), z.size(), 0) != 0) die("zero bytes from a zero register");
    }
    const uint64_t zeros[] = {0, 1, 65537};
    for (uint64_t n : zeros) {
        const uint32_t r = infw::crc_mul(r0, infw::crc_shift(n)) ^ 0u;
        printf("K zeros %llu %08x\n", (unsigned long long)n, ~r);
    }
    {
        uint32_t r = r0;
        const uint64_t parts[] = {(1ull << 31) + 1, 1ull << 31, 4};  // each under 2 GiB + 2, together 2^32 + 5
        uint64_t total = 0;
        for (uint64_t n : parts) {
            r = infw::crc_mul(r, infw::crc_shift(n)) ^ 0u;
            total += n;
        }
        if (total != (1ull << 32) + 5) die("the parts' sum");
        printf("K zeros %llu %08x\n", (unsigned long long)total, ~r);
    }
    {
        std::vector<uint8_t> p(65537);
        for (size_t i = 0; i < p.size(); ++i) p[i] = uint8_t(i * 131 + (i >> 8));
        const uint32_t r = infw::crc_mul(r0, infw::crc_shift(p.size())) ^ reg_of(p.data(), p.size(), 0);
        printf("K pattern %zu %08x\n", p.size(), ~r);
        if (r != reg_of(p.data(), p.size(), r0)) die("the combined register is not the serial one");
    }

    // B: every span stored, from every starting bit, first piece and last
    const uint64_t lens[] = {1, 32767, 32768, 32769, 65536, (2ull << 20) + 32769, 0x7FFFFFFFull};
    for (uint64_t len : lens) {
        uint64_t worst = 0;
        for (uint32_t s0 = 0; s0 < 8; ++s0) {
            uint64_t P = 80 + s0;  // (a piece starts at bit 0 of a byte; the other bits bound more than can happen)
            for (uint64_t done = 0; done < len; done += dfl::kSpan)
                P += dfl::stored_bits(P, uint32_t(len - done < dfl::kSpan ? len - done : dfl::kSpan));
            P += dfl::joiner_bits(P);
            const uint64_t bytes = P / 8 + dfl::kFinalBytes + 8;
            if (bytes > worst) worst = bytes;
        }
        if (worst > dfl::stream_piece_bound(len)) die("the bound is under the stored form");
        printf("B %llu %llu %llu\n", (unsigned long long)len, (unsigned long long)worst,
               (unsigned long long)dfl::stream_piece_bound(len));
    }
    puts("ok");
    return 0;
}
