// cdc::Carver (plakar_amd/csrc/cdc_hostmem.h) against the carving lambda it
// replaced, restated here: 1,000 seeded size lists at alignments 16 and 256.
// Offsets and totals must be equal, every offset aligned, the ranges disjoint
// and ascending.  Stand-alone (no HIP): built with the sanitizers by
// tests/test_hostmem_cpu.py.
#define CDC_HOSTMEM_NO_HIP
#include "../../plakar_amd/csrc/cdc_hostmem.h"

#include <cstdint>
#include <cstdio>
#include <vector>

static uint64_t g_rng;
static uint64_t rnd()
{
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the two roundings as the four call sites wrote them
static uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }
static size_t align_up_old(size_t x, size_t a) { return (x + a - 1) / a * a; }

int main()
{
    static const size_t kEdge[] = {0, 1, 15, 16, 17, 255, 256, 257};
    size_t lists = 0, regions = 0;
    for (size_t align : {size_t(16), size_t(256)}) {
        for (uint64_t seed = 1; seed <= 1000; ++seed) {
            g_rng = seed * 0x51ED27ull + align;
            const size_t n = 1 + rnd() % 40;
            std::vector<size_t> sizes(n);
            for (size_t &s : sizes) {
                const uint64_t pick = rnd() % 9;
                s = pick < 8 ? kEdge[pick] : size_t(rnd() % (1u << 20));
            }
            size_t off = 0;
            auto take = [&](size_t bytes) {
                const size_t o = off;
                off = align == 16 ? size_t(align16(off + bytes)) : align_up_old(off + bytes, 256);
                return o;
            };
            cdc::Carver cv(align);
            size_t prev_end = 0;
            for (size_t i = 0; i < n; ++i) {
                const size_t want = take(sizes[i]), got = cv.take(sizes[i]);
                if (got != want || got % align || got < prev_end || cv.bytes() != off || cv.bytes() < got + sizes[i]) {
                    std::printf("FAIL align %zu seed %llu region %zu: size %zu offset %zu (lambda %zu), end of the one "
                                "before %zu, total %zu (lambda %zu)\n",
                                align, (unsigned long long)seed, i, sizes[i], got, want, prev_end, cv.bytes(), off);
                    return 1;
                }
                prev_end = got + sizes[i];
                ++regions;
            }
            ++lists;
        }
    }
    std::printf("%zu lists, %zu regions\nok\n", lists, regions);
    return 0;
}
