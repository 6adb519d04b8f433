// Stand-alone checker of the restore path's host-only code (restore_plan.h):
// the packfile index reader and the batch planner, built by
// tests/test_restore_cpu.py with -fsanitize=address,undefined together with
// the library's host SHA-256 (cdc_sha256.cpp).
//
//   * index reader: packfiles serialised here (packfile.go:241-294 restated)
//     parse back to their rows; every reject case is CDC_E_CORRUPT; mutated
//     and truncated packfiles, each in a heap buffer of exactly its size so
//     that any read past the end is a sanitizer report, are either rejected
//     or pass an independent re-check of everything the reader promises;
//   * planner: random chunk lists; segments tile each batch's output exactly,
//     every distinct blob is listed once and in order of first use, pieces
//     split on chunk boundaries and cover every file once, and no batch
//     passes its budget by more than one chunk.
//
// Prints "<a> accepted, <r> rejected, <p> plans, ok" and exits 0, or says what
// failed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <utility>
#include <vector>

#include "cdc_internal.h"
#include "restore_plan.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
            exit(1);                              \
        }                                         \
    } while (0)

static void sha(const void *d, size_t n, uint8_t out[32]) { cdc::sha256(d, n, out); }

static void put32(std::vector<uint8_t> &v, uint32_t x)
{
    for (int i = 0; i < 4; ++i) v.push_back(uint8_t(x >> (8 * i)));
}
static void put64(std::vector<uint8_t> &v, uint64_t x)
{
    for (int i = 0; i < 8; ++i) v.push_back(uint8_t(x >> (8 * i)));
}

struct Row {
    uint8_t type;
    uint8_t sum[32];
    uint32_t off, len;
};

static std::vector<uint8_t> serialize(const std::vector<Row> &rows, uint32_t data_len, int64_t ts, uint32_t version = 100)
{
    std::vector<uint8_t> out(data_len);
    for (auto &b : out) b = uint8_t(rnd());
    std::vector<uint8_t> idx;
    for (const Row &r : rows) {
        idx.push_back(r.type);
        idx.insert(idx.end(), r.sum, r.sum + 32);
        put32(idx, r.off);
        put32(idx, r.len);
    }
    uint8_t h[32];
    sha(idx.data(), idx.size(), h);
    out.insert(out.end(), idx.begin(), idx.end());
    put32(out, version);
    put64(out, uint64_t(ts));
    put32(out, uint32_t(rows.size()));
    put32(out, data_len);
    out.insert(out.end(), h, h + 32);
    return out;
}

static std::vector<Row> random_rows(uint32_t count, uint32_t *data_len)
{
    std::vector<Row> rows(count);
    uint32_t off = 0;
    for (Row &r : rows) {
        r.type = uint8_t(1 + below(3));
        for (auto &b : r.sum) b = uint8_t(rnd());
        r.off = off;
        r.len = below(4) == 0 ? 0 : uint32_t(below(200));
        off += r.len;
    }
    *data_len = off;
    return rows;
}

// parse from a heap copy of exactly len bytes
static int parse_exact(const uint8_t *bytes, size_t len, cdc_packfile_footer *f, std::vector<cdc_packfile_row> *rows)
{
    uint8_t *p = static_cast<uint8_t *>(malloc(len ? len : 1));
    if (len) memcpy(p, bytes, len);
    cdc_packfile_footer f0;
    int st = rplan::parse_packfile(len ? p : nullptr, len, sha, &f0, nullptr, 0);
    if (st == CDC_OK) {
        rows->assign(f0.count, cdc_packfile_row());
        const int st2 = rplan::parse_packfile(p, len, sha, f, rows->data(), rows->size());
        CHECK(st2 == CDC_OK && memcmp(&f0, f, sizeof(f0)) == 0, "the second pass differs from the first");
    }
    free(p);
    return st;
}

// everything the reader promises about an accepted packfile, restated
static void recheck(const uint8_t *bytes, size_t len, const cdc_packfile_footer &f,
                    const std::vector<cdc_packfile_row> &rows)
{
    CHECK(len >= 52 && f.version == 100, "accepted a short packfile or a wrong version");
    CHECK(uint64_t(f.index_offset) + 41ull * f.count + 52 == len, "accepted an index of the wrong length");
    CHECK(rows.size() == f.count, "row count");
    const uint8_t *idx = bytes + f.index_offset;
    for (size_t i = 0; i < rows.size(); ++i) {
        CHECK(uint64_t(rows[i].offset) + rows[i].length <= f.index_offset, "accepted an entry past the index offset");
        CHECK(rows[i].type == idx[41 * i] && memcmp(rows[i].checksum, idx + 41 * i + 1, 32) == 0, "row %zu differs", i);
    }
    uint8_t h[32];
    sha(idx, 41 * rows.size(), h);
    CHECK(memcmp(h, f.index_checksum, 32) == 0, "accepted an index checksum mismatch");
}

static void check_index_reader(uint64_t *accepted, uint64_t *rejected)
{
    const uint32_t counts[] = {0, 1, 2, 7, 300};
    std::vector<std::vector<uint8_t>> valid;
    for (uint32_t count : counts) {
        uint32_t data_len;
        const std::vector<Row> rows = random_rows(count, &data_len);
        const std::vector<uint8_t> pk = serialize(rows, data_len, int64_t(rnd() >> 1));
        cdc_packfile_footer f;
        std::vector<cdc_packfile_row> got;
        CHECK(parse_exact(pk.data(), pk.size(), &f, &got) == CDC_OK, "a valid packfile of %u rows is rejected", count);
        recheck(pk.data(), pk.size(), f, got);
        for (uint32_t i = 0; i < count; ++i)
            CHECK(got[i].type == rows[i].type && got[i].offset == rows[i].off && got[i].length == rows[i].len &&
                      memcmp(got[i].checksum, rows[i].sum, 32) == 0,
                  "row %u", i);
        valid.push_back(pk);
        ++*accepted;
    }
    // the reject cases, each on its own
    {
        cdc_packfile_footer f;
        std::vector<cdc_packfile_row> got;
        uint32_t data_len;
        const std::vector<Row> rows = random_rows(5, &data_len);
        std::vector<uint8_t> pk = serialize(rows, data_len, 7);
        for (size_t n = 0; n < 52; ++n)
            CHECK(parse_exact(pk.data() + pk.size() - n, n, &f, &got) == CDC_E_CORRUPT, "%zu bytes accepted", n);
        std::vector<uint8_t> longer = pk;   // one byte too many before the footer: index length != 41 * count
        longer.insert(longer.begin() + data_len, 0);
        CHECK(parse_exact(longer.data(), longer.size(), &f, &got) == CDC_E_CORRUPT, "index length");
        std::vector<uint8_t> cnt = pk;      // count + 1
        cnt[pk.size() - 52 + 12] += 1;
        CHECK(parse_exact(cnt.data(), cnt.size(), &f, &got) == CDC_E_CORRUPT, "count");
        CHECK(parse_exact(serialize(rows, data_len, 7, 101).data(), pk.size(), &f, &got) == CDC_E_CORRUPT, "version");
        std::vector<Row> past = rows;       // an entry that ends one byte past the index offset
        past[4].len += 1;
        const std::vector<uint8_t> pp = serialize(past, data_len, 7);
        CHECK(parse_exact(pp.data(), pp.size(), &f, &got) == CDC_E_CORRUPT, "entry past the index offset");
        std::vector<uint8_t> sum = pk;      // a flipped bit in the index
        sum[data_len + 3] ^= 1;
        CHECK(parse_exact(sum.data(), sum.size(), &f, &got) == CDC_E_CORRUPT, "index checksum");
        std::vector<uint8_t> fsum = pk;     // and in the footer's checksum
        fsum[pk.size() - 1] ^= 0x80;
        CHECK(parse_exact(fsum.data(), fsum.size(), &f, &got) == CDC_E_CORRUPT, "footer checksum");
        *rejected += 58;
    }
    // mutations
    for (int it = 0; it < 20000; ++it) {
        std::vector<uint8_t> pk = valid[below(4)];  // the 300-row one only now and then: it costs a long SHA-256
        if (it % 50 == 0) pk = valid[4];
        const int kind = int(below(4));
        if (kind == 0) {  // footer fields
            const size_t at = pk.size() - 52 + below(20);
            pk[at] = uint8_t(below(2) ? rnd() : pk[at] ^ (1u << below(8)));
        } else if (kind == 1) {  // an index byte (offsets and lengths more often than checksums)
            if (pk.size() > 52) {
                const size_t at = below(pk.size() - 52);
                pk[at] ^= uint8_t(1u << below(8));
            }
        } else if (kind == 2) {  // truncated
            pk.resize(below(pk.size() + 1));
        } else {  // a changed row with the checksum made right again: only the bounds check is left
            cdc_packfile_footer f;
            std::vector<cdc_packfile_row> rows;
            if (parse_exact(pk.data(), pk.size(), &f, &rows) == CDC_OK && f.count) {
                uint8_t *e = pk.data() + f.index_offset + 41 * below(f.count);
                const uint32_t v = below(2) ? uint32_t(rnd()) : uint32_t(below(f.index_offset + 3));
                memcpy(e + (below(2) ? 33 : 37), &v, 4);
                sha(pk.data() + f.index_offset, 41 * size_t(f.count), pk.data() + pk.size() - 32);
            }
        }
        cdc_packfile_footer f;
        std::vector<cdc_packfile_row> rows;
        if (parse_exact(pk.data(), pk.size(), &f, &rows) == CDC_OK) {
            recheck(pk.data(), pk.size(), f, rows);
            ++*accepted;
        } else {
            ++*rejected;
        }
    }
}

static void check_plan(const std::vector<std::vector<uint32_t>> &blob, const std::vector<std::vector<uint32_t>> &len,
                       uint64_t budget)
{
    std::vector<rplan::File> files;
    for (size_t i = 0; i < blob.size(); ++i) files.push_back(rplan::File{blob[i].size(), blob[i].data(), len[i].data()});
    std::vector<rplan::Batch> batches;
    rplan::plan(files.data(), files.size(), budget, batches);
    std::vector<uint64_t> next_chunk(files.size(), 0), next_off(files.size(), 0);
    std::vector<int> pieces(files.size(), 0), lasts(files.size(), 0);
    int64_t prev_file = -1;
    for (const rplan::Batch &B : batches) {
        CHECK(!B.pieces.empty(), "an empty batch");
        // distinct blobs: once each, packed, every one used, in order of first use
        std::set<std::pair<uint32_t, uint32_t>> seen;
        uint64_t off = 0;
        for (const rplan::Blob &b : B.blobs) {
            CHECK(seen.insert({b.id, b.len}).second, "blob %u listed twice", b.id);
            CHECK(b.off == off, "blob offset");
            off += b.len;
        }
        CHECK(off == B.plain_bytes, "plain_bytes");
        // segments tile the output image exactly
        uint64_t dst = 0, nonzero = 0;
        uint32_t first_use = 0;
        bool identity = true;
        for (const rplan::Segment &S : B.segs) {
            CHECK(S.dst_off == dst, "segments do not tile the image");
            CHECK(S.blob < B.blobs.size() && S.src_off == B.blobs[S.blob].off && S.len == B.blobs[S.blob].len, "segment source");
            CHECK(S.blob <= first_use, "blobs are not in order of first use");
            if (S.blob == first_use) ++first_use;
            identity = identity && S.src_off == S.dst_off;
            nonzero += S.len != 0;
            dst += S.len;
        }
        CHECK(first_use == B.blobs.size(), "a listed blob is never used");
        CHECK(dst == B.out_bytes && identity == B.identity, "out_bytes / identity");
        CHECK(B.out_bytes <= budget || nonzero == 1, "a batch passes its budget by more than one chunk");
        // pieces: in file order, on chunk boundaries, back to back in the image
        uint64_t pdst = 0, seg = 0;
        for (const rplan::Piece &P : B.pieces) {
            CHECK(P.file < files.size() && int64_t(P.file) >= prev_file, "piece order");
            CHECK(int64_t(P.file) > prev_file || !P.first, "a file has two first pieces");
            prev_file = P.file;
            CHECK(P.chunk0 == next_chunk[P.file] && P.file_off == next_off[P.file], "a piece does not continue its file");
            CHECK(P.first == (pieces[P.file] == 0), "first");
            CHECK(P.dst_off == pdst && P.seg0 == seg, "piece placement");
            uint64_t sum = 0;
            for (uint64_t j = 0; j < P.nchunks; ++j) {
                const rplan::Segment &S = B.segs[size_t(seg + j)];
                CHECK(S.len == len[P.file][size_t(P.chunk0 + j)] && B.blobs[S.blob].id == blob[P.file][size_t(P.chunk0 + j)],
                      "a segment is not its chunk");
                sum += S.len;
            }
            CHECK(sum == P.len, "piece length");
            seg += P.nchunks;
            pdst += P.len;
            next_chunk[P.file] += P.nchunks;
            next_off[P.file] += P.len;
            ++pieces[P.file];
            CHECK(P.last == (next_chunk[P.file] == files[P.file].nchunks), "last");
            lasts[P.file] += P.last;
            CHECK(P.nchunks || P.last, "an empty piece in the middle of a file");
        }
        CHECK(seg == B.segs.size() && pdst == B.out_bytes, "pieces do not cover the batch");
    }
    for (size_t i = 0; i < files.size(); ++i)
        CHECK(pieces[i] >= 1 && lasts[i] == 1 && next_chunk[i] == files[i].nchunks, "file %zu is not covered once", i);
}

int main()
{
    uint64_t accepted = 0, rejected = 0, plans = 0;
    check_index_reader(&accepted, &rejected);
    for (int it = 0; it < 3000; ++it) {
        const size_t nfiles = size_t(below(12));
        const uint32_t nblobs = uint32_t(1 + below(it % 3 ? 8 : 200));  // few blobs: many repeats
        const uint32_t max_len = it % 5 ? 1000 : 16;
        std::vector<uint32_t> blob_len(nblobs);
        for (auto &l : blob_len) l = below(5) ? uint32_t(below(max_len)) : 0;
        std::vector<std::vector<uint32_t>> blob(nfiles), len(nfiles);
        for (size_t f = 0; f < nfiles; ++f) {
            const size_t n = size_t(below(4) ? below(40) : 0);  // files without chunks too
            for (size_t c = 0; c < n; ++c) {
                const uint32_t id = uint32_t(below(nblobs));
                blob[f].push_back(id);
                // now and then a recorded length that is not the blob's: its own distinct entry
                len[f].push_back(below(50) ? blob_len[id] : blob_len[id] + 1);
            }
        }
        const uint64_t budgets[] = {1, 7, 500, 1000, 4096, 1u << 20};
        check_plan(blob, len, budgets[below(6)]);
        ++plans;
    }
    printf("%llu accepted, %llu rejected, %llu plans, ok\n", (unsigned long long)accepted, (unsigned long long)rejected,
           (unsigned long long)plans);
    return 0;
}
