// The range planner of cdc_restore_ranges (plakar_amd/csrc/read_plan.h) under
//   g++ -fsanitize=address,undefined
// Hand-made and seeded cases, each held against a brute-force byte map: a
// file byte is named by (blob id, offset inside the blob), the plan is played
// (scratch buffer, then the segments into the output image), and every byte
// of every range must come out of the image named as the file names it.
// Checked besides: destinations sorted, disjoint and back to back; each blob
// once per batch, in order of first use; upto exactly the largest end inside
// the blob; the scratch places the exclusive sum of upto; both budgets passed
// by less than one chunk; pieces numbered, in order, cut on chunk boundaries;
// empty, invalid and not-found ranges.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <vector>

#include "../../plakar_amd/csrc/read_plan.h"

static int g_bad;
static unsigned long g_cases, g_ranges, g_bytes;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            ++g_bad;                                    \
            return;                                     \
        }                                               \
    } while (0)

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 16);
}

struct FileSpec {
    std::vector<uint32_t> blob, len;
};
typedef uint64_t Name;  // blob id << 32 | offset inside the blob
static const Name kNone = ~0ull;

static void run_case(const char *what, const std::vector<FileSpec> &fs, const std::vector<rplan::Range> &ranges,
                     uint64_t out_budget, uint64_t dec_budget)
{
    ++g_cases;
    std::vector<rplan::File> files;
    uint32_t max_chunk = 0;
    for (const FileSpec &f : fs) {
        files.push_back(rplan::File{f.blob.size(), f.blob.data(), f.len.data()});
        for (uint32_t l : f.len) max_chunk = std::max(max_chunk, l);
    }
    // the files as names, byte by byte, and their chunk starts
    std::vector<std::vector<Name>> bytes(fs.size());
    std::vector<std::set<uint64_t>> starts(fs.size());
    for (size_t i = 0; i < fs.size(); ++i) {
        uint64_t at = 0;
        for (size_t c = 0; c < fs[i].blob.size(); ++c) {
            starts[i].insert(at);
            for (uint32_t k = 0; k < fs[i].len[c]; ++k) bytes[i].push_back(Name(fs[i].blob[c]) << 32 | k);
            at += fs[i].len[c];
        }
        starts[i].insert(at);
    }
    std::vector<rplan::RBatch> batches;
    std::vector<rplan::RangeInfo> info;
    rplan::plan_ranges(files.data(), files.size(), ranges.data(), ranges.size(), out_budget, dec_budget, batches, info);
    CHECK(info.size() == ranges.size(), "%s", what);
    std::vector<uint64_t> got(ranges.size(), 0);   // bytes delivered so far, per range
    std::vector<uint32_t> seen(ranges.size(), 0);  // pieces seen
    std::vector<bool> closed(ranges.size(), false);
    uint32_t last_range = 0;
    bool any_piece = false;
    for (size_t bi = 0; bi < batches.size(); ++bi) {
        const rplan::RBatch &B = batches[bi];
        CHECK(!B.pieces.empty(), "%s: an empty batch", what);
        // blobs: distinct, placed by the exclusive sum of upto
        std::set<uint64_t> keys;
        uint64_t off = 0;
        std::vector<uint64_t> max_end(B.blobs.size(), 0);
        for (const rplan::RBlob &b : B.blobs) {
            CHECK(keys.insert(uint64_t(b.id) << 32 | b.len).second, "%s: a blob twice in a batch", what);
            CHECK(b.off == off && b.upto >= 1 && b.upto <= b.len, "%s: blob place or upto", what);
            off += b.upto;
        }
        CHECK(B.scratch_bytes == off, "%s: scratch bytes", what);
        // the scratch buffer as names: the first upto bytes of each blob
        std::vector<Name> scratch;
        for (const rplan::RBlob &b : B.blobs)
            for (uint64_t k = 0; k < b.upto; ++k) scratch.push_back(Name(b.id) << 32 | k);
        // the segments into the image
        std::vector<Name> image(B.out_bytes, kNone);
        uint64_t dst = 0;
        uint32_t first_use = 0;
        for (const rplan::Segment &S : B.segs) {
            CHECK(S.dst_off == dst && S.len > 0, "%s: destinations are not back to back", what);
            CHECK(S.blob < B.blobs.size() && S.blob <= first_use, "%s: blobs are not in order of first use", what);
            if (S.blob == first_use) ++first_use;
            const rplan::RBlob &b = B.blobs[S.blob];
            CHECK(S.src_off >= b.off && S.src_off + S.len <= b.off + b.upto, "%s: a source outside its blob's prefix", what);
            max_end[S.blob] = std::max(max_end[S.blob], S.src_off + S.len - b.off);
            CHECK(S.dst_off + S.len <= B.out_bytes, "%s: a destination past the image", what);
            for (uint64_t k = 0; k < S.len; ++k) image[S.dst_off + k] = scratch[S.src_off + k];
            dst += S.len;
        }
        CHECK(dst == B.out_bytes && first_use == B.blobs.size(), "%s: image bytes or an unused blob", what);
        for (size_t b = 0; b < B.blobs.size(); ++b) CHECK(max_end[b] == B.blobs[b].upto, "%s: upto is not the largest end", what);
        CHECK(B.out_bytes < out_budget + std::max<uint64_t>(max_chunk, 1) + (out_budget == 0), "%s: output budget", what);
        CHECK(B.scratch_bytes < dec_budget + std::max<uint64_t>(max_chunk, 1) + (dec_budget == 0), "%s: decoded budget", what);
        // the pieces
        uint64_t seg = 0, pdst = 0;
        for (const rplan::RPiece &P : B.pieces) {
            CHECK(P.range < ranges.size() && info[P.range].status == CDC_OK, "%s: a piece of a failed range", what);
            CHECK(!any_piece || P.range >= last_range, "%s: pieces out of the caller's order", what);
            any_piece = true;
            last_range = P.range;
            const rplan::Range &R = ranges[P.range];
            CHECK(!closed[P.range] && P.piece == seen[P.range] && P.range_off == got[P.range], "%s: piece order", what);
            CHECK(P.seg0 == seg && P.dst_off == pdst, "%s: piece segments or place", what);
            uint64_t sum = 0;
            for (uint64_t s = P.seg0; s < P.seg0 + P.nsegs; ++s) sum += B.segs[s].len;
            CHECK(sum == P.len, "%s: piece length", what);
            const uint64_t f0 = R.offset + P.range_off;
            for (uint64_t k = 0; k < P.len; ++k)
                CHECK(image[P.dst_off + k] == bytes[R.file][f0 + k], "%s: range %u byte %llu", what, P.range,
                      (unsigned long long)(P.range_off + k));
            g_bytes += P.len;
            if (P.piece != 0) CHECK(starts[R.file].count(f0), "%s: a piece begins inside a chunk", what);
            if (!P.last) CHECK(starts[R.file].count(f0 + P.len) && P.len > 0, "%s: a piece ends inside a chunk", what);
            seg += P.nsegs;
            pdst += P.len;
            got[P.range] += P.len;
            ++seen[P.range];
            closed[P.range] = P.last;
        }
        CHECK(seg == B.segs.size() && pdst == B.out_bytes, "%s: segments or bytes outside every piece", what);
    }
    for (size_t r = 0; r < ranges.size(); ++r) {
        ++g_ranges;
        const rplan::Range &R = ranges[r];
        int want = CDC_OK;
        uint64_t size = 0, len = 0;
        if (R.file >= fs.size()) {
            want = CDC_E_INVALID;
        } else {
            size = bytes[R.file].size();
            if (R.offset > size) {
                want = CDC_E_INVALID;
            } else {
                len = std::min(R.length, size - R.offset);
                for (uint64_t k = 0; k < len; ++k)
                    if (uint32_t(bytes[R.file][R.offset + k] >> 32) == rplan::kMissing) want = CDC_E_NOTFOUND;
            }
        }
        CHECK(info[r].status == want, "%s: range %zu status %d, want %d", what, r, info[r].status, want);
        if (want != CDC_OK) {
            CHECK(seen[r] == 0 && info[r].pieces == 0, "%s: a failed range has pieces", what);
            continue;
        }
        CHECK(info[r].size == size && info[r].length == len, "%s: range %zu size or length", what, r);
        CHECK(closed[r] && got[r] == len && seen[r] == info[r].pieces && seen[r] >= 1, "%s: range %zu not covered", what, r);
    }
}

static FileSpec file_of(std::vector<std::pair<uint32_t, uint32_t>> chunks)
{
    FileSpec f;
    for (auto &c : chunks) {
        f.blob.push_back(c.first);
        f.len.push_back(c.second);
    }
    return f;
}

int main()
{
    // hand-made: an empty file (one empty chunk), one byte, several chunks, a duplicate, a repeated chunk, a hole
    std::vector<FileSpec> fs = {file_of({{0, 0}}),
                                file_of({{1, 1}}),
                                file_of({{2, 100}, {3, 50}, {4, 1}, {5, 200}}),
                                file_of({{2, 100}, {3, 50}, {4, 1}, {5, 200}}),
                                file_of({{6, 64}, {6, 64}, {6, 64}, {7, 10}, {6, 64}}),
                                file_of({{8, 30}, {rplan::kMissing, 30}, {9, 30}}),
                                file_of({})};
    std::vector<rplan::Range> rs;
    for (uint32_t f = 0; f < 8; ++f)
        for (uint64_t off = 0; off <= 360; off += (off < 160 ? 1 : 13))
            for (uint64_t len : {0ull, 1ull, 2ull, 49ull, 50ull, 51ull, 150ull, 1000ull, ~0ull}) rs.push_back({f, off, len});
    rs.push_back({2, 10, 20});
    rs.push_back({2, 10, 20});  // the same range twice
    rs.push_back({2, 0, 351});
    rs.push_back({2, 5, 200});  // overlapping
    for (uint64_t ob : {0ull, 1ull, 64ull, 100ull, 151ull, 1000ull, 1ull << 40})
        for (uint64_t db : {0ull, 1ull, 64ull, 200ull, 1ull << 40}) run_case("hand-made", fs, rs, ob, db);
    run_case("no ranges", fs, {}, 100, 100);
    run_case("no files", {}, {{0, 0, 1}}, 100, 100);
    // seeded
    for (int it = 0; it < 300; ++it) {
        std::vector<FileSpec> files(1 + rnd() % 5);
        const uint32_t ids = 1 + rnd() % 12;
        std::map<uint32_t, uint32_t> len_of;
        for (FileSpec &f : files) {
            const uint32_t n = rnd() % 12;
            for (uint32_t c = 0; c < n; ++c) {
                uint32_t id = rnd() % ids;
                if (rnd() % 40 == 0) id = rplan::kMissing;
                if (!len_of.count(id)) len_of[id] = rnd() % 9 == 0 ? 0 : 1 + rnd() % 300;
                f.blob.push_back(id);
                f.len.push_back(len_of[id]);
            }
        }
        std::vector<rplan::Range> ranges(rnd() % 40);
        for (rplan::Range &R : ranges) {
            R.file = rnd() % (uint32_t(files.size()) + (rnd() % 10 == 0));
            R.offset = rnd() % 1500;
            R.length = rnd() % 5 == 0 ? ~0ull : rnd() % 800;
        }
        const uint64_t budgets[5] = {1, 100, 301, 1000, 1ull << 30};
        run_case("seeded", files, ranges, budgets[rnd() % 5], budgets[rnd() % 5]);
    }
    printf("read_plan_check: %lu cases, %lu ranges, %lu bytes, %s\n", g_cases, g_ranges, g_bytes, g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
