// Host-only pieces of archive's zip format, shared by the library
// (cdc_archive.cpp) and the stand-alone sanitizer program
// tests/c/zip_plan_check.cpp:
//
//   * the container of `plakar archive -format zip` (cmd/plakar/subcommands/
//     archive/archive.go:194-245 through Go's archive/zip Writer on a
//     non-seekable output: FileInfoHeader, Method = Deflate, CreateHeader): a
//     local header per file, after its stream a data descriptor (written on
//     the device, where the compressed size is known), and after the last
//     entry the central directory and the end records, zip64 where needed;
//   * the batch planner of a zip run: archive_plan.h's over file bytes and
//     local headers: which blobs a batch decodes, where every chunk occurrence
//     lands in the batch's image (file bytes back to back, nothing else) and
//     the pieces cdc_zip_pieces_device deflates.
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include "archive_plan.h"

namespace zplan {

constexpr uint64_t kMax32 = 0xFFFFFFFFull;
constexpr uint32_t kMax16 = 0xFFFFu;
constexpr uint16_t kVersion20 = 20, kVersion45 = 45, kCreator = 0x0314;  // Unix, 2.0
constexpr uint16_t kFlagDescriptor = 0x0008, kFlagUTF8 = 0x0800, kMethodDeflate = 8;
constexpr size_t kLocalFixed = 30, kCentralFixed = 46, kEndLen = 22, kEnd64Len = 56, kLoc64Len = 20, kTimeExtra = 9;

static inline void put16(std::vector<uint8_t> &o, uint32_t v)
{
    o.push_back(uint8_t(v));
    o.push_back(uint8_t(v >> 8));
}
static inline void put32(std::vector<uint8_t> &o, uint64_t v)
{
    for (int i = 0; i < 4; ++i) o.push_back(uint8_t(v >> (8 * i)));
}
static inline void put64(std::vector<uint8_t> &o, uint64_t v)
{
    for (int i = 0; i < 8; ++i) o.push_back(uint8_t(v >> (8 * i)));
}

// archive/zip's detectUTF8: `valid` when the name is UTF-8 as Go decodes it (no
// overlong forms, no surrogates, nothing past U+10FFFF), `require` when a rune
// is below 0x20, above 0x7d or a backslash: names CP-437 and UTF-8 spell alike
// need no flag.
static inline void detect_utf8(const char *s, size_t n, bool &valid, bool &require)
{
    valid = true;
    require = false;
    for (size_t i = 0; i < n;) {
        const uint8_t c = uint8_t(s[i]);
        uint32_t r = c;
        size_t len = 1;
        if (c >= 0x80) {
            uint32_t lo = 0x80, hi = 0xBF;  // the second byte's range
            if (c >= 0xC2 && c <= 0xDF) len = 2, r = c & 0x1Fu;
            else if (c >= 0xE0 && c <= 0xEF) len = 3, r = c & 0x0Fu, lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;
            else if (c >= 0xF0 && c <= 0xF4) len = 4, r = c & 0x07u, lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;
            else len = 0;
            if (len == 0 || i + len > n) {
                valid = require = false;
                return;
            }
            for (size_t k = 1; k < len; ++k) {
                const uint8_t d = uint8_t(s[i + k]);
                if (d < (k == 1 ? lo : 0x80u) || d > (k == 1 ? hi : 0xBFu)) {
                    valid = require = false;
                    return;
                }
                r = r << 6 | (d & 0x3Fu);
            }
        }
        i += len;
        if (r < 0x20 || r > 0x7d || r == 0x5c) require = true;
    }
}

// Days since 1970-01-01 to a civil date (proleptic Gregorian).
static inline void civil_from_days(int64_t z, int64_t &y, unsigned &m, unsigned &d)
{
    z += 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const unsigned doe = unsigned(z - era * 146097);
    const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    y = int64_t(yoe) + era * 400;
    const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const unsigned mp = (5 * doy + 2) / 153;
    d = doy - (153 * mp + 2) / 5 + 1;
    m = mp < 10 ? mp + 3 : mp - 9;
    if (m <= 2) ++y;
}

// archive/zip's timeToMsDosTime of mtime in UTC, two-second resolution.  A year
// outside the format's 1980..2107 is clamped to the range's end (Go lets the
// seven-bit year field wrap; that is not reproduced).
static inline void dos_time(int64_t mtime, uint16_t &date, uint16_t &time)
{
    const int64_t day = mtime >= 0 ? mtime / 86400 : -((-mtime + 86399) / 86400);
    const int64_t sec = mtime - day * 86400;
    int64_t y;
    unsigned m, d;
    civil_from_days(day, y, m, d);
    unsigned hh = unsigned(sec / 3600), mm = unsigned(sec / 60 % 60), ss = unsigned(sec % 60);
    if (y < 1980) y = 1980, m = 1, d = 1, hh = mm = ss = 0;
    if (y > 2107) y = 2107, m = 12, d = 31, hh = 23, mm = 59, ss = 58;
    date = uint16_t(d + (m << 5) + (unsigned(y - 1980) << 9));
    time = uint16_t(ss / 2 + (mm << 5) + (hh << 11));
}

struct Entry {
    const char *name;
    size_t name_len;
    uint32_t mode;   // permission bits, 0..07777
    int64_t mtime;   // whole seconds
};

struct Record {      // what the central directory keeps of an entry
    std::string name;  // trimmed
    uint16_t flags = 0, date = 0, time = 0;
    uint32_t mode = 0, mtime32 = 0, crc = 0;
    uint64_t csize = 0, usize = 0, offset = 0;
};

// The entry's local header appended to `out` and its record started (CRC,
// sizes and offset come later).  Leading slashes are trimmed, as
// strings.TrimLeft(path, "/").  CDC_E_INVALID: a name empty after trimming,
// with a NUL or over 65,535 bytes; mode bits above 07777.
static inline int build_local(const Entry &e, std::vector<uint8_t> &out, Record &r)
{
    if (!e.name || e.mode > 07777u) return CDC_E_INVALID;
    const char *nm = e.name;
    size_t n = e.name_len;
    while (n && *nm == '/') ++nm, --n;
    if (n == 0 || n > kMax16 || memchr(nm, 0, n)) return CDC_E_INVALID;
    bool valid, require;
    detect_utf8(nm, n, valid, require);
    r = Record();
    r.name.assign(nm, n);
    r.flags = uint16_t(kFlagDescriptor | (valid && require ? kFlagUTF8 : 0));
    dos_time(e.mtime, r.date, r.time);
    r.mode = e.mode;
    r.mtime32 = uint32_t(uint64_t(e.mtime));
    put32(out, 0x04034B50u);
    put16(out, kVersion20);
    put16(out, r.flags);
    put16(out, kMethodDeflate);
    put16(out, r.time);
    put16(out, r.date);
    put32(out, 0);  // CRC-32 and the sizes: in the data descriptor
    put32(out, 0);
    put32(out, 0);
    put16(out, uint32_t(n));
    put16(out, kTimeExtra);
    out.insert(out.end(), nm, nm + n);
    put16(out, 0x5455);  // extended timestamp: modification time only
    put16(out, 5);
    out.push_back(1);
    put32(out, r.mtime32);
    return CDC_OK;
}

static inline bool is_zip64(const Record &r) { return r.csize >= kMax32 || r.usize >= kMax32; }

// The record's central directory header appended to `out`.
static inline void put_central(const Record &r, std::vector<uint8_t> &out)
{
    const bool z64 = is_zip64(r) || r.offset >= kMax32;
    put32(out, 0x02014B50u);
    put16(out, kCreator);
    put16(out, is_zip64(r) ? kVersion45 : kVersion20);
    put16(out, r.flags);
    put16(out, kMethodDeflate);
    put16(out, r.time);
    put16(out, r.date);
    put32(out, r.crc);
    put32(out, z64 ? kMax32 : r.csize);
    put32(out, z64 ? kMax32 : r.usize);
    put16(out, uint32_t(r.name.size()));
    put16(out, uint32_t(kTimeExtra + (z64 ? 28 : 0)));
    put16(out, 0);  // comment
    put16(out, 0);  // disk number
    put16(out, 0);  // internal attributes
    put32(out, uint64_t(0100000u | r.mode) << 16 | ((r.mode & 0200u) ? 0u : 1u));  // S_IFREG; MS-DOS read-only
    put32(out, z64 ? kMax32 : r.offset);
    out.insert(out.end(), r.name.begin(), r.name.end());
    if (z64) {
        put16(out, 0x0001);
        put16(out, 24);
        put64(out, r.usize);
        put64(out, r.csize);
        put64(out, r.offset);
    }
    put16(out, 0x5455);
    put16(out, 5);
    out.push_back(1);
    put32(out, r.mtime32);
}

// The end records of a directory of `records` headers, `size` bytes long, that
// starts at `offset`: the zip64 end record and its locator first when a count
// or an offset does not fit the plain one, which then holds the saturated values.
static inline void put_end(uint64_t records, uint64_t size, uint64_t offset, std::vector<uint8_t> &out)
{
    if (records >= kMax16 || size >= kMax32 || offset >= kMax32) {
        put32(out, 0x06064B50u);
        put64(out, kEnd64Len - 12);
        put16(out, kVersion45);
        put16(out, kVersion45);
        put32(out, 0);
        put32(out, 0);
        put64(out, records);
        put64(out, records);
        put64(out, size);
        put64(out, offset);
        put32(out, 0x07064B50u);
        put32(out, 0);
        put64(out, offset + size);
        put32(out, 1);
        records = kMax16;
        size = offset = kMax32;
    }
    put32(out, 0x06054B50u);
    put16(out, 0);
    put16(out, 0);
    put16(out, uint32_t(records));
    put16(out, uint32_t(records));
    put32(out, size);
    put32(out, offset);
    put16(out, 0);
}

// The whole tail: the directory at `offset` and the end records.
static inline void build_tail(const Record *recs, size_t n, uint64_t offset, std::vector<uint8_t> &out)
{
    const size_t at = out.size();
    for (size_t i = 0; i < n; ++i) put_central(recs[i], out);
    put_end(n, out.size() - at, offset, out);
}

// ---- batch planner -------------------------------------------------------------
// Items, in archive order: an entry's local header (whole: it never straddles
// a batch) and each of its chunk occurrences.  A batch holds at most `budget`
// bytes of them and always takes its first item.  The image a batch assembles
// is its file bytes back to back (aplan::Segment::dst_off; no headers, no
// padding); the headers travel in the batch's arena.  A file is one piece, or,
// when it does not fit the room left, several on chunk boundaries, one per
// batch; its last chunk is in its last piece, and a file with no bytes is one
// empty piece, first and last.  Distinct blobs are decoded once per batch, in
// order of first use.
struct Piece {
    uint32_t entry;        // the planned entry
    bool first, last;
    uint64_t img_off, len; // in the batch's image
    uint32_t hdr_off, hdr_len;  // in the batch's arena (first)
};
struct Batch {
    aplan::Batch a;        // blobs, segs (none from the arena), out_bytes: the image; a.arena stays empty
    std::vector<uint8_t> hdrs;
    std::vector<Piece> pieces;
    uint64_t used = 0;     // file bytes and headers: what the budget counts
};

static inline void plan(const aplan::File *files, size_t nfiles, uint64_t budget, std::vector<Batch> &out)
{
    out.clear();
    if (budget == 0) budget = 1;
    Batch cur;
    std::unordered_map<uint64_t, uint32_t> seen;
    auto close = [&] {
        out.push_back(std::move(cur));
        cur = Batch();
        seen.clear();
    };
    for (size_t fi = 0; fi < nfiles; ++fi) {
        const aplan::File &F = files[fi];
        if (cur.used != 0 && cur.used + F.hdr_len > budget) close();
        cur.pieces.push_back(Piece{uint32_t(fi), true, false, cur.a.out_bytes, 0, uint32_t(cur.hdrs.size()), uint32_t(F.hdr_len)});
        cur.hdrs.insert(cur.hdrs.end(), F.hdr, F.hdr + F.hdr_len);
        cur.used += F.hdr_len;
        for (uint64_t c = 0; c < F.nchunks; ++c) {
            const uint64_t len = F.len[c];
            if (!len) continue;
            if (cur.used != 0 && cur.used + len > budget) {  // the file goes on in the next batch
                close();
                cur.pieces.push_back(Piece{uint32_t(fi), false, false, 0, 0, 0, 0});
            }
            const uint64_t key = uint64_t(F.blob[c]) << 32 | len;
            auto it = seen.find(key);
            uint32_t local;
            if (it == seen.end()) {
                local = uint32_t(cur.a.blobs.size());
                seen.emplace(key, local);
                cur.a.blobs.push_back(aplan::Blob{F.blob[c], uint32_t(len), cur.a.plain_bytes});
                cur.a.plain_bytes += len;
            } else {
                local = it->second;
            }
            cur.a.segs.push_back(aplan::Segment{cur.a.blobs[local].off, len, cur.a.out_bytes, local, uint32_t(fi), false});
            cur.a.out_bytes += len;
            cur.used += len;
            cur.pieces.back().len += len;
        }
        cur.pieces.back().last = true;
    }
    if (!cur.pieces.empty()) close();
}

}  // namespace zplan
