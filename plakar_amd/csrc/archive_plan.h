// Host-only pieces of the archive path, shared by the library (cdc_archive.cpp)
// and the stand-alone sanitizer program tests/c/archive_plan_check.cpp:
//
//   * the tar layout of `plakar archive` (cmd/plakar/subcommands/archive/
//     archive.go:125-190 through Go's archive/tar Writer): a POSIX ustar header
//     block per entry, a PAX extended header before an entry that does not fit
//     one, file bytes, zeros to the next 512, and 1,024 zeros at the end
//     (tar.Writer.Close; no blocking factor);
//   * the batch planner of cdc_archive_run: restore's (restore_plan.h) over
//     the tar stream instead of the files: which blobs a batch decodes and
//     where every chunk occurrence, header block and padding run lands.
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "plakar_cdc.h"

namespace aplan {

constexpr uint64_t kBlock = 512;
constexpr size_t kNameSize = 100, kPrefixSize = 155;
constexpr uint64_t kOctal12Max = (1ull << 33) - 1;  // eleven octal digits: a size under 8 GiB, a time up to 2242
constexpr int kTypeFile = 0, kTypeDir = 1;          // CDC_ARCHIVE_FILE, CDC_ARCHIVE_DIR

struct Entry {
    const char *name;
    size_t name_len;
    int type;        // kTypeFile or kTypeDir
    uint32_t mode;   // permission bits, 0..07777
    int64_t mtime;   // whole seconds
    uint64_t size;   // a directory's is 0
};

static inline bool is_ascii(const char *s, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (uint8_t(s[i]) >= 0x80) return false;
    return true;
}

// archive/tar's splitUSTARPath: a name over 100 bytes as prefix (<= 155) "/"
// name (<= 100), cut at the last slash that leaves both in range.
static inline bool split_ustar(const char *name, size_t n, size_t &plen)
{
    if (n <= kNameSize || !is_ascii(name, n)) return false;
    size_t length = n;
    if (length > kPrefixSize + 1) length = kPrefixSize + 1;
    else if (name[length - 1] == '/') --length;
    size_t i = length;
    while (i > 0 && name[i - 1] != '/') --i;
    if (i == 0) return false;  // no slash
    --i;                       // the slash's index
    const size_t nlen = n - i - 1;
    if (i == 0 || nlen > kNameSize || nlen == 0 || i > kPrefixSize) return false;
    plen = i;
    return true;
}

// The field's octal digits and a NUL (archive/tar formatOctal); 0 when the
// value does not fit, as Go leaves it beside a PAX record.
static inline void put_octal(uint8_t *f, size_t width, uint64_t v, bool fits)
{
    if (!fits) v = 0;
    for (size_t i = width - 1; i-- > 0;) {
        f[i] = uint8_t('0' + (v & 7u));
        v >>= 3;
    }
    f[width - 1] = 0;
}

static inline void put_checksum(uint8_t *blk)
{
    memset(blk + 148, ' ', 8);
    uint32_t sum = 0;
    for (size_t i = 0; i < kBlock; ++i) sum += blk[i];
    put_octal(blk + 148, 7, sum, true);  // six digits and a NUL; the space stays
}

static inline void put_magic(uint8_t *blk)
{
    memcpy(blk + 257, "ustar\0" "00", 8);
}

// "%d %s=%s\n", the length counting itself.
static inline std::string pax_record(const char *key, const std::string &val)
{
    const size_t body = 1 + strlen(key) + 1 + val.size() + 1;
    size_t n = body + 1;
    for (;;) {
        char d[24];
        const size_t digits = size_t(snprintf(d, sizeof(d), "%zu", n));
        if (digits + body == n) break;
        n = digits + body;
    }
    return std::to_string(n) + " " + key + "=" + val + "\n";
}

// The entry's header blocks appended to `out`: one block, or, where a field
// does not fit it, a PAX extended header (typeflag x: its block and its
// records padded to 512) and then the block, with what fits.  The records are
// the ones archive/tar chooses: path (no valid split, over 255 bytes or a byte
// >= 0x80), size (8 GiB or more), mtime (negative or past eleven octal
// digits).  CDC_E_INVALID: no name, a NUL in the name, a type that is neither
// file nor directory, mode bits above 07777.
static inline int build_header(const Entry &e, std::vector<uint8_t> &out)
{
    if (!e.name || e.name_len == 0 || memchr(e.name, 0, e.name_len)) return CDC_E_INVALID;
    if ((e.type != kTypeFile && e.type != kTypeDir) || e.mode > 07777u) return CDC_E_INVALID;
    const uint64_t size = e.type == kTypeDir ? 0 : e.size;
    size_t plen = 0;
    const bool ascii = is_ascii(e.name, e.name_len);
    const bool split = split_ustar(e.name, e.name_len, plen);
    const bool pax_path = !ascii || (e.name_len > kNameSize && !split);
    const bool pax_size = size > kOctal12Max;
    const bool pax_mtime = e.mtime < 0 || uint64_t(e.mtime) > kOctal12Max;
    const bool pax = pax_path || pax_size || pax_mtime;
    if (pax) {
        std::string recs;  // keys in sorted order
        if (pax_mtime) recs += pax_record("mtime", std::to_string((long long)e.mtime));
        if (pax_path) recs += pax_record("path", std::string(e.name, e.name_len));
        if (pax_size) recs += pax_record("size", std::to_string((unsigned long long)size));
        // the extended header's own name: dir/PaxHeaders.0/file, ASCII only, 100 bytes at most
        size_t slash = e.name_len;
        while (slash > 0 && e.name[slash - 1] != '/') --slash;
        std::string xn(e.name, slash);
        xn += "PaxHeaders.0";
        if (slash < e.name_len) xn += "/" + std::string(e.name + slash, e.name_len - slash);
        std::string xa;
        for (char c : xn)
            if (uint8_t(c) < 0x80) xa.push_back(c);
        if (xa.size() > kNameSize) xa.resize(kNameSize);
        while (!xa.empty() && xa.back() == '/') xa.pop_back();
        const size_t at = out.size();
        out.resize(at + kBlock + (recs.size() + kBlock - 1) / kBlock * kBlock, 0);
        uint8_t *x = out.data() + at;
        memcpy(x, xa.data(), xa.size());
        put_octal(x + 100, 8, 0, true);
        put_octal(x + 108, 8, 0, true);
        put_octal(x + 116, 8, 0, true);
        put_octal(x + 124, 12, recs.size(), true);
        put_octal(x + 136, 12, 0, true);
        x[156] = 'x';
        put_magic(x);
        put_checksum(x);
        memcpy(x + kBlock, recs.data(), recs.size());
    }
    const size_t at = out.size();
    out.resize(at + kBlock, 0);
    uint8_t *b = out.data() + at;
    if (!pax && split) {
        memcpy(b + 345, e.name, plen);
        memcpy(b, e.name + plen + 1, e.name_len - plen - 1);
    } else {
        size_t k = 0;  // what fits of the name's ASCII bytes; the PAX path overrides it
        for (size_t i = 0; i < e.name_len && k < kNameSize; ++i)
            if (uint8_t(e.name[i]) < 0x80) b[k++] = uint8_t(e.name[i]);
    }
    put_octal(b + 100, 8, e.mode, true);
    put_octal(b + 108, 8, 0, true);   // uid
    put_octal(b + 116, 8, 0, true);   // gid
    put_octal(b + 124, 12, size, !pax_size);
    put_octal(b + 136, 12, uint64_t(e.mtime), !pax_mtime);
    b[156] = e.type == kTypeDir ? '5' : '0';
    put_magic(b);
    put_octal(b + 329, 8, 0, true);   // devmajor, devminor: zero, as archive/tar formats them
    put_octal(b + 337, 8, 0, true);
    put_checksum(b);
    return CDC_OK;
}

// ---- batch planner -------------------------------------------------------------
// The tar stream is laid into batches of at most `budget` bytes of it (a batch
// always takes its first item, so one item larger than the budget exceeds it).
// Items, in stream order: an entry's header blocks (whole: a header never
// straddles a batch), each chunk occurrence (a file larger than a batch goes
// in pieces on chunk boundaries), the file's padding run (after its last
// chunk, at the next batch's start when it does not fit), and the two closing
// zero blocks.  A segment's source is the batch's plaintext buffer (distinct
// blobs back to back, in order of first use, as restore's) or the batch's
// arena: its header blocks back to back, then one zero block.
struct File {              // an entry as the planner sees it
    const uint8_t *hdr;    // its header blocks (build_header)
    uint64_t hdr_len;
    uint64_t nchunks;
    const uint32_t *blob;  // chunk i's blob id (equal for equal checksums)
    const uint32_t *len;   // chunk i's recorded Length
};
struct Segment {
    uint64_t src_off;      // in the plaintext buffer, or in the arena
    uint64_t len;
    uint64_t dst_off;      // in the batch's image
    uint32_t blob;         // index into Batch::blobs (plaintext segments)
    uint32_t entry;        // the planned entry it belongs to (the closing blocks: the entry count)
    bool arena;
};
struct Blob {
    uint32_t id;
    uint32_t len;
    uint64_t off;
};
struct Batch {
    std::vector<Blob> blobs;
    std::vector<Segment> segs;
    std::vector<uint8_t> arena;  // header blocks, then kBlock zeros
    uint64_t out_bytes = 0;
    uint64_t plain_bytes = 0;
    uint64_t stream_off = 0;     // where the image starts in the tar stream
};

static inline void plan(const File *files, size_t nfiles, uint64_t budget, std::vector<Batch> &out)
{
    out.clear();
    if (budget == 0) budget = 1;
    Batch cur;
    uint64_t stream = 0;
    std::unordered_map<uint64_t, uint32_t> seen;
    auto close = [&] {
        // the zero block comes last: the zero segments' offsets are moved behind the headers
        const uint64_t z = cur.arena.size();
        for (Segment &s : cur.segs)
            if (s.arena && s.src_off == UINT64_MAX) s.src_off = z;
        cur.arena.resize(size_t(z + kBlock), 0);
        stream += cur.out_bytes;
        out.push_back(std::move(cur));
        cur = Batch();
        cur.stream_off = stream;
        seen.clear();
    };
    auto room = [&](uint64_t len) {
        if (cur.out_bytes != 0 && cur.out_bytes + len > budget) close();
    };
    auto zeros = [&](uint64_t len, uint32_t entry) {  // len <= kBlock
        room(len);
        cur.segs.push_back(Segment{UINT64_MAX, len, cur.out_bytes, 0, entry, true});
        cur.out_bytes += len;
    };
    for (size_t fi = 0; fi < nfiles; ++fi) {
        const File &F = files[fi];
        room(F.hdr_len);
        cur.segs.push_back(Segment{cur.arena.size(), F.hdr_len, cur.out_bytes, 0, uint32_t(fi), true});
        cur.arena.insert(cur.arena.end(), F.hdr, F.hdr + F.hdr_len);
        cur.out_bytes += F.hdr_len;
        uint64_t size = 0;
        for (uint64_t c = 0; c < F.nchunks; ++c) {
            const uint64_t len = F.len[c];
            size += len;
            if (!len) continue;
            room(len);
            const uint64_t key = uint64_t(F.blob[c]) << 32 | len;
            auto it = seen.find(key);
            uint32_t local;
            if (it == seen.end()) {
                local = uint32_t(cur.blobs.size());
                seen.emplace(key, local);
                cur.blobs.push_back(Blob{F.blob[c], uint32_t(len), cur.plain_bytes});
                cur.plain_bytes += len;
            } else {
                local = it->second;
            }
            cur.segs.push_back(Segment{cur.blobs[local].off, len, cur.out_bytes, local, uint32_t(fi), false});
            cur.out_bytes += len;
        }
        if (size % kBlock) zeros(kBlock - size % kBlock, uint32_t(fi));
    }
    zeros(kBlock, uint32_t(nfiles));
    zeros(kBlock, uint32_t(nfiles));
    close();
}

}  // namespace aplan
