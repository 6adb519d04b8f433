// The packfile locator of the runs that read blobs by checksum (restore, archive):
// registered packfiles, in memory or by path, and checksum -> (packfile,
// offset, length) for every TYPE_CHUNK row (state.GetSubpartForBlob,
// repository/repository.go:449-466); a checksum already there keeps its first
// location.  Sync registers packfiles the same way and keeps their whole
// indexes instead (keep_rows).  Host only.
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "cdc_hostutil.h"
#include "cdc_internal.h"
#include "restore_plan.h"

namespace cdc {

struct Sum {
    uint8_t b[32];
    bool operator==(const Sum &o) const { return std::memcmp(b, o.b, 32) == 0; }
};
struct SumHash {  // the checksums are SHA-256: any eight bytes are a hash
    size_t operator()(const Sum &s) const
    {
        uint64_t v;
        std::memcpy(&v, s.b, 8);
        return size_t(v);
    }
};

struct Locator {
    struct Pack {
        const uint8_t *mem;  // the caller's buffer, or NULL: read from path
        std::string path;
        uint64_t len;
    };
    struct Loc {
        uint32_t pack, offset, length;
    };
    std::vector<Pack> packs;
    std::unordered_map<Sum, uint32_t, SumHash> index;  // checksum -> blob id
    std::vector<Loc> locs;                             // by blob id
    std::vector<Sum> sums;                             // by blob id
    // Sync walks every row of every type in index order and looks nothing up
    // by checksum: with keep_rows each packfile's whole index is kept in
    // rows[pack] and the checksum index above stays empty.
    bool keep_rows = false;
    std::vector<std::vector<cdc_packfile_row>> rows;

    static void sha(const void *data, size_t n, uint8_t out[32]) { cdc::sha256(data, n, out); }

    void add_rows(Pack &&P, const std::vector<cdc_packfile_row> &rows)
    {
        if (keep_rows) {  // both lists grow or neither does
            packs.reserve(packs.size() + 1);
            this->rows.push_back(rows);
            packs.push_back(std::move(P));
            return;
        }
        const uint32_t pack = uint32_t(packs.size());
        packs.push_back(std::move(P));
        for (const cdc_packfile_row &r : rows) {
            if (r.type != rplan::kTypeChunk) continue;
            Sum s;
            std::memcpy(s.b, r.checksum, 32);
            if (index.emplace(s, uint32_t(locs.size())).second) {
                locs.push_back(Loc{pack, r.offset, r.length});
                sums.push_back(s);
            }
        }
    }
    // CDC_OK, CDC_E_CORRUPT.  `bytes` stays valid while the locator is used.
    int add_memory(const uint8_t *bytes, uint64_t len)
    {
        cdc_packfile_footer f;
        int st = rplan::parse_packfile(bytes, len, sha, &f, nullptr, 0);
        if (st != CDC_OK) return st;
        std::vector<cdc_packfile_row> rows(f.count);
        st = rplan::parse_packfile(bytes, len, sha, &f, rows.data(), rows.size());
        if (st != CDC_OK) return st;
        add_rows(Pack{bytes, std::string(), len}, rows);
        return CDC_OK;
    }
    // CDC_OK, CDC_E_IO, CDC_E_CORRUPT: the footer and the index are read now, blob ranges during a run.
    int add_path(const char *path)
    {
        const int fd = open(path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) return CDC_E_IO;
        int st = CDC_OK;
        struct stat sb;
        if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
            st = CDC_E_IO;
        } else if (uint64_t(sb.st_size) < rplan::kFooterBytes) {
            st = CDC_E_CORRUPT;
        } else {
            const uint64_t len = uint64_t(sb.st_size);
            uint8_t tail[rplan::kFooterBytes];
            cdc_packfile_footer f;
            if (!pread_all(fd, tail, sizeof(tail), len - sizeof(tail))) st = CDC_E_IO;
            if (st == CDC_OK) st = rplan::parse_footer(tail, len, &f);
            if (st == CDC_OK) {
                std::vector<uint8_t> idx(size_t(rplan::kRowBytes * f.count) + 1);
                std::vector<cdc_packfile_row> rows(f.count);
                if (!pread_all(fd, idx.data(), rplan::kRowBytes * f.count, f.index_offset)) st = CDC_E_IO;
                if (st == CDC_OK) st = rplan::parse_index(idx.data(), f, sha, rows.data(), rows.size());
                if (st == CDC_OK) add_rows(Pack{nullptr, std::string(path), len}, rows);
            }
        }
        close(fd);
        return st;
    }
};

}  // namespace cdc
