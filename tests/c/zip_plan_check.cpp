// The zip format's host-only header (plakar_amd/csrc/zip_plan.h) under the
// address and undefined-behaviour sanitizers (tests/test_archive_zip_cpu.py
// builds and runs it, and judges what it prints):
//
//   zip_plan_check SPEC OUT
//
// SPEC, one item per line:
//   H <mode> <mtime> <name in hex>                      a local header case
//   U <name in hex>                                     detect_utf8 alone
//   B <budget>                                          the budget of the plan that follows
//   E <mode> <mtime> <name in hex> <nchunks> {<blob id> <length>}   an entry of the plan
//   R <mode> <mtime> <name in hex> <crc> <csize> <usize> <offset>   a synthetic directory record
//   N <count>                                           <count> more records, generated: "e%07d", 2 and 0 bytes
//   D <offset>                                          the tail (directory at <offset>, end records) of the records
// Printed:
//   H <index> <status> <flags> <date> <time> <local header in hex>
//   U <valid> <require>
//   P <batch> <used> <image bytes> <plain bytes> <blobs> <header arena bytes>
//   S <batch> <src_off> <len> <dst_off> <entry> <blob id>
//   Q <batch> <entry> <first> <last> <img_off> <len> <hdr_off> <hdr_len>
// OUT receives, for a plan, per batch an 8-byte length and the header arena,
// an 8-byte length and the image, assembled here from the segments the way
// cdc_assemble_device does (blob `id` of length n being the bytes
// (id * 131 + j * 7 + (j >> 8)) & 255); for a D line, the tail.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../plakar_amd/csrc/zip_plan.h"

static std::string unhex(const std::string &h)
{
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back(char(strtoul(h.substr(i, 2).c_str(), nullptr, 16)));
    return s;
}

struct PlanEntry {
    std::string name;
    uint32_t mode;
    int64_t mtime;
    std::vector<uint32_t> blob, len;
    std::vector<uint8_t> hdr;
};

static void put_len(FILE *f, uint64_t n)
{
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = uint8_t(n >> (8 * i));
    fwrite(b, 1, 8, f);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        puts("usage: zip_plan_check SPEC OUT");
        return 2;
    }
    std::ifstream in(argv[1]);
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    std::string line;
    uint64_t budget = 0;
    std::vector<PlanEntry> ents;
    std::vector<zplan::Record> recs;
    int hi = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, hex;
        ss >> kind;
        if (kind == "H") {
            uint32_t mode;
            long long mtime;
            ss >> std::oct >> mode >> std::dec >> mtime >> hex;
            const std::string name = unhex(hex);
            std::vector<uint8_t> out;
            zplan::Record R;
            const int st = zplan::build_local(zplan::Entry{name.data(), name.size(), mode, int64_t(mtime)}, out, R);
            printf("H %d %d %u %u %u ", hi++, st, unsigned(R.flags), unsigned(R.date), unsigned(R.time));
            for (uint8_t b : out) printf("%02x", b);
            printf("\n");
        } else if (kind == "U") {
            ss >> hex;
            const std::string name = unhex(hex);
            bool valid, require;
            zplan::detect_utf8(name.data(), name.size(), valid, require);
            printf("U %d %d\n", int(valid), int(require));
        } else if (kind == "B") {
            ss >> budget;
        } else if (kind == "E") {
            PlanEntry P;
            long long mtime;
            size_t n;
            ss >> std::oct >> P.mode >> std::dec >> mtime >> hex >> n;
            P.mtime = mtime;
            P.name = unhex(hex);
            for (size_t i = 0; i < n; ++i) {
                uint32_t id, len;
                ss >> id >> len;
                P.blob.push_back(id);
                P.len.push_back(len);
            }
            ents.push_back(std::move(P));
        } else if (kind == "R") {
            uint32_t mode;
            long long mtime;
            unsigned long long crc, csize, usize, offset;
            ss >> std::oct >> mode >> std::dec >> mtime >> hex >> crc >> csize >> usize >> offset;
            const std::string name = unhex(hex);
            std::vector<uint8_t> out;
            zplan::Record R;
            if (zplan::build_local(zplan::Entry{name.data(), name.size(), mode, int64_t(mtime)}, out, R) != CDC_OK) {
                puts("FAIL a record's header");
                return 1;
            }
            R.crc = uint32_t(crc);
            R.csize = csize;
            R.usize = usize;
            R.offset = offset;
            recs.push_back(std::move(R));
        } else if (kind == "N") {
            size_t n;
            ss >> n;
            for (size_t i = 0; i < n; ++i) {
                char nm[16];
                snprintf(nm, sizeof(nm), "e%07zu", recs.size());
                std::vector<uint8_t> out;
                zplan::Record R;
                if (zplan::build_local(zplan::Entry{nm, strlen(nm), 0644, 1700000000}, out, R) != CDC_OK) return 1;
                R.csize = 2;
                R.offset = uint64_t(recs.size()) * 64;
                recs.push_back(std::move(R));
            }
        } else if (kind == "D") {
            unsigned long long offset;
            ss >> offset;
            std::vector<uint8_t> tail;
            zplan::build_tail(recs.data(), recs.size(), offset, tail);
            fwrite(tail.data(), 1, tail.size(), f);
        }
    }
    if (budget) {
        for (PlanEntry &P : ents)
            if (zplan::Record R; zplan::build_local(zplan::Entry{P.name.data(), P.name.size(), P.mode, P.mtime}, P.hdr, R) != CDC_OK) {
                puts("FAIL a plan entry's header");
                return 1;
            }
        std::vector<aplan::File> files;
        for (PlanEntry &P : ents) files.push_back(aplan::File{P.hdr.data(), P.hdr.size(), P.blob.size(), P.blob.data(), P.len.data()});
        std::vector<zplan::Batch> batches;
        zplan::plan(files.data(), files.size(), budget, batches);
        for (size_t k = 0; k < batches.size(); ++k) {
            const zplan::Batch &B = batches[k];
            printf("P %zu %llu %llu %llu %zu %zu\n", k, (unsigned long long)B.used, (unsigned long long)B.a.out_bytes,
                   (unsigned long long)B.a.plain_bytes, B.a.blobs.size(), B.hdrs.size());
            // the plaintext buffer as Decode leaves it, exactly sized: the sanitizer sees any segment past it
            std::vector<uint8_t> plain(B.a.plain_bytes), image(B.a.out_bytes, 0xA5);
            for (const aplan::Blob &b : B.a.blobs) {
                if (b.off + b.len > plain.size()) {
                    puts("FAIL a blob past the plaintext buffer");
                    return 1;
                }
                for (uint32_t j = 0; j < b.len; ++j) plain[b.off + j] = uint8_t(b.id * 131u + j * 7u + (j >> 8));
            }
            uint64_t at = 0;
            for (const aplan::Segment &S : B.a.segs) {
                printf("S %zu %llu %llu %llu %u %u\n", k, (unsigned long long)S.src_off, (unsigned long long)S.len,
                       (unsigned long long)S.dst_off, S.entry, B.a.blobs[S.blob].id);
                if (S.arena || S.dst_off != at || S.src_off + S.len > plain.size() || S.dst_off + S.len > image.size()) {
                    puts("FAIL a segment out of range or out of order");
                    return 1;
                }
                if (S.len) memcpy(image.data() + S.dst_off, plain.data() + S.src_off, S.len);
                at += S.len;
            }
            if (at != B.a.out_bytes || !B.a.arena.empty()) {
                puts("FAIL the segments do not cover the image");
                return 1;
            }
            for (const zplan::Piece &Q : B.pieces) {
                printf("Q %zu %u %d %d %llu %llu %u %u\n", k, Q.entry, int(Q.first), int(Q.last), (unsigned long long)Q.img_off,
                       (unsigned long long)Q.len, Q.hdr_off, Q.hdr_len);
                if (Q.img_off + Q.len > image.size() || (Q.first && uint64_t(Q.hdr_off) + Q.hdr_len > B.hdrs.size())) {
                    puts("FAIL a piece out of range");
                    return 1;
                }
            }
            put_len(f, B.hdrs.size());
            if (!B.hdrs.empty()) fwrite(B.hdrs.data(), 1, B.hdrs.size(), f);
            put_len(f, image.size());
            if (!image.empty()) fwrite(image.data(), 1, image.size(), f);
        }
    }
    fclose(f);
    puts("ok");
    return 0;
}
