// The archive path's host-only header (plakar_amd/csrc/archive_plan.h) under the
// address and undefined-behaviour sanitizers (tests/test_archive_cpu.py builds
// and runs it, and judges what it prints):
//
//   archive_plan_check SPEC OUT
//
// SPEC, one item per line:
//   H <type> <mode> <mtime> <size> <name in hex>        a header case
//   B <budget>                                          the budget of the plan that follows
//   E <type> <mode> <mtime> <name in hex> <nchunks> {<blob id> <length>}   an entry of the plan
// Printed:
//   H <index> <status> <header blocks in hex>
//   P <batch> <stream_off> <out_bytes> <plain_bytes> <blobs> <arena bytes>
//   S <batch> <arena 0/1> <src_off> <len> <dst_off> <entry> <blob id or -1>
// OUT receives the plan's batches' images back to back, assembled here from
// the segments the way cdc_assemble_device does, blob `id` of length n being
// the bytes (id * 131 + j * 7 + (j >> 8)) & 255.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../plakar_amd/csrc/archive_plan.h"

static std::string unhex(const std::string &h)
{
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back(char(strtoul(h.substr(i, 2).c_str(), nullptr, 16)));
    return s;
}

struct PlanEntry {
    std::string name;
    int type;
    uint32_t mode;
    int64_t mtime;
    std::vector<uint32_t> blob, len;
    std::vector<uint8_t> hdr;
};

int main(int argc, char **argv)
{
    if (argc != 3) {
        puts("usage: archive_plan_check SPEC OUT");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    uint64_t budget = 0;
    std::vector<PlanEntry> ents;
    int hi = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        if (kind == "H") {
            int type;
            uint32_t mode;
            long long mtime;
            unsigned long long size;
            std::string hex;
            ss >> type >> std::oct >> mode >> std::dec >> mtime >> size >> hex;
            const std::string name = hex == "-" ? std::string() : unhex(hex);
            std::vector<uint8_t> out;
            const aplan::Entry e{name.data(), name.size(), type, mode, int64_t(mtime), uint64_t(size)};
            const int st = aplan::build_header(e, out);
            printf("H %d %d ", hi++, st);
            for (uint8_t b : out) printf("%02x", b);
            printf("\n");
        } else if (kind == "B") {
            ss >> budget;
        } else if (kind == "E") {
            PlanEntry P;
            std::string hex;
            long long mtime;
            size_t n;
            ss >> P.type >> std::oct >> P.mode >> std::dec >> mtime >> hex >> n;
            P.mtime = mtime;
            P.name = unhex(hex);
            for (size_t i = 0; i < n; ++i) {
                uint32_t id, len;
                ss >> id >> len;
                P.blob.push_back(id);
                P.len.push_back(len);
            }
            ents.push_back(std::move(P));
        }
    }
    std::vector<aplan::File> files;
    for (PlanEntry &P : ents) {
        uint64_t size = 0;
        for (uint32_t l : P.len) size += l;
        const aplan::Entry e{P.name.data(), P.name.size(), P.type, P.mode, P.mtime, size};
        if (aplan::build_header(e, P.hdr) != CDC_OK) {
            puts("FAIL a plan entry's header");
            return 1;
        }
    }
    for (PlanEntry &P : ents) files.push_back(aplan::File{P.hdr.data(), P.hdr.size(), P.blob.size(), P.blob.data(), P.len.data()});
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (budget) {
        std::vector<aplan::Batch> batches;
        aplan::plan(files.data(), files.size(), budget, batches);
        for (size_t k = 0; k < batches.size(); ++k) {
            const aplan::Batch &B = batches[k];
            printf("P %zu %llu %llu %llu %zu %zu\n", k, (unsigned long long)B.stream_off, (unsigned long long)B.out_bytes,
                   (unsigned long long)B.plain_bytes, B.blobs.size(), B.arena.size());
            // the plaintext buffer as Decode leaves it: the distinct blobs back to back (exactly sized: the
            // sanitizer sees any segment that reaches past it)
            std::vector<uint8_t> plain(B.plain_bytes), image(B.out_bytes, 0xA5);
            for (const aplan::Blob &b : B.blobs) {
                if (b.off + b.len > plain.size()) {
                    puts("FAIL a blob past the plaintext buffer");
                    return 1;
                }
                for (uint32_t j = 0; j < b.len; ++j) plain[b.off + j] = uint8_t(b.id * 131u + j * 7u + (j >> 8));
            }
            uint64_t at = 0;
            for (const aplan::Segment &S : B.segs) {
                printf("S %zu %d %llu %llu %llu %u %lld\n", k, int(S.arena), (unsigned long long)S.src_off,
                       (unsigned long long)S.len, (unsigned long long)S.dst_off, S.entry,
                       S.arena ? -1ll : (long long)B.blobs[S.blob].id);
                const std::vector<uint8_t> &src = S.arena ? B.arena : plain;
                if (S.dst_off != at || S.src_off + S.len > src.size() || S.dst_off + S.len > image.size()) {
                    puts("FAIL a segment out of range or out of order");
                    return 1;
                }
                memcpy(image.data() + S.dst_off, src.data() + S.src_off, S.len);
                at += S.len;
            }
            if (at != B.out_bytes) {
                puts("FAIL the segments do not cover the image");
                return 1;
            }
            fwrite(image.data(), 1, image.size(), f);
        }
    }
    fclose(f);
    puts("ok");
    return 0;
}
