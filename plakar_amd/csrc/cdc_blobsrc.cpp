// cdc_blobsrc.h: layout, threaded read and checksum lookup.  Host only.
#include "cdc_blobsrc.h"

#include <fcntl.h>
#include <unistd.h>

#include <cstring>
#include <unordered_map>

namespace cdc {

uint64_t lay_out(const Span *spans, size_t n, std::vector<uint64_t> &eoff, std::vector<uint64_t> &elen)
{
    eoff.resize(n);
    elen.resize(n);
    uint64_t total = 0;
    for (size_t b = 0; b < n; ++b) {
        eoff[b] = total;
        elen[b] = spans[b].length;
        total += spans[b].length;
    }
    return total;
}

void read_spans(const Locator &loc, const Span *spans, size_t n, const uint64_t *eoff, uint8_t *dst, int threads,
                int32_t *pre)
{
    std::fill(pre, pre + n, int32_t(CDC_OK));
    if (!dst) return;
    std::unordered_map<uint32_t, int> fds;  // the packfiles this batch reads by path, open for the batch
    struct Close {
        std::unordered_map<uint32_t, int> &fds;
        ~Close()
        {
            for (auto &f : fds)
                if (f.second >= 0) close(f.second);
        }
    } closer{fds};
    for (size_t b = 0; b < n; ++b) {
        const Locator::Pack &P = loc.packs[spans[b].pack];
        if (!P.mem && !fds.count(spans[b].pack)) {
            fds[spans[b].pack] = -1;  // the entry first: a throwing insert leaves no descriptor behind
            fds[spans[b].pack] = open(P.path.c_str(), O_RDONLY | O_CLOEXEC);
        }
    }
    parallel_for(threads, n, [&](size_t b) {
        const Span &S = spans[b];
        const Locator::Pack &P = loc.packs[S.pack];
        if (P.mem) {
            if (S.length) std::memcpy(dst + eoff[b], P.mem + S.offset, S.length);
            return;
        }
        const int fd = fds.find(S.pack)->second;
        if (fd < 0 || !pread_all(fd, dst + eoff[b], S.length, S.offset)) pre[b] = CDC_E_IO;
    });
}

int64_t resolve(const Locator &loc, const uint8_t *checksums, uint64_t nchunks, uint32_t *ids)
{
    for (uint64_t c = 0; c < nchunks; ++c) {
        Sum s;
        std::memcpy(s.b, checksums + 32 * c, 32);
        const auto it = loc.index.find(s);
        if (it == loc.index.end()) return int64_t(c);
        ids[c] = it->second;
    }
    return -1;
}

}  // namespace cdc
