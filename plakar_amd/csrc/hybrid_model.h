// The device/host split model of the hybrid digests, shared by
// cdc_chunk_digests_hybrid (cdc_api.cpp) and the check pipeline
// (check_plan.h).  Host only, no library state: the host's SHA-256 rate is an
// argument.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace hybrid {

constexpr double kDevPerByte = 2.05e-6 / 64.0;  // one round wave's chain: ~2.05 us per 64-B block
constexpr double kPcie = 40e9;                  // device-to-host bytes per second

// The host's share: the longest messages, as many as balance the two sides
// (the count k of `sorted_desc`, lengths longest first, that go to the host).
// Device: the longest message left to it (its chain).  Host: its messages come
// back over PCIe in `parts` pieces while the threads hash the pieces already
// landed, so its time is the first piece's copy plus the slower of the copy of
// the rest and the hashing (bytes over `threads` cores at `rate` bytes per
// second, the longest message's own chain at least).
inline size_t split(const std::vector<uint64_t> &sorted_desc, int threads, int parts, double rate)
{
    double best = 1e30, bytes = 0;
    size_t k_best = 0;
    const size_t n = std::min<size_t>(sorted_desc.size(), 1u << 16);
    for (size_t k = 0; k <= n; ++k) {
        const double dev = k < sorted_desc.size() ? double(sorted_desc[k]) * kDevPerByte : 0.0;
        const double host =
            k ? bytes / double(std::min<size_t>(size_t(parts), k)) / kPcie +
                    std::max({double(sorted_desc[0]) / rate, bytes / (threads * rate), bytes / kPcie})
              : 0.0;
        const double t = std::max(dev, host);
        if (t < best) {
            best = t;
            k_best = k;
        }
        if (k < n) bytes += double(sorted_desc[k]);
    }
    return k_best;
}

}  // namespace hybrid
