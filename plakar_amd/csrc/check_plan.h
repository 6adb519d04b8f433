// Host-only planning of the check path (cdc_check.cpp, cdc_object_digests_device),
// shared with the stand-alone sanitizer program tests/c/check_plan_check.cpp:
//
//   * the run and seam planner of k_object_digest: an object is the
//     concatenation of its segments of one source buffer; the kernel walks
//     *runs*, aligned-dword streams of which every one but an object's last
//     holds a multiple of 64 bytes;
//   * the split of a batch's objects between the device and the host.
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "hybrid_model.h"
#include "sha_blocks.h"

namespace cplan {

constexpr uint64_t kSeam = 1ull << 63;  // Run::src: an offset into the seam area, not into the source

struct Run {
    uint64_t src;    // byte offset in the source buffer, or kSeam | offset in the seam area
    uint64_t bytes;  // a multiple of 64 in every run but an object's last
};
struct Copy {        // seam area [dst_off, + len) = source [src_off, + len); dst_off ascending, disjoint
    uint64_t src_off, len, dst_off;
};
struct Runs {
    std::vector<Run> runs;
    std::vector<uint64_t> run0;   // n + 1: object i's runs are [run0[i], run0[i + 1]), at least one
    std::vector<uint64_t> total;  // n: the object's message length
    std::vector<Copy> copies;
    uint64_t seam_bytes = 0;      // the seam area: the end of the last copy
};

// Every segment inside [0, len), the object list ascending to nsegs, every
// object's total a length SHA-256 can state (shab::kMaxTotal).
inline bool segments_valid(const uint64_t *seg_off, const uint64_t *seg_len, uint64_t nsegs, const uint64_t *obj_seg0,
                           uint64_t n, uint64_t len)
{
    for (uint64_t s = 0; s < nsegs; ++s)
        if (seg_off[s] > len || seg_len[s] > len - seg_off[s]) return false;
    for (uint64_t i = 0; i < n; ++i)
        if (obj_seg0[i] > obj_seg0[i + 1]) return false;
    if (obj_seg0[n] != nsegs) return false;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t t = 0;
        for (uint64_t s = obj_seg0[i]; s < obj_seg0[i + 1]; ++s) {
            if (seg_len[s] > shab::kMaxTotal - t) return false;
            t += seg_len[s];
        }
    }
    return true;
}

// Runs and seam copies of n objects (segments_valid holds).  A 64-byte block
// of the message that lies inside one segment is *plain*: consecutive plain
// blocks of a segment are one run that points at the segment's bytes, and so
// is everything from a block boundary on in the object's last segment with
// bytes (the last run may end anywhere).  A block that a segment boundary
// cuts is a *seam* block: its parts are copied into the seam area, one copy
// per part, and consecutive seam blocks are one run there.  An object's seam
// blocks start on a 64-byte boundary of the area.  An object without bytes
// gets one empty run.
inline void plan_runs(const uint64_t *seg_off, const uint64_t *seg_len, const uint64_t *obj_seg0, uint64_t n, Runs &out)
{
    out.runs.clear();
    out.copies.clear();
    out.run0.assign(size_t(n) + 1, 0);
    out.total.assign(size_t(n), 0);
    uint64_t seam = 0;  // the area's fill
    for (uint64_t i = 0; i < n; ++i) {
        out.run0[size_t(i)] = out.runs.size();
        const size_t first_run = out.runs.size();
        uint64_t s_last = obj_seg0[i + 1];  // the last segment with bytes
        while (s_last > obj_seg0[i] && seg_len[s_last - 1] == 0) --s_last;
        uint64_t total = 0;
        uint32_t fill = 0;  // bytes in the open seam block
        bool seam_open = false;  // the object's last run is a seam run that ends at `seam`
        seam = (seam + 63) & ~63ull;
        auto to_seam = [&](uint64_t off, uint64_t len) {
            out.copies.push_back(Copy{off, len, seam});
            if (seam_open) {
                out.runs.back().bytes += len;
            } else {
                out.runs.push_back(Run{kSeam | seam, len});
                seam_open = true;
            }
            seam += len;
        };
        for (uint64_t s = obj_seg0[i]; s < s_last; ++s) {
            uint64_t off = seg_off[s], len = seg_len[s];
            total += len;
            if (len == 0) continue;
            if (fill) {  // the open seam block takes the segment's head
                const uint64_t t = std::min<uint64_t>(len, 64u - fill);
                to_seam(off, t);
                fill = (fill + uint32_t(t)) & 63u;
                off += t;
                len -= t;
            }
            if (len == 0) continue;
            // on a block boundary of the message
            const uint64_t plain = s + 1 == s_last ? len : len & ~63ull;
            if (plain) {
                out.runs.push_back(Run{off, plain});
                seam_open = false;
                off += plain;
                len -= plain;
            }
            if (len) {  // the tail opens a seam block
                to_seam(off, len);
                fill = uint32_t(len);
            }
        }
        if (out.runs.size() == first_run) out.runs.push_back(Run{0, 0});
        out.total[size_t(i)] = total;
    }
    out.run0[size_t(n)] = out.runs.size();
    out.seam_bytes = out.copies.empty() ? 0 : out.copies.back().dst_off + out.copies.back().len;
}

// Which of a batch's objects the host hashes (host[i] != 0).  A device chain
// costs ~2 us per 64-byte block and a host core ~35-40 ns, and a launch lasts
// as long as its longest object, so the longest go to the host: with
// host_min_len == 0 as many as hybrid::split's model balances (`rate`: one
// host core's SHA-256 bytes per second; their bytes come back in one copy),
// else every object of at least host_min_len bytes.  An object without bytes
// stays on the device, unless nothing else does: then no launch is made for
// empty objects alone and the host settles them.
inline void split(const uint64_t *lens, size_t n, int threads, uint64_t host_min_len, double rate,
                  std::vector<uint8_t> &host)
{
    host.assign(n, 0);
    if (host_min_len) {
        for (size_t i = 0; i < n; ++i) host[i] = lens[i] >= host_min_len;
    } else if (n) {
        std::vector<size_t> order(n);
        std::iota(order.begin(), order.end(), size_t(0));
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return lens[a] > lens[b]; });
        std::vector<uint64_t> sd(n);
        for (size_t q = 0; q < n; ++q) sd[q] = lens[order[q]];
        size_t k = hybrid::split(sd, std::max(threads, 1), 1, rate);
        while (k > 0 && sd[k - 1] == 0) --k;
        for (size_t q = 0; q < k; ++q) host[order[q]] = 1;
    }
    bool device_bytes = false;
    for (size_t i = 0; i < n; ++i) device_bytes = device_bytes || (!host[i] && lens[i]);
    if (!device_bytes) host.assign(n, 1);
}

}  // namespace cplan
