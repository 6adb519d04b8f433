// Host-only pieces of a sweep plan, shared by the library
// (cdc_state.cpp, cdc_state.hip) and the stand-alone sanitizer program
// tests/c/sweep_plan_check.cpp:
//
//   verdict       a packfile's KEEP / DROP / REPACK from its three integers;
//                 carries SWPLAN_FN, so that k_state_verdict compiles the same
//                 arithmetic for the device
//   group_repack  the repack rows, which the device leaves in record-number
//                 order, grouped by packfile in the packfile list's order and
//                 ascending in offset within one, with each packfile's slice
//
// No HIP, no library state: everything is a function of its arguments.
#pragma once

#include <stdint.h>
#include <string.h>

#include "plakar_cdc.h"

#ifndef SWPLAN_FN
#define SWPLAN_FN static inline
#endif

namespace swplan {

constexpr uint32_t kMaxPermille = 1000;

// live_bytes * 1000 < extent * permille without leaving 64 bits.  live_bytes
// is a sum of u32 lengths and extent at most 2^33, but neither is trusted to
// be: the products are taken in 128 bits as (hi, lo) pairs of 64.
SWPLAN_FN void mul_64x32(uint64_t a, uint32_t b, uint64_t *hi, uint64_t *lo)
{
    const uint64_t l = (a & 0xFFFFFFFFull) * b, h = (a >> 32) * b;  // each below 2^64
    *lo = l + (h << 32);
    *hi = (h >> 32) + (*lo < l ? 1 : 0);
}

// DROP: nothing live.  REPACK: something live, and live_bytes / extent below
// permille / 1000 (exactly at the threshold is KEEP; permille 0 never repacks,
// 1000 repacks every packfile that is not live to its last byte).  KEEP
// otherwise.
SWPLAN_FN int32_t verdict(uint64_t live_rows, uint64_t live_bytes, uint64_t extent, uint32_t permille)
{
    if (live_rows == 0) return CDC_SWEEP_DROP;
    uint64_t lh, ll, rh, rl;
    mul_64x32(live_bytes, 1000, &lh, &ll);
    mul_64x32(extent, permille, &rh, &rl);
    const bool below = lh < rh || (lh == rh && ll < rl);
    return below ? CDC_SWEEP_REPACK : CDC_SWEEP_KEEP;
}

}  // namespace swplan

#ifndef SWPLAN_NO_HOST

#include <algorithm>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "state_plan.h"

namespace swplan {

// rows[0, n): the live rows of REPACK packfiles in any order; packs[0, npacks)
// the packfile list.  Reorders rows in place (packfile in list order, then
// offset, then the order given: a stable sort) and sets row_first / row_count
// of every pack (0, 0 where it has no row here).  CDC_E_INVALID, with nothing
// changed, when a row names a packfile that is not in the list.
static inline int group_repack(cdc_state_row *rows, uint64_t n, cdc_sweep_pack *packs, uint64_t npacks)
{
    std::unordered_map<splan::Sum, uint64_t, splan::SumHash> index;
    index.reserve(size_t(npacks));
    for (uint64_t i = 0; i < npacks; ++i) {
        splan::Sum s;
        memcpy(s.b, packs[i].packfile, 32);
        index.emplace(s, i);
    }
    std::vector<uint64_t> of(size_t(n), 0);
    for (uint64_t i = 0; i < n; ++i) {
        splan::Sum s;
        memcpy(s.b, rows[i].packfile, 32);
        const auto it = index.find(s);
        if (it == index.end()) return CDC_E_INVALID;
        of[size_t(i)] = it->second;
    }
    std::vector<uint64_t> order(size_t(n), 0);
    std::iota(order.begin(), order.end(), uint64_t(0));
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (of[size_t(a)] != of[size_t(b)]) return of[size_t(a)] < of[size_t(b)];
        return rows[a].offset < rows[b].offset;
    });
    std::vector<cdc_state_row> sorted(size_t(n), cdc_state_row{});
    for (uint64_t i = 0; i < n; ++i) sorted[size_t(i)] = rows[order[size_t(i)]];
    for (uint64_t i = 0; i < npacks; ++i) packs[i].row_first = packs[i].row_count = 0;
    for (uint64_t i = 0; i < n; ++i) {
        cdc_sweep_pack &P = packs[of[size_t(order[size_t(i)])]];
        if (P.row_count++ == 0) P.row_first = i;
        rows[i] = sorted[size_t(i)];
    }
    return CDC_OK;
}

}  // namespace swplan

#endif  // SWPLAN_NO_HOST
