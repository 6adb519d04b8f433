// cdc_assemble_device: the restore path's gather.  A batch's output image is
// put together from the plaintext of its distinct blobs: one segment per chunk
// occurrence, dst[dst_off, + len) = src[src_off, + len), the `copy(p, data)`
// of snapshot/vfs/vfilep.go:58-122 for every chunk of every file of the batch
// in one launch.
//
// Work is split by destination bytes.  The destination is cut into tiles of
// kTile bytes on 16-byte address boundaries; workgroups take tiles round
// robin, and a tile finds the segments that reach into it by a binary search
// over the sorted dst_off table, so one 4-MiB segment beside a thousand small
// ones is 64 tiles like any other 4 MiB.  Inside a tile each part of a segment
// is copied by the whole workgroup: 16-byte stores at 16-byte aligned
// destination addresses, one per lane, consecutive lanes on consecutive
// addresses; the loads are 16 bytes at whatever alignment the source offset
// leaves (gfx950 takes unaligned global loads; a misaligned one touches one
// more 16-byte granule, which the neighbouring lane's load touches as well).
// Tile boundaries are 16-byte aligned, so the byte-by-byte head and tail (at
// most 15 bytes each) occur only at a segment's own ends.
//
// Cache policy: the stores are nontemporal, the destination
// is written once and next read by the copy engine; the loads keep the default
// policy, since a deduplicated source is read many times and misaligned
// neighbours share their granules.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>

#include "cdc_hostmem.h"
#include "cdc_internal.h"

namespace asmb {

constexpr uint32_t kThreads = 256;
constexpr uint64_t kTile = 64u << 10;
constexpr int kBlocksPerCU = 8;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));

struct Job {
    const uint8_t *src;
    uint8_t *dst16;           // d_dst - mis: 16-byte aligned; addressed with v = dst offset + mis
    const uint64_t *dst_off;  // device tables of n rows: ascending, disjoint, no empty segment
    const uint64_t *src_off;
    const uint64_t *len;
    uint64_t n;
    uint64_t tile0, ntiles;   // tiles [tile0, tile0 + ntiles) of v space
    uint64_t mis;             // d_dst & 15
};

template <int POL>
__device__ __forceinline__ u32x4 load16(const uint8_t *p)
{
    const u32x4_u *q = reinterpret_cast<const u32x4_u *>(p);
    if (POL & 1) return __builtin_nontemporal_load(q);
    return *q;
}

template <int POL>
__device__ __forceinline__ void store16(uint8_t *p, u32x4 v)
{
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
    if (POL & 2)
        __builtin_nontemporal_store(v, q);
    else
        *q = v;
}

template <int POL>
__global__ __launch_bounds__(kThreads) void k_assemble(const Job J)
{
    const uint32_t tid = threadIdx.x;
    for (uint64_t t = blockIdx.x; t < J.ntiles; t += gridDim.x) {
        const uint64_t vlo = (J.tile0 + t) * kTile, vhi = vlo + kTile;
        // the last segment that starts at or before the tile: the only one
        // that can reach into it from the left
        uint64_t lo = 0, hi = J.n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (J.dst_off[mid] + J.mis <= vlo)
                lo = mid + 1;
            else
                hi = mid;
        }
        for (uint64_t s = lo ? lo - 1 : 0; s < J.n; ++s) {
            const uint64_t d0 = J.dst_off[s] + J.mis;
            if (d0 >= vhi) break;
            const uint64_t a = d0 > vlo ? d0 : vlo, e = d0 + J.len[s], b = e < vhi ? e : vhi;
            if (a >= b) continue;
            // destination byte v comes from sp[v - a]
            const uint8_t *sp = J.src + (J.src_off[s] + (a - d0));
            uint8_t *dp = J.dst16;
            const uint64_t up = (a + 15) & ~15ull, v0 = up < b ? up : b;   // head [a, v0)
            const uint64_t dn = b & ~15ull, v1 = dn > v0 ? dn : v0;         // body [v0, v1), tail [v1, b)
            if (tid < v0 - a) dp[a + tid] = sp[tid];
            if (tid >= 32 && tid - 32 < b - v1) dp[v1 + (tid - 32)] = sp[v1 - a + (tid - 32)];
            const uint64_t nvec = (v1 - v0) >> 4;
            const uint8_t *sv = sp + (v0 - a);
            uint8_t *dv = dp + v0;
            uint64_t i = tid;
            for (; i + 3 * kThreads < nvec; i += 4 * kThreads) {
                const u32x4 x0 = load16<POL>(sv + 16 * i), x1 = load16<POL>(sv + 16 * (i + kThreads));
                const u32x4 x2 = load16<POL>(sv + 16 * (i + 2 * kThreads)), x3 = load16<POL>(sv + 16 * (i + 3 * kThreads));
                store16<POL>(dv + 16 * i, x0);
                store16<POL>(dv + 16 * (i + kThreads), x1);
                store16<POL>(dv + 16 * (i + 2 * kThreads), x2);
                store16<POL>(dv + 16 * (i + 3 * kThreads), x3);
            }
            for (; i < nvec; i += kThreads) store16<POL>(dv + 16 * i, load16<POL>(sv + 16 * i));
        }
    }
}

// The segment tables travel through a small ring of pinned/device buffer
// pairs per device, so the call stays asynchronous: a slot is reused only once
// the launch that read it has finished (its event).
struct TabSlot {
    cdc::PinBuf h;
    cdc::DevBuf d;
    hipEvent_t ev = nullptr;
    bool used = false;
};
struct TabRing {
    std::mutex mu;
    TabSlot s[4];
    unsigned next = 0;
};
static TabRing *const g_ring = new TabRing[cdc::kMaxDevices];  // never destroyed (DevBuf)
static std::atomic<int> g_policy{2};

// The slot once its last launch is done, with room for `rows` rows of 24 bytes
// (it grows by half again, from 1,024 rows).
static int slot_reserve(TabSlot &S, size_t rows)
{
    if (!S.ev && hipEventCreateWithFlags(&S.ev, hipEventDisableTiming) != hipSuccess) return CDC_E_DEVICE;
    if (S.used && hipEventSynchronize(S.ev) != hipSuccess) return CDC_E_DEVICE;
    S.used = false;
    const size_t want = std::max<size_t>(rows + rows / 2, 1024);
    return S.h.reserve(rows * 24, want * 24) && S.d.reserve(rows * 24, want * 24) ? CDC_OK : CDC_E_NOMEM;
}

}  // namespace asmb

using namespace asmb;

extern "C" int cdc_debug_set_assemble_policy(int policy)
{
    if (policy < 0 || policy > 3) return CDC_E_INVALID;
    g_policy.store(policy, std::memory_order_relaxed);
    return CDC_OK;
}

extern "C" int cdc_assemble_device(int device, const void *d_src, uint64_t src_cap, const uint64_t *src_off,
                                   const uint64_t *len, const uint64_t *dst_off, uint64_t n, void *d_dst,
                                   uint64_t dst_cap, void *stream)
{
    if (device < 0 || device >= cdc::kMaxDevices || (n && (!src_off || !len || !dst_off))) return CDC_E_INVALID;
    uint64_t rows = 0, end = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (len[i] > src_cap || src_off[i] > src_cap - len[i]) return CDC_E_INVALID;
        if (len[i] > dst_cap || dst_off[i] > dst_cap - len[i]) return CDC_E_INVALID;
        if (dst_off[i] < end) return CDC_E_INVALID;  // unsorted, or it overlaps the one before
        end = dst_off[i] + len[i];
        rows += len[i] != 0;
    }
    if (rows && (!d_src || !d_dst)) return CDC_E_INVALID;
    if (rows) {  // the two buffers do not alias
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (s0 < d0 + dst_cap && d0 < s0 + src_cap) return CDC_E_INVALID;
    }
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    if (!rows) return CDC_OK;
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TabRing &R = g_ring[device];
    std::lock_guard<std::mutex> lk(R.mu);
    TabSlot &S = R.s[R.next++ % 4];
    int st = slot_reserve(S, rows);
    if (st != CDC_OK) return st;
    uint64_t *const h = S.h.as<uint64_t>(), *const d = S.d.as<uint64_t>();
    uint64_t k = 0, first = 0, last = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!len[i]) continue;
        if (!k) first = dst_off[i];
        last = dst_off[i] + len[i];
        h[k] = dst_off[i];
        h[rows + k] = src_off[i];
        h[2 * rows + k] = len[i];
        ++k;
    }
    Job J{};
    J.mis = reinterpret_cast<uintptr_t>(d_dst) & 15;
    J.src = static_cast<const uint8_t *>(d_src);
    J.dst16 = static_cast<uint8_t *>(d_dst) - J.mis;
    J.dst_off = d;
    J.src_off = d + rows;
    J.len = d + 2 * rows;
    J.n = rows;
    J.tile0 = (first + J.mis) / kTile;
    J.ntiles = (last + J.mis - 1) / kTile - J.tile0 + 1;
    const uint32_t grid = uint32_t(std::min<uint64_t>(J.ntiles, uint64_t(cdc::device_cus(device)) * kBlocksPerCU));
    if (hipMemcpyAsync(d, h, rows * 24, hipMemcpyHostToDevice, s) != hipSuccess) return CDC_E_DEVICE;
    switch (g_policy.load(std::memory_order_relaxed)) {
    case 0: hipLaunchKernelGGL(k_assemble<0>, dim3(grid), dim3(kThreads), 0, s, J); break;
    case 1: hipLaunchKernelGGL(k_assemble<1>, dim3(grid), dim3(kThreads), 0, s, J); break;
    case 3: hipLaunchKernelGGL(k_assemble<3>, dim3(grid), dim3(kThreads), 0, s, J); break;
    default: hipLaunchKernelGGL(k_assemble<2>, dim3(grid), dim3(kThreads), 0, s, J); break;
    }
    S.used = true;  // even when the launch failed: the copy above reads the slot
    if (hipGetLastError() != hipSuccess || hipEventRecord(S.ev, s) != hipSuccess) return CDC_E_DEVICE;
    return CDC_OK;
}
