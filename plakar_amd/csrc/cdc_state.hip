// The state kernels: a repository's blob index built and
// queried in device memory.  All states of one cdc_state_merge call go through
// each stage in one launch; a grid-stride item finds its state and section by
// bisection over the exclusive sums of the record counts (Seg::first).
//
//   k_state_plan     one lane per state: the checked reader of state_plan.h,
//                    compiled for the device, over the decoded plaintext
//   k_state_index    IdToChecksum records -> per-state table id -> record
//                    position (compare-and-swap on a 0xFFFFFFFF-filled table:
//                    a second writer of an entry, or an id >= count, marks
//                    the state bad)
//   k_state_resolve  every location (and deleted-snapshot) record -> an
//                    80-byte cdc_state_row with both checksums, in the record
//                    store; a record's number there is its rank
//   k_state_insert   records -> the open-addressing table, keyed by (type,
//                    32-byte checksum); a slot holds the smallest record
//                    number of its key
//   k_state_lookup, k_state_rows, k_state_count: the queries
//
// Memory model.  The only words two lanes of one launch both touch are the id
// table's entries and the table's slots, and both are only ever accessed with
// agent-scope atomics (compare-and-swap, min, relaxed atomic loads: executed
// at the memory side, past the per-CU L1 and the per-XCD L2).  Everything a
// lane reads through a slot's value, a record's key, was written by an earlier
// launch on the same stream (k_state_resolve, or an earlier merge) and is
// visible at the kernel boundary.  No lane waits for another: a lane that
// loses a compare-and-swap compares keys and either lowers the slot with an
// atomic minimum or probes on, and every probe loop ends after `capacity`
// slots.
//
// Why the winner does not depend on scheduling: record numbers are given in
// (merge call, state order, section, record position) order before anything is
// inserted.  A slot's key never changes once set (it is only ever replaced by
// a smaller record number of the SAME key), so every record of a key walks the
// same probe sequence to the same slot, and the slot ends as the minimum of
// the numbers that reached it.
//
// Every index is checked before use: a section's range against the state's
// length (k_state_plan), an id against the state's id count, a table entry
// against kNoPos.  A bad state is a status and its records are voided by the
// host before the insert.
#include <hip/hip_runtime.h>

#define SPLAN_FN __host__ __device__ static inline
#define SPLAN_NO_WRITER
#include "cdc_state.h"

#include <algorithm>
#include <atomic>

#include "cdc_hostmem.h"

namespace cst {

constexpr uint32_t kThreads = 256;
constexpr int kBlocksPerCU = 8;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));

static std::atomic<uint32_t> g_blocks{0};

static uint32_t grid_for(int device, uint64_t items)
{
    const uint32_t cap = g_blocks.load(std::memory_order_relaxed);
    const uint64_t most = cap ? cap : uint64_t(cdc::device_cus(device)) * kBlocksPerCU;
    return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((items + kThreads - 1) / kThreads, most)));
}

static int launched() { return hipGetLastError() == hipSuccess ? CDC_OK : CDC_E_DEVICE; }

// The run that holds `item`: the last one whose first <= item (runs are not
// empty and item < the total, so there is one).
__device__ __forceinline__ uint32_t find_seg(const Seg *segs, uint32_t n, uint64_t item)
{
    uint32_t lo = 0, hi = n;  // segs[lo].first <= item < segs[hi].first
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (segs[mid].first <= item)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t mix_key(uint32_t type, u32x4 a, u32x4 b)
{
    // SHA-256 output: any bytes hash.  Bytes 0-7 and 24-31 and the type, so
    // that neither end alone decides the slot.
    uint64_t h = (uint64_t(a.y) << 32 | a.x) ^ ((uint64_t(b.w) << 32 | b.z) * 0x9E3779B97F4A7C15ull) ^
                 (uint64_t(type + 1) * 0xD6E8FEB86659FD93ull);
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 29;
    return h;
}

__device__ __forceinline__ bool same_key(const cdc_state_row *recs, uint64_t r, uint32_t type, u32x4 a, u32x4 b)
{
    const u32x4 *p = reinterpret_cast<const u32x4 *>(recs + r);
    const u32x4 x = p[0], y = p[1];
    const uint32_t t = reinterpret_cast<const uint32_t *>(recs + r)[18] & 0xFF;
    return t == type && x.x == a.x && x.y == a.y && x.z == a.z && x.w == a.w && y.x == b.x && y.y == b.y && y.z == b.z &&
           y.w == b.w;
}

// The record number the table holds for the key, or kEmpty.  Read-only use
// (no insert runs beside it).
__device__ __forceinline__ uint64_t probe(const Table &T, uint32_t type, u32x4 a, u32x4 b)
{
    const uint64_t h = mix_key(type, a, b);
    for (uint64_t i = 0; i <= T.mask; ++i) {
        const uint64_t s = T.slots[(h + i) & T.mask];
        if (s == kEmpty) return kEmpty;
        if (same_key(T.recs, s, type, a, b)) return s;
    }
    return kEmpty;
}

__global__ __launch_bounds__(kThreads) void k_state_plan(StateDesc *desc, uint32_t n, const uint8_t *plain)
{
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        StateDesc &D = desc[i];
        D.status = splan::read(plain + D.plain, D.len, &D.L);
        D.bad = 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_state_index(StateDesc *desc, const Seg *segs, uint32_t nsegs, uint64_t items,
                                                          const uint8_t *plain, uint32_t *idtab)
{
    for (uint64_t it = uint64_t(blockIdx.x) * kThreads + threadIdx.x; it < items; it += uint64_t(gridDim.x) * kThreads) {
        const Seg S = segs[find_seg(segs, nsegs, it)];
        const uint64_t j = it - S.first;  // < S.count, the state's id count: below 2^32
        const uint64_t id = splan::rd64(plain + S.src + splan::kIdBytes * j);
        bool ok = id < S.count;
        if (ok) ok = atomicCAS(idtab + desc[S.state].id_base + id, kNoPos, uint32_t(j)) == kNoPos;
        if (!ok) atomicOr(&desc[S.state].bad, 1u);
    }
}

__device__ __forceinline__ u32x4 load_sum(const uint8_t *p, int half)
{
    return *reinterpret_cast<const u32x4_u *>(p + 16 * half);
}

__global__ __launch_bounds__(kThreads) void k_state_resolve(StateDesc *desc, const Seg *segs, uint32_t nsegs,
                                                            uint64_t items, const uint8_t *plain, const uint32_t *idtab,
                                                            cdc_state_row *recs)
{
    for (uint64_t it = uint64_t(blockIdx.x) * kThreads + threadIdx.x; it < items; it += uint64_t(gridDim.x) * kThreads) {
        const Seg S = segs[find_seg(segs, nsegs, it)];
        const uint64_t j = it - S.first;
        const StateDesc &D = desc[S.state];
        const uint64_t nids = D.L.sec[splan::kSecIds].count;
        const uint8_t *ids = plain + D.plain + D.L.sec[splan::kSecIds].off;
        const bool loc = S.type != kTypeDeleted;
        const uint8_t *rec = plain + S.src + (loc ? splan::kLocBytes : splan::kDeletedBytes) * j;
        const uint64_t id = splan::rd64(rec), pack = loc ? splan::rd64(rec + 8) : id;
        uint32_t pi = kNoPos, pp = kNoPos;
        if (id < nids && pack < nids) {
            pi = idtab[D.id_base + id];
            pp = idtab[D.id_base + pack];
        }
        const bool ok = pi != kNoPos && pp != kNoPos;  // a position is below nids: k_state_index wrote it
        u32x4 w0 = {0, 0, 0, 0}, w1 = w0, w2 = w0, w3 = w0, w4 = w0;
        if (ok) {
            const uint8_t *sum = ids + splan::kIdBytes * pi + 8;
            w0 = load_sum(sum, 0), w1 = load_sum(sum, 1);
            if (loc) {
                const uint8_t *psum = ids + splan::kIdBytes * pp + 8;
                w2 = load_sum(psum, 0), w3 = load_sum(psum, 1);
                w4.x = splan::rd32(rec + 16), w4.y = splan::rd32(rec + 20);
            }
            w4.z = S.type | 1u << 8;  // type, found
        } else {
            atomicOr(&desc[S.state].bad, 1u);
        }
        u32x4 *out = reinterpret_cast<u32x4 *>(recs + S.out + j);
        out[0] = w0, out[1] = w1, out[2] = w2, out[3] = w3, out[4] = w4;
    }
}

__global__ __launch_bounds__(kThreads) void k_state_insert(const Table T, uint64_t lo, uint64_t hi)
{
    for (uint64_t r = lo + uint64_t(blockIdx.x) * kThreads + threadIdx.x; r < hi; r += uint64_t(gridDim.x) * kThreads) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(T.recs + r);
        const u32x4 a = p[0], b = p[1];
        const uint32_t tf = reinterpret_cast<const uint32_t *>(T.recs + r)[18];
        if (!(tf >> 8 & 0xFF)) continue;  // a voided record (its state was rejected)
        const uint32_t type = tf & 0xFF;
        const uint64_t h = mix_key(type, a, b);
        for (uint64_t i = 0; i <= T.mask; ++i) {
            unsigned long long *slot = reinterpret_cast<unsigned long long *>(T.slots + ((h + i) & T.mask));
            unsigned long long s = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s == kEmpty) {
                s = atomicCAS(slot, kEmpty, r);
                if (s == kEmpty) break;  // claimed
            }
            // taken, by record s: its key stays this slot's key for good
            if (same_key(T.recs, s, type, a, b)) {
                if (r < s) atomicMin(slot, r);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_state_count(const Table T, uint64_t *counts)
{
    __shared__ uint32_t hist[splan::kTypes + 1];
    if (threadIdx.x <= splan::kTypes) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= T.mask; i += uint64_t(gridDim.x) * kThreads) {
        const uint64_t s = T.slots[i];
        if (s == kEmpty) continue;
        const uint32_t t = T.recs[s].type;
        if (t <= splan::kTypes) atomicAdd(&hist[t], 1u);
    }
    __syncthreads();
    if (threadIdx.x <= splan::kTypes && hist[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long *>(counts) + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void k_state_lookup(const Table T, uint32_t type, const uint8_t *sums, uint64_t n,
                                                           cdc_state_row *outs)
{
    for (uint64_t q = uint64_t(blockIdx.x) * kThreads + threadIdx.x; q < n; q += uint64_t(gridDim.x) * kThreads) {
        const u32x4 a = load_sum(sums + 32 * q, 0), b = load_sum(sums + 32 * q, 1);
        const uint64_t s = probe(T, type, a, b);
        u32x4 w2 = {0, 0, 0, 0}, w3 = w2, w4 = w2;
        if (s != kEmpty) {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(T.recs + s);
            w2 = p[2], w3 = p[3], w4 = p[4];
        }
        w4.z = type | (s != kEmpty ? 1u << 8 : 0u);
        w4.w = 0;
        u32x4 *out = reinterpret_cast<u32x4 *>(outs + q);
        out[0] = a, out[1] = b, out[2] = w2, out[3] = w3, out[4] = w4;
    }
}

// The capacity is a multiple of the block size, so every lane of a wave makes
// the same number of trips and the ballot below sees whole waves.
__global__ __launch_bounds__(kThreads) void k_state_rows(const Table T, uint32_t type, cdc_state_row *outs, uint64_t cap,
                                                         uint64_t *n_out)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= T.mask; i += uint64_t(gridDim.x) * kThreads) {
        const uint64_t s = T.slots[i];
        bool hit = s != kEmpty && T.recs[s].type == type;
        if (hit && type == 0) {  // ListSnapshots: not the ones some merged state deleted
            const u32x4 *p = reinterpret_cast<const u32x4 *>(T.recs + s);
            hit = probe(T, kTypeDeleted, p[0], p[1]) == kEmpty;
        }
        // one atomic per wave: the hits take consecutive places
        const uint64_t votes = __ballot(hit);
        if (!votes) continue;
        const uint32_t lane = threadIdx.x & 63, leader = uint32_t(__ffsll((unsigned long long)votes)) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(reinterpret_cast<unsigned long long *>(n_out), (unsigned long long)__popcll(votes));
        base = __shfl(base, int(leader));
        const uint64_t at = base + __popcll(votes & ((1ull << lane) - 1));
        if (hit && at < cap) {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(T.recs + s);
            u32x4 *out = reinterpret_cast<u32x4 *>(outs + at);
            out[0] = p[0], out[1] = p[1], out[2] = p[2], out[3] = p[3], out[4] = p[4];
        }
    }
}

int launch_plan(int device, StateDesc *d_desc, uint32_t n, const uint8_t *d_plain, void *stream)
{
    if (!n) return CDC_OK;
    hipLaunchKernelGGL(k_state_plan, dim3(grid_for(device, n)), dim3(kThreads), 0, hipStream_t(stream), d_desc, n, d_plain);
    return launched();
}

int launch_index(int device, StateDesc *d_desc, const Seg *d_segs, uint32_t nsegs, uint64_t items, const uint8_t *d_plain,
                 uint32_t *d_idtab, void *stream)
{
    if (!items) return CDC_OK;
    hipLaunchKernelGGL(k_state_index, dim3(grid_for(device, items)), dim3(kThreads), 0, hipStream_t(stream), d_desc, d_segs,
                       nsegs, items, d_plain, d_idtab);
    return launched();
}

int launch_resolve(int device, StateDesc *d_desc, const Seg *d_segs, uint32_t nsegs, uint64_t items,
                   const uint8_t *d_plain, const uint32_t *d_idtab, cdc_state_row *d_recs, void *stream)
{
    if (!items) return CDC_OK;
    hipLaunchKernelGGL(k_state_resolve, dim3(grid_for(device, items)), dim3(kThreads), 0, hipStream_t(stream), d_desc,
                       d_segs, nsegs, items, d_plain, d_idtab, d_recs);
    return launched();
}

int launch_insert(int device, const Table &T, uint64_t lo, uint64_t hi, void *stream)
{
    if (lo >= hi) return CDC_OK;
    hipLaunchKernelGGL(k_state_insert, dim3(grid_for(device, hi - lo)), dim3(kThreads), 0, hipStream_t(stream), T, lo, hi);
    return launched();
}

int launch_count(int device, const Table &T, uint64_t *d_counts, void *stream)
{
    if (hipMemsetAsync(d_counts, 0, 8 * (splan::kTypes + 1), hipStream_t(stream)) != hipSuccess) return CDC_E_DEVICE;
    hipLaunchKernelGGL(k_state_count, dim3(grid_for(device, T.mask + 1)), dim3(kThreads), 0, hipStream_t(stream), T,
                       d_counts);
    return launched();
}

int launch_lookup(int device, const Table &T, uint32_t type, const uint8_t *d_sums, uint64_t n, cdc_state_row *d_out,
                  void *stream)
{
    if (!n) return CDC_OK;
    hipLaunchKernelGGL(k_state_lookup, dim3(grid_for(device, n)), dim3(kThreads), 0, hipStream_t(stream), T, type, d_sums, n,
                       d_out);
    return launched();
}

int launch_rows(int device, const Table &T, uint32_t type, cdc_state_row *d_out, uint64_t cap, uint64_t *d_n, void *stream)
{
    if (hipMemsetAsync(d_n, 0, 8, hipStream_t(stream)) != hipSuccess) return CDC_E_DEVICE;
    hipLaunchKernelGGL(k_state_rows, dim3(grid_for(device, T.mask + 1)), dim3(kThreads), 0, hipStream_t(stream), T, type,
                       d_out, cap, d_n);
    return launched();
}

}  // namespace cst

extern "C" int cdc_debug_set_state_blocks(uint32_t blocks)
{
    cst::g_blocks.store(blocks, std::memory_order_relaxed);
    return CDC_OK;
}
