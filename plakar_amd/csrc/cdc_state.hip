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
//   k_state_mark ... k_sweep_compact: maintenance, described
//                    where they stand, after k_state_insert
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
#define SWPLAN_FN __host__ __device__ static inline
#define SWPLAN_NO_HOST
#include "cdc_state.h"
#include "sweep_plan.h"

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

// Record r's key against (type, a, b).  The blob table's key is the record's
// type and checksum; the packfile table's (kPack) is the 32 bytes of its
// packfile, and the type is not part of it.
template <bool kPack>
__device__ __forceinline__ bool same_key_of(const cdc_state_row *recs, uint64_t r, uint32_t type, u32x4 a, u32x4 b)
{
    const u32x4 *p = reinterpret_cast<const u32x4 *>(recs + r) + (kPack ? 2 : 0);
    const u32x4 x = p[0], y = p[1];
    const uint32_t t = kPack ? type : reinterpret_cast<const uint32_t *>(recs + r)[18] & 0xFF;
    return t == type && x.x == a.x && x.y == a.y && x.z == a.z && x.w == a.w && y.x == b.x && y.y == b.y && y.z == b.z &&
           y.w == b.w;
}

__device__ __forceinline__ bool same_key(const cdc_state_row *recs, uint64_t r, uint32_t type, u32x4 a, u32x4 b)
{
    return same_key_of<false>(recs, r, type, a, b);
}

// Enter record r under its key: the slot of the key ends as the smallest
// record number that reached it.  True when this call claimed a free slot
// (once per key, whoever comes first).
template <bool kPack>
__device__ __forceinline__ bool enter(const Table &T, uint64_t r, uint32_t type, u32x4 a, u32x4 b)
{
    const uint64_t h = mix_key(type, a, b);
    for (uint64_t i = 0; i <= T.mask; ++i) {
        unsigned long long *slot = reinterpret_cast<unsigned long long *>(T.slots + ((h + i) & T.mask));
        unsigned long long s = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s == kEmpty) {
            s = atomicCAS(slot, kEmpty, r);
            if (s == kEmpty) return true;  // claimed
        }
        // taken, by record s: its key stays this slot's key for good
        if (same_key_of<kPack>(T.recs, s, type, a, b)) {
            if (r < s) atomicMin(slot, r);
            return false;
        }
    }
    return false;
}

// The slot that holds the key, or kEmpty.  Read-only use.
template <bool kPack>
__device__ __forceinline__ uint64_t slot_of(const Table &T, uint32_t type, u32x4 a, u32x4 b)
{
    const uint64_t h = mix_key(type, a, b);
    for (uint64_t i = 0; i <= T.mask; ++i) {
        const uint64_t at = (h + i) & T.mask, s = T.slots[at];
        if (s == kEmpty) return kEmpty;
        if (same_key_of<kPack>(T.recs, s, type, a, b)) return at;
    }
    return kEmpty;
}

// Adds the lanes' v to *dst: one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_add(uint64_t *dst, uint32_t v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
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
        enter<false>(T, r, tf & 0xFF, a, b);
    }
}

// ---- maintenance ----------------------------------------------------
//
//   k_state_mark     one lane per reference: probe the blob table, set the bit
//                    of the winner's record number in the mark bitmap
//   k_state_missing  the zeros of found[]
//   k_state_packs    every valid location record's packfile -> the packfile
//                    table (k_state_insert's algorithm over the other key)
//   k_state_sweep    per record: winner? live? the packfile's slot; extent,
//                    live rows and live bytes accumulated per slot; the live
//                    bitmap, one 64-bit word per wave
//   k_state_verdict  per packfile slot: the verdict, and the slot's entry of
//                    the packfile list
//   k_sweep_classes, k_sweep_scan, k_sweep_compact: the stable compaction of
//                    the live records into kept rows and repack rows
//
// Memory model.  The mark bitmap, the packfile table's slots and the per-slot
// accumulators are the words lanes share, and they are only touched with
// agent-scope atomics inside the launch that writes them (or, and, max, add,
// compare-and-swap, min); every reader is a later launch on the same stream.
// All sums are integer, so they do not depend on the order of arrival.  The
// live bitmap's words and the class bytes have one writer each.

__global__ __launch_bounds__(kThreads) void k_state_mark(const Table T, uint32_t type, const uint8_t *refs, uint64_t n,
                                                         uint32_t *marks, uint8_t *found)
{
    const bool per = type == kTypeOfRecord;
    for (uint64_t q = uint64_t(blockIdx.x) * kThreads + threadIdx.x; q < n; q += uint64_t(gridDim.x) * kThreads) {
        const uint8_t *rec = refs + (per ? kRefBytes : 32) * q;  // a 33-byte record has no alignment
        const uint32_t t = per ? rec[0] : type;
        const uint8_t *sum = rec + (per ? 1 : 0);
        const uint64_t s = probe(T, t, load_sum(sum, 0), load_sum(sum, 1));
        if (s != kEmpty) atomicOr(marks + (s >> 5), 1u << (s & 31));
        if (found) found[q] = s != kEmpty;
    }
}

__global__ __launch_bounds__(kThreads) void k_state_missing(const uint8_t *found, uint64_t n, uint64_t *missing)
{
    uint32_t zeros = 0;
    for (uint64_t q = uint64_t(blockIdx.x) * kThreads + threadIdx.x; q < n; q += uint64_t(gridDim.x) * kThreads)
        zeros += found[q] == 0;
    wave_add(missing, zeros);
}

__global__ __launch_bounds__(kThreads) void k_state_packs(const Table P, uint64_t nrecs, SweepCounts *counts)
{
    uint32_t claimed = 0;
    for (uint64_t r = uint64_t(blockIdx.x) * kThreads + threadIdx.x; r < nrecs; r += uint64_t(gridDim.x) * kThreads) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(P.recs + r);
        const uint32_t tf = reinterpret_cast<const uint32_t *>(P.recs + r)[18];
        if (!(tf >> 8 & 0xFF) || (tf & 0xFF) >= splan::kTypes) continue;  // voided, or a deletion: it names no packfile
        claimed += enter<true>(P, r, 0, p[2], p[3]);
    }
    wave_add(&counts->packs, claimed);
}

// A wave's lanes hold 64 consecutive records that start at a multiple of 64
// (the block size and the grid's stride are multiples of 64), and the loop
// runs to the record count rounded up to 64, so whole waves reach the ballot
// and lane 0 writes the wave's word of the live bitmap.
__global__ __launch_bounds__(kThreads) void k_state_sweep(const Table T, const Packs K, uint64_t nrecs, const uint32_t *marks,
                                                          uint32_t keep_types, uint64_t *live_words, uint64_t *slot_of_rec,
                                                          SweepCounts *counts)
{
    const uint64_t padded = (nrecs + 63) & ~63ull;
    uint32_t seen = 0, lives = 0, losers = 0;
    for (uint64_t r = uint64_t(blockIdx.x) * kThreads + threadIdx.x; r < padded; r += uint64_t(gridDim.x) * kThreads) {
        bool live = false;
        if (r < nrecs) {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(T.recs + r);
            const u32x4 w4 = p[4];
            const uint32_t type = w4.z & 0xFF;
            if ((w4.z >> 8 & 0xFF) && type < splan::kTypes) {
                ++seen;
                const u32x4 a = p[0], b = p[1];
                const bool winner = probe(T, type, a, b) == r;
                losers += !winner;
                live = winner && ((marks[r >> 5] >> (r & 31) & 1) || (keep_types >> type & 1));
                if (live && type == 0) live = probe(T, kTypeDeleted, a, b) == kEmpty;  // deletion beats a mark
                const uint64_t ps = slot_of<true>(K.P, 0, p[2], p[3]);
                if (ps == kEmpty) {
                    live = false;  // cannot be: k_state_packs entered every such record
                } else {
                    atomicMax(reinterpret_cast<unsigned long long *>(K.extent + ps), (unsigned long long)w4.x + w4.y);
                    if (live) {
                        atomicAdd(reinterpret_cast<unsigned long long *>(K.live_rows + ps), 1ull);
                        atomicAdd(reinterpret_cast<unsigned long long *>(K.live_bytes + ps), (unsigned long long)w4.y);
                        slot_of_rec[r] = ps;
                        ++lives;
                    }
                }
            }
        }
        const uint64_t votes = __ballot(live);
        if ((threadIdx.x & 63) == 0) live_words[r >> 6] = votes;
    }
    wave_add(&counts->seen, seen);
    wave_add(&counts->live, lives);
    wave_add(&counts->losers, losers);
}

__global__ __launch_bounds__(kThreads) void k_state_verdict(const Packs K, uint32_t permille, cdc_sweep_pack *list,
                                                            uint64_t cap, SweepCounts *counts)
{
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i <= K.P.mask; i += uint64_t(gridDim.x) * kThreads) {
        const uint64_t s = K.P.slots[i];
        if (s == kEmpty) continue;
        const int32_t v = swplan::verdict(K.live_rows[i], K.live_bytes[i], K.extent[i], permille);
        K.verdict[i] = v;
        // the list's order here is the order of arrival; the host sorts it by first_record
        const uint64_t at = atomicAdd(reinterpret_cast<unsigned long long *>(&counts->listed), 1ull);
        if (at >= cap) continue;
        cdc_sweep_pack e;  // 88 bytes, 8-byte aligned: stored as the struct it is
        memcpy(e.packfile, K.P.recs[s].packfile, 32);
        e.extent = K.extent[i], e.live_bytes = K.live_bytes[i], e.live_rows = K.live_rows[i];
        e.first_record = s, e.row_first = 0, e.row_count = 0, e.verdict = v, e.reserved = 0;
        list[at] = e;
    }
}

// One trip of a workgroup is one tile of kSweepTile records.  The class of a
// record: 0 nothing, 1 kept row, 2 repack row.
__global__ __launch_bounds__(kThreads) void k_sweep_classes(const Packs K, uint64_t nrecs, const uint64_t *live_words,
                                                            const uint64_t *slot_of_rec, uint8_t *cls, uint64_t *tiles)
{
    __shared__ uint32_t wcount[kThreads / 64][2];
    const uint64_t ntiles = (nrecs + kSweepTile - 1) / kSweepTile;
    const uint32_t wave = threadIdx.x >> 6;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t r = t * kSweepTile + threadIdx.x;
        uint32_t c = 0;
        if (r < nrecs) {
            if (live_words[r >> 6] >> (r & 63) & 1) {
                const int32_t v = K.verdict[slot_of_rec[r]];
                c = v == CDC_SWEEP_KEEP ? 1 : v == CDC_SWEEP_REPACK ? 2 : 0;
            }
            cls[r] = uint8_t(c);
        }
        const uint64_t k = __ballot(c == 1), q = __ballot(c == 2);
        if ((threadIdx.x & 63) == 0) wcount[wave][0] = __popcll(k), wcount[wave][1] = __popcll(q);
        __syncthreads();
        if (threadIdx.x < 2) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < kThreads / 64; ++w) sum += wcount[w][threadIdx.x];
            tiles[2 * t + threadIdx.x] = sum;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane)
{
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// One workgroup: tiles[0, 2 * ntiles) from counts to exclusive sums in place
// (kept at even, repack at odd indices), the totals at [2 * ntiles] and
// [2 * ntiles + 1] and in the counters.  256 values at a time with a carry, as
// k_tile_scan of cdc_diff.hip.
__global__ __launch_bounds__(kThreads) void k_sweep_scan(uint64_t *tiles, uint64_t ntiles, SweepCounts *counts)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t which = 0; which < 2; ++which) {
        uint64_t carry = 0;
        for (uint64_t base = 0; base < ntiles; base += kThreads) {
            const uint64_t i = base + tid;
            const uint32_t v = i < ntiles ? uint32_t(tiles[2 * i + which]) : 0;  // at most kSweepTile
            const uint32_t incl = wave_incl_scan(v, lane);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < kThreads / 64; ++w) {
                if (w < wave) before += wsum[w];
                all += wsum[w];
            }
            if (i < ntiles) tiles[2 * i + which] = carry + before + incl - v;
            carry += all;
            __syncthreads();
        }
        if (tid == 0) {
            tiles[2 * ntiles + which] = carry;
            (which ? counts->repack : counts->kept) = carry;
        }
    }
}

// A row's place is its tile's exclusive sum plus its rank in the tile: the
// rows of the earlier waves, then the lanes below it in its own ballot.  Record
// order comes out of the ranks.
__global__ __launch_bounds__(kThreads) void k_sweep_compact(const cdc_state_row *recs, uint64_t nrecs, const uint8_t *cls,
                                                            const uint64_t *tiles, cdc_state_row *kept, uint64_t kept_cap,
                                                            cdc_state_row *repack, uint64_t repack_cap)
{
    __shared__ uint32_t wcount[kThreads / 64][2];
    const uint64_t ntiles = (nrecs + kSweepTile - 1) / kSweepTile;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t r = t * kSweepTile + threadIdx.x;
        const uint32_t c = r < nrecs ? cls[r] : 0;
        const uint64_t k = __ballot(c == 1), q = __ballot(c == 2);
        if (lane == 0) wcount[wave][0] = __popcll(k), wcount[wave][1] = __popcll(q);
        __syncthreads();
        if (c == 1 || c == 2) {
            const uint32_t which = c - 1;
            uint32_t rank = __popcll((which ? q : k) & ((1ull << lane) - 1));
            for (uint32_t w = 0; w < wave; ++w) rank += wcount[w][which];
            const uint64_t at = tiles[2 * t + which] + rank;
            if (at < (which ? repack_cap : kept_cap)) {
                const u32x4 *p = reinterpret_cast<const u32x4 *>(recs + r);
                u32x4 *out = reinterpret_cast<u32x4 *>((which ? repack : kept) + at);
                out[0] = p[0], out[1] = p[1], out[2] = p[2], out[3] = p[3], out[4] = p[4];
            }
        }
        __syncthreads();
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

int launch_mark(int device, const Table &T, uint32_t type, const uint8_t *d_refs, uint64_t n, uint32_t *d_marks,
                uint8_t *d_found, void *stream)
{
    if (!n) return CDC_OK;
    hipLaunchKernelGGL(k_state_mark, dim3(grid_for(device, n)), dim3(kThreads), 0, hipStream_t(stream), T, type, d_refs, n,
                       d_marks, d_found);
    return launched();
}

int launch_missing(int device, const uint8_t *d_found, uint64_t n, uint64_t *d_missing, void *stream)
{
    if (hipMemsetAsync(d_missing, 0, 8, hipStream_t(stream)) != hipSuccess) return CDC_E_DEVICE;
    if (!n) return CDC_OK;
    hipLaunchKernelGGL(k_state_missing, dim3(grid_for(device, n)), dim3(kThreads), 0, hipStream_t(stream), d_found, n,
                       d_missing);
    return launched();
}

int launch_packs(int device, const Table &P, uint64_t nrecs, SweepCounts *d_counts, void *stream)
{
    if (!nrecs) return CDC_OK;
    hipLaunchKernelGGL(k_state_packs, dim3(grid_for(device, nrecs)), dim3(kThreads), 0, hipStream_t(stream), P, nrecs,
                       d_counts);
    return launched();
}

int launch_sweep(int device, const Table &T, const Packs &K, uint64_t nrecs, const uint32_t *d_marks, uint32_t keep_types,
                 uint64_t *d_live, uint64_t *d_slot, SweepCounts *d_counts, void *stream)
{
    if (!nrecs) return CDC_OK;
    hipLaunchKernelGGL(k_state_sweep, dim3(grid_for(device, nrecs)), dim3(kThreads), 0, hipStream_t(stream), T, K, nrecs,
                       d_marks, keep_types, d_live, d_slot, d_counts);
    return launched();
}

int launch_verdict(int device, const Packs &K, uint32_t permille, cdc_sweep_pack *d_list, uint64_t cap,
                   SweepCounts *d_counts, void *stream)
{
    hipLaunchKernelGGL(k_state_verdict, dim3(grid_for(device, K.P.mask + 1)), dim3(kThreads), 0, hipStream_t(stream), K,
                       permille, d_list, cap, d_counts);
    return launched();
}

int launch_classes(int device, const Packs &K, uint64_t nrecs, const uint64_t *d_live, const uint64_t *d_slot,
                   uint8_t *d_class, uint64_t *d_tiles, SweepCounts *d_counts, void *stream)
{
    if (!nrecs) return CDC_OK;
    hipLaunchKernelGGL(k_sweep_classes, dim3(grid_for(device, nrecs)), dim3(kThreads), 0, hipStream_t(stream), K, nrecs,
                       d_live, d_slot, d_class, d_tiles);
    if (launched() != CDC_OK) return CDC_E_DEVICE;
    hipLaunchKernelGGL(k_sweep_scan, dim3(1), dim3(kThreads), 0, hipStream_t(stream), d_tiles,
                       (nrecs + kSweepTile - 1) / kSweepTile, d_counts);
    return launched();
}

int launch_compact(int device, const cdc_state_row *d_recs, uint64_t nrecs, const uint8_t *d_class, const uint64_t *d_tiles,
                   cdc_state_row *d_kept, uint64_t kept_cap, cdc_state_row *d_repack, uint64_t repack_cap, void *stream)
{
    if (!nrecs) return CDC_OK;
    hipLaunchKernelGGL(k_sweep_compact, dim3(grid_for(device, nrecs)), dim3(kThreads), 0, hipStream_t(stream), d_recs, nrecs,
                       d_class, d_tiles, d_kept, kept_cap, d_repack, repack_cap);
    return launched();
}

}  // namespace cst

extern "C" int cdc_debug_set_state_blocks(uint32_t blocks)
{
    cst::g_blocks.store(blocks, std::memory_order_relaxed);
    return CDC_OK;
}
