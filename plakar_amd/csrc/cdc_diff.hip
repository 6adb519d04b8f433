// The device side of diff (include/plakar_cdc.h, "diff"): the line table of a
// batch of texts, the byte comparison behind the exact line ids, and the
// executor of an emit plan.
//
// cdc_line_table_device, three passes over texts cut into tiles of kTile bytes
// (tiles belong to one text; an empty text has one empty tile):
//   k_line_count  a wave per tile: 16-byte loads, the newline bytes of each
//                 dword found with a carry-free zero-byte test, a popcount per
//                 lane and one wave reduction per tile;
//   k_tile_scan   one workgroup walks the tile counts 256 at a time and
//                 carries the running sum, so any number of tiles is scanned;
//                 k_text_lines turns the scan into the line count of each text;
//   k_line_mark   a wave per tile again: a wave scan of the lanes' newline
//                 counts gives every newline its line number, and its lane
//                 writes the end of that line and the start of the next;
//   k_line_hash   a lane per line: off, len and the hash.  A line of
//                 `threshold` bytes or more is put on a list instead, and
//                 k_line_hash_long gives each listed line a whole wave.
// The hash of a line is the sum of the hashes of its 256-byte blocks (each
// seeded with its block number), mixed with the length at the end: a lane
// adds the blocks up one after the other, a wave takes 64 at a time and adds
// the lanes' sums, and both get the same value.
//
// k_line_verify / k_line_verify_long compare a line with its candidate leader
// byte for byte, by the same split.
//
// k_diff_emit executes an emit plan.  The host cuts the records into units: up
// to 64 short records (at most 8 KiB of output together) for one wave, whose
// lanes then walk the unit's output bytes and find each byte's record by a
// binary search over the unit's prefix sums in LDS; or a 16-KiB piece of one
// long record, copied with 16-byte stores at aligned destinations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "cdc_hostmem.h"
#include "cdc_internal.h"
#include "diff_plan.h"

namespace dl {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTile = 16384;
constexpr uint32_t kHashBlock = 256;
constexpr uint32_t kDefaultThreshold = 4096;
constexpr uint32_t kEmitLong = 2048;        // a record this long goes in pieces
constexpr uint32_t kEmitPiece = 16384;
constexpr uint32_t kEmitUnitBytes = 8192;   // output bytes of a unit of short records
constexpr int kBlocksPerCU = 8;
constexpr int kEmitBlocksPerCU = 32;        // k_diff_emit: one wave per workgroup

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));
typedef uint64_t u64_u __attribute__((aligned(1)));

struct Text {       // a text and its first tile
    uint64_t off;
    uint32_t len, tile0;
};
struct VerifyItem { // a line and its candidate leader: equal lengths
    uint64_t a, b;
    uint32_t len, reserved;
};
struct Unit {       // nrec > 0: records [rec0, rec0 + nrec); nrec == 0: bytes [piece_off, + piece_len) of record rec0
    uint32_t rec0, nrec, piece_off, piece_len;
};

template <class T>
__device__ __forceinline__ T dmin(T a, T b)
{
    return a < b ? a : b;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= uint32_t(d)) v += o;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor(uint32_t(v), d, 64), hi = __shfl_xor(uint32_t(v >> 32), d, 64);
        v += uint64_t(hi) << 32 | lo;
    }
    return v;
}

// 0x80 in every byte of w that is '\n'
__device__ __forceinline__ uint32_t nl_bits(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// bit k set: byte k of w is '\n'
__device__ __forceinline__ uint32_t nl_mask4(uint32_t w)
{
    const uint32_t y = nl_bits(w);
    return ((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u);
}

// bit k set: byte o + k of the text is '\n', for the 16 bytes at o clipped to hi (o < hi)
__device__ __forceinline__ uint32_t nl_mask16(const uint8_t *p, uint64_t o, uint64_t hi)
{
    if (o + 16 <= hi) {
        const u32x4 v = *reinterpret_cast<const u32x4_u *>(p + o);
        return nl_mask4(v.x) | nl_mask4(v.y) << 4 | nl_mask4(v.z) << 8 | nl_mask4(v.w) << 12;
    }
    uint32_t m = 0;
    for (uint32_t k = 0; o + k < hi; ++k) m |= uint32_t(p[o + k] == '\n') << k;
    return m;
}

__global__ __launch_bounds__(kThreads) void k_line_count(const uint8_t *data, const Text *texts, const uint32_t *tile_text,
                                                         uint32_t ntiles, uint32_t *tile_cnt)
{
    const uint32_t lane = threadIdx.x & 63, nwaves = gridDim.x * (kThreads / 64);
    for (uint32_t tile = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); tile < ntiles; tile += nwaves) {
        const Text T = texts[tile_text[tile]];
        const uint64_t lo = uint64_t(tile - T.tile0) * kTile, hi = dmin(lo + kTile, uint64_t(T.len));
        const uint8_t *p = data + T.off;
        uint32_t cnt = 0;
        for (uint64_t o = lo + lane * 16; o < hi; o += 1024) cnt += __popc(nl_mask16(p, o, hi));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) tile_cnt[tile] = cnt;
    }
}

// tile_base[i] = the newlines of tiles [0, i); tile_base[ntiles] = all of them
__global__ __launch_bounds__(kThreads) void k_tile_scan(const uint32_t *tile_cnt, uint32_t ntiles, uint32_t *tile_base)
{
    __shared__ uint32_t wsum[kThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kThreads) {
        const uint32_t i = base + tid, v = i < ntiles ? tile_cnt[i] : 0;
        const uint32_t incl = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kThreads / 64; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (i < ntiles) tile_base[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) tile_base[ntiles] = carry;
}

// counts[t] = the lines of text t (its newlines + 1); counts[n] = the lines of all texts
__global__ void k_text_lines(const Text *texts, uint32_t n, uint32_t ntiles, const uint32_t *tile_base, uint64_t *counts)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) counts[t] = uint64_t(tile_base[texts[t + 1].tile0] - tile_base[texts[t].tile0]) + 1;
    if (t == 0) counts[n] = uint64_t(tile_base[ntiles]) + n;
}

// Line g of the batch: text t's line j is g = tile_base[tile0(t)] + t + j.  The
// newline that ends line g writes its place to recs[g].hash[0] (k_line_hash
// reads it and puts the hash there) and the next byte's to recs[g + 1].off.
__global__ __launch_bounds__(kThreads) void k_line_mark(const uint8_t *data, const Text *texts, const uint32_t *tile_text,
                                                        uint32_t ntiles, const uint32_t *tile_base, cdc_line_rec *recs,
                                                        uint64_t cap)
{
    const uint32_t lane = threadIdx.x & 63, nwaves = gridDim.x * (kThreads / 64);
    for (uint32_t tile = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); tile < ntiles; tile += nwaves) {
        const uint32_t t = tile_text[tile];
        const Text T = texts[t];
        const uint64_t lo = uint64_t(tile - T.tile0) * kTile, hi = dmin(lo + kTile, uint64_t(T.len));
        const uint8_t *p = data + T.off;
        const uint64_t g = uint64_t(tile_base[tile]) + t;
        if (lo == 0 && lane == 0 && g < cap) recs[g].off = T.off;
        uint64_t run = 0;
        for (uint64_t o0 = lo; o0 < hi; o0 += 1024) {  // wave-uniform
            const uint64_t o = o0 + lane * 16;
            uint32_t m = o < hi ? nl_mask16(p, o, hi) : 0;
            const uint32_t c = __popc(m), incl = wave_incl_scan(c, lane);
            uint64_t idx = g + run + (incl - c);
            while (m) {
                const uint32_t k = __ffs(m) - 1;
                m &= m - 1;
                const uint64_t pos = T.off + o + k;
                if (idx < cap) recs[idx].hash[0] = pos;
                if (idx + 1 < cap) recs[idx + 1].off = pos + 1;
                ++idx;
            }
            run += __shfl(incl, 63, 64);
        }
        if (hi == T.len && lane == 0 && g + run < cap) recs[g + run].hash[0] = T.off + T.len;  // the text's last line
    }
}

// ---- the line hash ------------------------------------------------------------------
struct H2 {
    uint64_t x, y;
};
__device__ __forceinline__ uint64_t rotl64(uint64_t v, int r) { return v << r | v >> (64 - r); }
__device__ __forceinline__ uint64_t fmix64(uint64_t k)
{
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k;
}
// up to 8 bytes at p, zero-extended
__device__ __forceinline__ uint64_t load_tail(const uint8_t *p, uint32_t n)
{
    uint64_t w = 0;
    for (uint32_t k = 0; k < n; ++k) w |= uint64_t(p[k]) << (8 * k);
    return w;
}
// block `blk` of a line: n bytes (1..kHashBlock) at p
__device__ __forceinline__ H2 block_hash(const uint8_t *p, uint32_t n, uint64_t blk)
{
    uint64_t h1 = 0x243F6A8885A308D3ull ^ (blk + 1) * 0x9E3779B97F4A7C15ull;
    uint64_t h2 = 0x13198A2E03707344ull + (blk + 1) * 0xD6E8FEB86659FD93ull;
    uint32_t o = 0;
    for (; o + 8 <= n; o += 8) {
        const uint64_t w = *reinterpret_cast<const u64_u *>(p + o);
        h1 = rotl64((h1 ^ w) * 0x9E3779B97F4A7C15ull, 29);
        h2 = (h2 + w) * 0xC2B2AE3D27D4EB4Full;
        h2 ^= h2 >> 31;
    }
    if (o < n) {
        const uint64_t w = load_tail(p + o, n - o);
        h1 = rotl64((h1 ^ w) * 0x9E3779B97F4A7C15ull, 29);
        h2 = (h2 + w) * 0xC2B2AE3D27D4EB4Full;
        h2 ^= h2 >> 31;
    }
    return H2{fmix64(h1), fmix64(h2 ^ h1)};
}
__device__ __forceinline__ H2 line_final(uint64_t x, uint64_t y, uint32_t len)
{
    const uint64_t a = fmix64(x ^ (uint64_t(len) * 0xD6E8FEB86659FD93ull + 0xA4093822299F31D0ull));
    return H2{a, fmix64(y + a + len)};
}

__global__ __launch_bounds__(kThreads) void k_line_hash(const uint8_t *data, uint64_t data_len, cdc_line_rec *recs,
                                                        uint64_t nlines, uint32_t threshold, uint32_t *long_list,
                                                        uint32_t *long_cnt)
{
    const uint64_t g = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (g >= nlines) return;
    uint64_t off = recs[g].off, end = recs[g].hash[0];
    // k_line_mark wrote both from the bytes k_line_count saw; bytes that changed in between must not lead outside
    if (end > data_len || off > end) off = end = 0, recs[g].off = 0;
    const uint32_t len = uint32_t(end - off);
    recs[g].len = len;
    recs[g].reserved = 0;
    if (len >= threshold) {
        long_list[atomicAdd(long_cnt, 1u)] = uint32_t(g);  // at most nlines entries
        return;
    }
    uint64_t x = 0, y = 0;
    for (uint32_t o = 0; o < len; o += kHashBlock) {
        const H2 h = block_hash(data + off + o, dmin(kHashBlock, len - o), o / kHashBlock);
        x += h.x, y += h.y;
    }
    const H2 f = line_final(x, y, len);
    recs[g].hash[0] = f.x;
    recs[g].hash[1] = f.y;
}

__global__ __launch_bounds__(kThreads) void k_line_hash_long(const uint8_t *data, cdc_line_rec *recs, const uint32_t *long_list,
                                                             const uint32_t *long_cnt)
{
    const uint32_t lane = threadIdx.x & 63, nwaves = gridDim.x * (kThreads / 64), cnt = *long_cnt;
    for (uint32_t e = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); e < cnt; e += nwaves) {
        const uint32_t g = long_list[e];
        const uint64_t off = recs[g].off;
        const uint32_t len = recs[g].len;
        uint64_t x = 0, y = 0;
        for (uint64_t o = uint64_t(lane) * kHashBlock; o < len; o += 64 * kHashBlock) {
            const H2 h = block_hash(data + off + o, uint32_t(dmin(uint64_t(kHashBlock), len - o)), o / kHashBlock);
            x += h.x, y += h.y;
        }
        x = wave_sum64(x), y = wave_sum64(y);
        if (lane == 0) {
            const H2 f = line_final(x, y, len);
            recs[g].hash[0] = f.x;
            recs[g].hash[1] = f.y;
        }
    }
}

// ---- the byte comparison ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_line_verify(const uint8_t *data, const VerifyItem *items, uint32_t n,
                                                          uint32_t threshold, uint32_t *flags, uint32_t *long_list,
                                                          uint32_t *long_cnt)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const VerifyItem V = items[i];
    if (V.len >= threshold) {
        long_list[atomicAdd(long_cnt, 1u)] = i;
        return;
    }
    const uint8_t *a = data + V.a, *b = data + V.b;
    uint32_t o = 0, diff = 0;
    for (; o + 8 <= V.len && !diff; o += 8)
        diff = *reinterpret_cast<const u64_u *>(a + o) != *reinterpret_cast<const u64_u *>(b + o);
    for (; o < V.len && !diff; ++o) diff = a[o] != b[o];
    flags[i] = diff;
}

__global__ __launch_bounds__(kThreads) void k_line_verify_long(const uint8_t *data, const VerifyItem *items, uint32_t *flags,
                                                               const uint32_t *long_list, const uint32_t *long_cnt)
{
    const uint32_t lane = threadIdx.x & 63, nwaves = gridDim.x * (kThreads / 64), cnt = *long_cnt;
    for (uint32_t e = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); e < cnt; e += nwaves) {
        const uint32_t i = long_list[e];
        const VerifyItem V = items[i];
        const uint8_t *a = data + V.a, *b = data + V.b;
        uint32_t diff = 0;
        for (uint64_t o0 = 0; o0 < V.len; o0 += 512) {  // wave-uniform
            const uint64_t o = o0 + lane * 8;
            if (o + 8 <= V.len)
                diff |= *reinterpret_cast<const u64_u *>(a + o) != *reinterpret_cast<const u64_u *>(b + o);
            else if (o < V.len)
                diff |= load_tail(a + o, uint32_t(V.len - o)) != load_tail(b + o, uint32_t(V.len - o));
            if (__any(diff)) break;
        }
        const bool differ = __any(diff);
        if (lane == 0) flags[i] = differ ? 1u : 0u;
    }
}

// ---- the emit plan's executor ---------------------------------------------------------
// One wave per workgroup: __syncthreads() orders the wave's LDS traffic.
__global__ __launch_bounds__(64) void k_diff_emit(const uint8_t *plain, const uint8_t *lit, const cdc_emit_rec *recs,
                                                  const Unit *units, uint32_t nunits, uint8_t *dst)
{
    __shared__ uint32_t s_start[65];
    __shared__ const uint8_t *s_src[64];
    __shared__ uint8_t *s_dst[64];
    __shared__ uint32_t s_len[64], s_flags[64];
    const uint32_t lane = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const Unit U = units[u];
        if (U.nrec) {
            uint32_t sz = 0;
            if (lane < U.nrec) {
                const cdc_emit_rec r = recs[U.rec0 + lane];
                sz = r.len + ((r.flags >> 8) & 1u) + ((r.flags >> 10) & 1u);
                s_src[lane] = ((r.flags & CDC_EMIT_LITERAL) ? lit : plain) + r.src_off;
                s_dst[lane] = dst + r.dst_off;
                s_len[lane] = r.len;
                s_flags[lane] = r.flags;
            }
            const uint32_t incl = wave_incl_scan(sz, lane);
            s_start[lane + 1] = incl;
            if (lane == 0) s_start[0] = 0;
            __syncthreads();
            const uint32_t total = s_start[64];
            for (uint32_t b = lane; b < total; b += 64) {
                uint32_t lo = 0, hi = U.nrec;  // the last record with start <= b: a record of 0 bytes is never found
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_start[mid] <= b)
                        lo = mid;
                    else
                        hi = mid;
                }
                const uint32_t o = b - s_start[lo], f = s_flags[lo], hp = (f >> 8) & 1u;
                uint8_t v;
                if (hp && o == 0)
                    v = uint8_t(f);
                else if (o - hp < s_len[lo])
                    v = s_src[lo][o - hp];
                else
                    v = '\n';
                s_dst[lo][o] = v;
            }
            __syncthreads();
        } else {
            const cdc_emit_rec r = recs[U.rec0];
            const uint32_t hp = (r.flags >> 8) & 1u;
            const uint8_t *s = ((r.flags & CDC_EMIT_LITERAL) ? lit : plain) + r.src_off + U.piece_off;
            uint8_t *d = dst + r.dst_off + hp + U.piece_off;
            const uint32_t n = U.piece_len;
            const uint32_t head = dmin(n, uint32_t((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15));
            const uint32_t nvec = (n - head) >> 4, tail0 = head + 16 * nvec;
            if (lane < head) d[lane] = s[lane];
            for (uint32_t i = lane; i < nvec; i += 64)
                *reinterpret_cast<u32x4 *>(d + head + 16 * i) = *reinterpret_cast<const u32x4_u *>(s + head + 16 * i);
            if (lane >= 32 && lane - 32 < n - tail0) d[tail0 + lane - 32] = s[tail0 + lane - 32];
            if (lane == 0 && hp && U.piece_off == 0) dst[r.dst_off] = uint8_t(r.flags);
            if (lane == 1 && (r.flags & CDC_EMIT_NEWLINE) && U.piece_off + n == r.len) dst[r.dst_off + hp + r.len] = '\n';
        }
    }
}

// ---- host side ------------------------------------------------------------------------
struct Scratch {  // per device, kept across calls and grown on demand
    std::mutex mu;
    cdc::PinBuf h;
    cdc::DevBuf d, lst;
    hipEvent_t ev = nullptr;  // the emit scratch: its last launch (that call is asynchronous)
    bool used = false;
};
static Scratch &scratch(int device, int which)
{
    static Scratch *s = new Scratch[3 * cdc::kMaxDevices];  // never destroyed (DevBuf)
    return s[3 * (unsigned(device) % cdc::kMaxDevices) + which];
}
static std::atomic<uint32_t> g_threshold{kDefaultThreshold};

struct Drain {  // from the first enqueue on, every return drains the stream: the scratch is the next call's
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
};

static uint32_t grid_for(int device, uint64_t waves)
{
    const uint64_t blocks = (waves + kThreads / 64 - 1) / (kThreads / 64);
    return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(blocks, uint64_t(cdc::device_cus(device)) * kBlocksPerCU)));
}

// room != NULL (cdc::line_table_raw): the records go where room(ctx, lines) says, once the count is known, and
// k_line_hash does not run: a record then holds off, and in hash[0] the place of the line's end
static int line_table(int device, const uint8_t *d_data, uint64_t data_len, const uint64_t *text_off, const uint64_t *text_len, uint32_t n,
                      cdc_line_rec *d_recs, uint64_t cap, uint64_t *counts, uint64_t *total, hipStream_t st,
                      cdc::line_room_fn room = nullptr, void *room_ctx = nullptr)
{
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    uint64_t ntiles64 = 0;
    for (uint32_t t = 0; t < n; ++t) ntiles64 += std::max<uint64_t>(1, (text_len[t] + kTile - 1) / kTile);
    const uint32_t ntiles = uint32_t(ntiles64);  // at most n + 2^32 / kTile
    Scratch &S = scratch(device, 0);
    std::lock_guard<std::mutex> lk(S.mu);
    cdc::Carver hc(16), dc(16);
    const size_t h_texts = hc.take(sizeof(Text) * (size_t(n) + 1)), h_tt = hc.take(4 * size_t(ntiles));
    const size_t up_bytes = hc.bytes();
    const size_t h_counts = hc.take(8 * (size_t(n) + 1));
    const size_t d_texts = dc.take(sizeof(Text) * (size_t(n) + 1)), d_tt = dc.take(4 * size_t(ntiles));
    const size_t d_cnt = dc.take(4 * size_t(ntiles)), d_base = dc.take(4 * (size_t(ntiles) + 1));
    const size_t d_counts = dc.take(8 * (size_t(n) + 1)), d_lcnt = dc.take(16);
    (void)d_texts;
    if (!S.h.reserve(hc.bytes()) || !S.d.reserve(dc.bytes())) return CDC_E_NOMEM;
    uint8_t *const h = S.h.as<uint8_t>(), *const d = S.d.as<uint8_t>();
    Text *ht = reinterpret_cast<Text *>(h + h_texts);
    uint32_t *htt = reinterpret_cast<uint32_t *>(h + h_tt);
    uint32_t tile = 0;
    for (uint32_t t = 0; t < n; ++t) {
        ht[t] = Text{text_off[t], uint32_t(text_len[t]), tile};
        const uint32_t k = uint32_t(std::max<uint64_t>(1, (text_len[t] + kTile - 1) / kTile));
        for (uint32_t j = 0; j < k; ++j) htt[tile + j] = t;
        tile += k;
    }
    ht[n] = Text{0, 0, ntiles};
    const Text *dt = reinterpret_cast<const Text *>(d);
    const uint32_t *dtt = reinterpret_cast<const uint32_t *>(d + d_tt);
    uint32_t *dcnt = reinterpret_cast<uint32_t *>(d + d_cnt), *dbase = reinterpret_cast<uint32_t *>(d + d_base);
    uint64_t *dcounts = reinterpret_cast<uint64_t *>(d + d_counts);
    uint32_t *dlcnt = reinterpret_cast<uint32_t *>(d + d_lcnt);
    static_assert(sizeof(Text) == 16, "texts and the tile map share one upload");
    Drain drain{st};
    // the host carve's first two regions are the device carve's first two
    if (hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return CDC_E_DEVICE;
    const uint32_t tgrid = grid_for(device, ntiles);
    hipLaunchKernelGGL(k_line_count, dim3(tgrid), dim3(kThreads), 0, st, d_data, dt, dtt, ntiles, dcnt);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kThreads), 0, st, dcnt, ntiles, dbase);
    hipLaunchKernelGGL(k_text_lines, dim3((n + 255) / 256), dim3(256), 0, st, dt, n, ntiles, dbase, dcounts);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h + h_counts, dcounts, 8 * (size_t(n) + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return CDC_E_DEVICE;
    const uint64_t *hcounts = reinterpret_cast<const uint64_t *>(h + h_counts);
    const uint64_t nlines = hcounts[n];
    if (counts) std::memcpy(counts, hcounts, 8 * size_t(n));
    if (total) *total = nlines;
    if (nlines > cap) return CDC_E_NOSPACE;
    if (room) {
        if (!(d_recs = room(room_ctx, nlines))) return CDC_E_NOMEM;
        hipLaunchKernelGGL(k_line_mark, dim3(tgrid), dim3(kThreads), 0, st, d_data, dt, dtt, ntiles, dbase, d_recs, nlines);
        return hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess ? CDC_OK : CDC_E_DEVICE;
    }
    if (!S.lst.reserve(4 * size_t(nlines))) return CDC_E_NOMEM;
    uint32_t *dlist = S.lst.as<uint32_t>();
    if (hipMemsetAsync(dlcnt, 0, 16, st) != hipSuccess) return CDC_E_DEVICE;
    hipLaunchKernelGGL(k_line_mark, dim3(tgrid), dim3(kThreads), 0, st, d_data, dt, dtt, ntiles, dbase, d_recs, nlines);
    hipLaunchKernelGGL(k_line_hash, dim3(uint32_t((nlines + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_data,
                       data_len, d_recs, nlines, g_threshold.load(std::memory_order_relaxed), dlist, dlcnt);
    hipLaunchKernelGGL(k_line_hash_long, dim3(grid_for(device, nlines)), dim3(kThreads), 0, st, d_data, d_recs, dlist, dlcnt);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
    return CDC_OK;
}

// flags[i] = item i's two lines differ; one launch pair, synchronous
static int verify(int device, const uint8_t *d_data, const std::vector<VerifyItem> &items, std::vector<uint32_t> &flags,
                  hipStream_t st)
{
    const size_t n = items.size();
    flags.assign(n, 0);
    if (!n) return CDC_OK;
    Scratch &S = scratch(device, 1);
    std::lock_guard<std::mutex> lk(S.mu);
    cdc::Carver c(16);
    const size_t o_items = c.take(sizeof(VerifyItem) * n), o_flags = c.take(4 * n), o_list = c.take(4 * n), o_cnt = c.take(16);
    if (!S.h.reserve(c.bytes()) || !S.d.reserve(c.bytes())) return CDC_E_NOMEM;
    uint8_t *const h = S.h.as<uint8_t>(), *const d = S.d.as<uint8_t>();
    std::memcpy(h + o_items, items.data(), sizeof(VerifyItem) * n);
    Drain drain{st};
    if (hipMemcpyAsync(d + o_items, h + o_items, sizeof(VerifyItem) * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d + o_cnt, 0, 16, st) != hipSuccess)
        return CDC_E_DEVICE;
    const VerifyItem *di = reinterpret_cast<const VerifyItem *>(d + o_items);
    uint32_t *df = reinterpret_cast<uint32_t *>(d + o_flags), *dlist = reinterpret_cast<uint32_t *>(d + o_list);
    uint32_t *dcnt = reinterpret_cast<uint32_t *>(d + o_cnt);
    hipLaunchKernelGGL(k_line_verify, dim3(uint32_t((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_data, di,
                       uint32_t(n), g_threshold.load(std::memory_order_relaxed), df, dlist, dcnt);
    hipLaunchKernelGGL(k_line_verify_long, dim3(grid_for(device, n)), dim3(kThreads), 0, st, d_data, di, df, dlist, dcnt);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h + o_flags, df, 4 * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return CDC_E_DEVICE;
    std::memcpy(flags.data(), h + o_flags, 4 * n);
    return CDC_OK;
}

static int line_ids(int device, const uint8_t *d_data, const cdc_line_rec *recs, uint64_t nlines, const uint64_t *group,
                    uint32_t ngroups, int hash_bits, uint32_t *ids, uint32_t *rounds, hipStream_t st, int threads)
{
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    std::vector<dplan::Ids> I(ngroups);
    std::vector<uint64_t> todo, next;  // global line numbers, ascending
    {   // the hash maps, a group per task
        std::atomic<uint32_t> at{0};
        std::atomic<bool> oom{false};
        auto work = [&] {
            try {
                for (uint32_t g; (g = at.fetch_add(1)) < ngroups;)
                    I[g].propose(recs + group[g], size_t(group[g + 1] - group[g]), hash_bits);
            } catch (...) {
                oom.store(true);
            }
        };
        std::vector<std::thread> th;
        for (int k = 1; k < std::min<int>(std::max(threads, 1), int(std::min<uint32_t>(ngroups, 256))); ++k) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
        if (oom.load()) return CDC_E_NOMEM;
    }
    for (uint32_t g = 0; g < ngroups; ++g) {
        for (uint64_t i = group[g]; i < group[g + 1]; ++i)
            if (I[g].cand[size_t(i - group[g])] != i - group[g]) todo.push_back(i);
    }
    std::vector<VerifyItem> items;
    std::vector<uint32_t> flags;
    uint32_t nrounds = 0;
    for (bool first = true; !todo.empty(); first = false) {
        // in index order: a flagged line moves on, past every candidate of another length
        items.clear();
        next.clear();
        uint32_t g = 0;
        for (uint64_t i : todo) {
            while (i >= group[g + 1]) ++g;
            const cdc_line_rec *L = recs + group[g];
            const size_t k = size_t(i - group[g]);
            dplan::Ids &X = I[g];
            if (!first) X.relead(k);
            while (X.cand[k] != k && L[X.cand[k]].len != L[k].len) X.relead(k);
            if (X.cand[k] == k) continue;
            items.push_back(VerifyItem{L[k].off, L[X.cand[k]].off, L[k].len, 0});
            next.push_back(i);
        }
        if (items.empty()) break;
        const int s = verify(device, d_data, items, flags, st);
        if (s != CDC_OK) return s;
        ++nrounds;
        todo.clear();
        for (size_t j = 0; j < next.size(); ++j)
            if (flags[j]) todo.push_back(next[j]);
    }
    for (uint32_t g = 0; g < ngroups; ++g)
        std::memcpy(ids + group[g], I[g].cand.data(), 4 * size_t(group[g + 1] - group[g]));
    if (rounds) *rounds = nrounds;
    return CDC_OK;
}

static int emit(int device, const uint8_t *d_plain, const uint8_t *d_lit, const cdc_emit_rec *recs, uint64_t n, uint8_t *d_dst,
                hipStream_t st)
{
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    std::vector<Unit> units;
    Unit cur{0, 0, 0, 0};
    uint64_t cur_bytes = 0;
    auto close = [&] {
        if (cur.nrec) units.push_back(cur);
        cur = Unit{0, 0, 0, 0};
        cur_bytes = 0;
    };
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t out = dplan::rec_out_bytes(recs[i]);
        if (!out) continue;
        if (recs[i].len >= kEmitLong) {
            close();
            for (uint32_t o = 0; o < recs[i].len; o += kEmitPiece)
                units.push_back(Unit{uint32_t(i), 0, o, std::min(kEmitPiece, recs[i].len - o)});
            continue;
        }
        if (cur.nrec && (cur.nrec == 64 || cur_bytes + out > kEmitUnitBytes || cur.rec0 + cur.nrec != i)) close();
        if (!cur.nrec) cur.rec0 = uint32_t(i);
        ++cur.nrec;
        cur_bytes += out;
    }
    close();
    if (units.empty()) return CDC_OK;
    Scratch &S = scratch(device, 2);
    std::lock_guard<std::mutex> lk(S.mu);
    cdc::Carver c(16);
    const size_t o_recs = c.take(sizeof(cdc_emit_rec) * size_t(n)), o_units = c.take(sizeof(Unit) * units.size());
    // the scratch is reused, or freed to grow, only once the launch that read it has finished
    if (!S.ev && hipEventCreateWithFlags(&S.ev, hipEventDisableTiming) != hipSuccess) return CDC_E_DEVICE;
    if (S.used && hipEventSynchronize(S.ev) != hipSuccess) return CDC_E_DEVICE;
    if (!S.h.reserve(c.bytes()) || !S.d.reserve(c.bytes())) return CDC_E_NOMEM;
    uint8_t *const h = S.h.as<uint8_t>(), *const d = S.d.as<uint8_t>();
    std::memcpy(h + o_recs, recs, sizeof(cdc_emit_rec) * size_t(n));
    std::memcpy(h + o_units, units.data(), sizeof(Unit) * units.size());
    if (hipMemcpyAsync(d, h, c.bytes(), hipMemcpyHostToDevice, st) != hipSuccess) return CDC_E_DEVICE;
    const uint32_t grid = uint32_t(std::min<uint64_t>(units.size(), uint64_t(cdc::device_cus(device)) * kEmitBlocksPerCU));
    hipLaunchKernelGGL(k_diff_emit, dim3(grid), dim3(64), 0, st, d_plain, d_lit, reinterpret_cast<const cdc_emit_rec *>(d + o_recs),
                       reinterpret_cast<const Unit *>(d + o_units), uint32_t(units.size()), d_dst);
    S.used = true;  // even when the launch failed: the copy above reads the slot
    return hipGetLastError() == hipSuccess && hipEventRecord(S.ev, st) == hipSuccess ? CDC_OK : CDC_E_DEVICE;
}

}  // namespace dl

int cdc::line_ids(int device, const void *d_data, const cdc_line_rec *recs, uint64_t nlines, const uint64_t *group,
                  uint32_t ngroups, int hash_bits, uint32_t *ids, uint32_t *rounds, void *stream, int threads)
{
    return dl::line_ids(device, static_cast<const uint8_t *>(d_data), recs, nlines, group, ngroups, hash_bits, ids, rounds,
                        reinterpret_cast<hipStream_t>(stream), threads);
}

int cdc::line_table_raw(int device, const void *d_data, uint64_t len, const uint64_t *text_off, const uint64_t *text_len, uint32_t n,
                        uint64_t cap, line_room_fn room, void *ctx, uint64_t *counts, uint64_t *total, void *stream)
{
    return dl::line_table(device, static_cast<const uint8_t *>(d_data), len, text_off, text_len, n, nullptr, cap, counts, total,
                          reinterpret_cast<hipStream_t>(stream), room, ctx);
}

extern "C" {

int cdc_debug_set_line_threshold(uint32_t bytes)
{
    dl::g_threshold.store(bytes ? bytes : dl::kDefaultThreshold, std::memory_order_relaxed);
    return CDC_OK;
}

int cdc_line_table_device(int device, const void *d_data, uint64_t len, const uint64_t *text_off, const uint64_t *text_len,
                          uint32_t n, cdc_line_rec *d_recs, uint64_t cap, uint64_t *counts, uint64_t *total, void *stream)
{
    if (device < 0 || device >= cdc::kMaxDevices || (n && (!text_off || !text_len)) || (len && !d_data) ||
        (cap && (!d_recs || (reinterpret_cast<uintptr_t>(d_recs) & 15u))))
        return CDC_E_INVALID;
    uint64_t most = n;  // the lines there can be
    for (uint32_t t = 0; t < n; ++t) {
        if (text_len[t] > len || text_off[t] > len - text_len[t] || text_len[t] >= (1ull << 32)) return CDC_E_INVALID;
        most += text_len[t];
        if (most > 0xFFFFFFFEull) return CDC_E_INVALID;
    }
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    if (total) *total = 0;
    if (n == 0) return CDC_OK;
    try {
        return dl::line_table(device, static_cast<const uint8_t *>(d_data), len, text_off, text_len, n, d_recs, cap, counts, total,
                              reinterpret_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_line_ids_device(int device, const void *d_data, uint64_t len, const cdc_line_rec *recs, uint64_t nlines,
                        const uint64_t *group, uint32_t ngroups, int hash_bits, uint32_t *ids, uint32_t *rounds, void *stream)
{
    if (device < 0 || device >= cdc::kMaxDevices || !group || (nlines && (!recs || !ids)) || (len && !d_data) ||
        hash_bits < 0 || hash_bits > 128 || nlines >= 0xFFFFFFFFull)
        return CDC_E_INVALID;
    if (group[0] != 0 || group[ngroups] != nlines) return CDC_E_INVALID;
    for (uint32_t g = 0; g < ngroups; ++g)
        if (group[g] > group[g + 1]) return CDC_E_INVALID;
    for (uint64_t i = 0; i < nlines; ++i)
        if (recs[i].len > len || recs[i].off > len - recs[i].len) return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    if (rounds) *rounds = 0;
    if (nlines == 0) return CDC_OK;
    try {
        return dl::line_ids(device, static_cast<const uint8_t *>(d_data), recs, nlines, group, ngroups, hash_bits, ids, rounds,
                            reinterpret_cast<hipStream_t>(stream), 8);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

int cdc_diff_emit_device(int device, const void *d_plain, uint64_t plain_cap, const void *d_lit, uint64_t lit_cap,
                         const cdc_emit_rec *recs, uint64_t n, void *d_dst, uint64_t dst_cap, void *stream)
{
    if (device < 0 || device >= cdc::kMaxDevices || (n && !recs) || n > 0xFFFFFFFFull) return CDC_E_INVALID;
    uint64_t end = 0, written = 0;
    bool from_plain = false, from_lit = false;
    for (uint64_t i = 0; i < n; ++i) {
        const cdc_emit_rec &r = recs[i];
        if (r.flags & ~(0xFFu | CDC_EMIT_PREFIX | CDC_EMIT_LITERAL | CDC_EMIT_NEWLINE)) return CDC_E_INVALID;
        const uint64_t cap = (r.flags & CDC_EMIT_LITERAL) ? lit_cap : plain_cap;
        if (r.len > cap || r.src_off > cap - r.len) return CDC_E_INVALID;
        const uint64_t out = dplan::rec_out_bytes(r);
        if (out > dst_cap || r.dst_off > dst_cap - out || r.dst_off < end) return CDC_E_INVALID;
        end = r.dst_off + out;
        written += out;
        if (r.len) ((r.flags & CDC_EMIT_LITERAL) ? from_lit : from_plain) = true;
    }
    if ((written && !d_dst) || (from_plain && !d_plain) || (from_lit && !d_lit)) return CDC_E_INVALID;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(d_dst);
    auto aliases = [&](const void *p, uint64_t cap) {
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(p);
        return s0 < d0 + dst_cap && d0 < s0 + cap;
    };
    if (written && ((from_plain && aliases(d_plain, plain_cap)) || (from_lit && aliases(d_lit, lit_cap)))) return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    if (!written) return CDC_OK;
    try {
        return dl::emit(device, static_cast<const uint8_t *>(d_plain), static_cast<const uint8_t *>(d_lit), recs, n,
                        static_cast<uint8_t *>(d_dst), reinterpret_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

}  // extern "C"
