// The device side of grep (include/plakar_cdc.h, "grep"): fixed strings in a
// batch of texts, reported per matching line.
//
// cdc_grep_device, over texts cut into tiles of kTile bytes (tiles belong to
// one text; an empty text has one empty tile):
//   the line table  cdc_line_table_device's kernels without k_line_hash
//                   (cdc::line_table_raw): a record per line with its first
//                   byte and its end;
//   k_grep_scan     position-parallel.  A workgroup keeps the query block
//                   (grep_plan.h) in LDS and takes tile after tile: the tile
//                   and a halo of 255 bytes, clipped to the text's end, go to
//                   LDS with 16-byte loads; a lane filters its 16 start
//                   positions of every 4-KiB step through the first-byte set
//                   and the two-byte bitmap and compares the survivors with the
//                   patterns that start with that byte.  A position's line is
//                   the tile's first line (a binary search over the records'
//                   offsets, once per tile) plus the newlines before it in the
//                   tile (a workgroup scan of the lanes' newline counts).  An
//                   occurrence must end inside the loaded bytes, which end with
//                   the text, and holds no newline since no pattern does: so it
//                   lies in one line of one text.  A lane adds up its
//                   occurrences of one line and then does one atomicOr (mask),
//                   atomicAdd (count) and atomicMax (~column) on the line;
//   k_grep_count, k_grep_block_scan, k_grep_rank
//                   the matching lines' ranks: a count per 256 lines, a scan of
//                   the counts by one workgroup, the exclusive rank of every
//                   line;
//   k_grep_text     per text: its lines by grep's count, its matching lines
//                   (the ranks at its first line and at the next text's);
//   k_grep_compact  a lane per line: a matching line whose rank in its text is
//                   below the limit writes its record at the text's base plus
//                   that rank.
// All grids are capped and stride.  Worst case of the scan: a text of one byte
// value against 32 patterns of 256 such bytes compares 8 KiB per position.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "cdc_hostmem.h"
#include "cdc_hostutil.h"
#include "cdc_internal.h"
#include "grep_plan.h"

namespace gr {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTile = 16384;
constexpr uint32_t kHalo = 255;               // kMaxPatternLen - 1
constexpr uint32_t kStep = kThreads * 16;     // start positions of one pass of the workgroup
constexpr uint32_t kTileLds = kTile + 272;    // the tile, the halo, and the last lane's look-ahead, in 16-byte units
constexpr int kScanBlocksPerCU = 4;           // 34,416 B of LDS each
constexpr int kBlocksPerCU = 8;

static_assert(gplan::kMaxPatternLen - 1 == kHalo && kTile % kStep == 0 && kTileLds % 16 == 0 && kTileLds >= kTile + kHalo + 1, "");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));

struct Text {  // a text, its first tile and its first line
    uint64_t off;
    uint32_t len, tile0, line0, reserved;
};
struct Acc {   // of a line; zero: no occurrence
    uint32_t mask, invcol;  // invcol: ~(the smallest column)
    unsigned long long nocc;
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

// bit k set: byte k of w is zero
__device__ __forceinline__ uint32_t zero_mask4(uint32_t x)
{
    const uint32_t y = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return ((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u);
}
__device__ __forceinline__ uint32_t eq_mask16(u32x4 v, uint32_t byte4)
{
    return zero_mask4(v.x ^ byte4) | zero_mask4(v.y ^ byte4) << 4 | zero_mask4(v.z ^ byte4) << 8 | zero_mask4(v.w ^ byte4) << 12;
}
__device__ __forceinline__ uint32_t dfold(uint32_t b) { return b - 'A' < 26u ? b | 0x20u : b; }
__device__ __forceinline__ uint32_t qbit(const uint32_t *w, uint32_t i) { return (w[i >> 5] >> (i & 31)) & 1u; }

__global__ __launch_bounds__(kThreads) void k_grep_scan(const uint8_t *data, const Text *texts, const uint32_t *tile_text,
                                                        uint32_t ntiles, const uint32_t *query, const cdc_line_rec *recs, Acc *acc,
                                                        uint32_t *binary)
{
    __shared__ uint32_t s_q[gplan::kMaxBlockBytes / 4];
    __shared__ u32x4 s_tile4[kTileLds / 16];
    __shared__ uint32_t s_wsum[kThreads / 64];
    __shared__ uint32_t s_line;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t qwords = dmin(query[gplan::kBlockBytes] / 4, gplan::kMaxBlockBytes / 4);
    for (uint32_t i = tid; i < qwords; i += kThreads) s_q[i] = query[i];
    const uint8_t *s_tile = reinterpret_cast<const uint8_t *>(s_tile4);
    const uint8_t *s_pat = reinterpret_cast<const uint8_t *>(s_q + gplan::kBytes);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t t = tile_text[tile];
        const Text T = texts[t];
        const uint32_t line_end = texts[t + 1].line0;
        const uint32_t lo = (tile - T.tile0) * kTile;
        const uint32_t tlen = dmin(kTile, T.len - lo), avail = dmin(kTile + kHalo, T.len - lo);
        const uint8_t *p = data + T.off + lo;
        __syncthreads();  // the query block is there; the tile before this one is done with
        for (uint32_t i = tid * 16; i < avail; i += kStep) {
            if (i + 16 <= avail) {
                s_tile4[i >> 4] = *reinterpret_cast<const u32x4_u *>(p + i);
            } else {
                uint8_t *d = reinterpret_cast<uint8_t *>(s_tile4);
                for (uint32_t k = i; k < avail; ++k) d[k] = p[k];
            }
        }
        if (tid == 0) {  // the line the tile's first byte lies in: the last one that starts at or before it
            uint32_t a = T.line0, b = line_end;
            const uint64_t pos = T.off + lo;
            while (lo && b - a > 1) {
                const uint32_t mid = a + (b - a) / 2;
                if (recs[mid].off <= pos)
                    a = mid;
                else
                    b = mid;
            }
            s_line = a;
        }
        __syncthreads();
        const bool ic = (s_q[gplan::kFlags] & CDC_GREP_IGNORE_CASE) != 0;
        const uint32_t line0 = s_line;
        uint32_t run = 0, zacc = 0;  // run: the newlines of the steps before this one
        for (uint32_t s0 = 0; s0 < tlen; s0 += kStep) {  // uniform over the workgroup
            const uint32_t o = s0 + tid * 16;
            const u32x4 v = s_tile4[o >> 4];
            const uint32_t nvalid = o < tlen ? dmin(16u, tlen - o) : 0u, vm = (1u << nvalid) - 1u;
            const uint32_t nl = eq_mask16(v, 0x0A0A0A0Au) & vm;
            zacc |= eq_mask16(v, 0u) & vm;
            uint32_t next = __shfl_down(v.x & 0xFFu, 1, 64);  // the byte after the lane's 16
            if (lane == 63) next = s_tile[o + 16];
            const uint32_t c = __popc(nl), incl = wave_incl_scan(c, lane);
            if (lane == 63) s_wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (uint32_t w = 0; w < kThreads / 64; ++w) {
                if (w < wave) before += s_wsum[w];
                all += s_wsum[w];
            }
            const uint32_t g0 = line0 + run + before + incl - c;  // the line of the lane's first byte
            run += all;
            // the filter: bit k of cand set, position o + k may start a pattern
            uint32_t cand = 0;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
                const uint32_t wn = k + 1 < 4 ? v.x : k + 1 < 8 ? v.y : k + 1 < 12 ? v.z : v.w;
                const uint32_t b0 = (w >> (8 * (k & 3))) & 0xFFu;
                const uint32_t b1 = k == 15 ? next : (wn >> (8 * ((k + 1) & 3))) & 0xFFu;
                if (qbit(s_q + gplan::kFirst, b0) && (qbit(s_q + gplan::kOne, b0) || qbit(s_q + gplan::kPrefix, b0 | b1 << 8)))
                    cand |= 1u << k;
            }
            cand &= vm;
            // the survivors, in position order; the occurrences of one line are added up before they go out
            uint32_t cur_g = 0, cur_mask = 0, cur_cnt = 0, cur_min = 0;
            auto flush = [&] {
                if (!cur_cnt || cur_g >= line_end) return;
                const uint64_t col = T.off + lo + cur_min - recs[cur_g].off;
                atomicOr(&acc[cur_g].mask, cur_mask);
                atomicAdd(&acc[cur_g].nocc, static_cast<unsigned long long>(cur_cnt));
                atomicMax(&acc[cur_g].invcol, ~uint32_t(col));
            };
            while (cand) {
                const uint32_t k = __ffs(cand) - 1, q = o + k;
                cand &= cand - 1;
                uint32_t pm = s_q[gplan::kStart + s_tile[q]], hit = 0, cnt = 0;
                while (pm) {
                    const uint32_t j = __ffs(pm) - 1, m = s_q[gplan::kLen + j];
                    pm &= pm - 1;
                    if (q + m > avail) continue;  // past the text's end (or the halo: never, m <= 256)
                    const uint8_t *pat = s_pat + s_q[gplan::kOff + j];
                    uint32_t i = 0;
                    for (; i < m; ++i) {
                        const uint32_t x = s_tile[q + i];
                        if ((ic ? dfold(x) : x) != pat[i]) break;
                    }
                    if (i == m) hit |= 1u << j, ++cnt;
                }
                if (!hit) continue;
                const uint32_t g = g0 + __popc(nl & ((1u << k) - 1u));
                if (cur_cnt && g != cur_g) {
                    flush();
                    cur_cnt = 0, cur_mask = 0;
                }
                if (!cur_cnt) cur_g = g, cur_min = q;
                cur_mask |= hit;
                cur_cnt += cnt;
            }
            flush();
            __syncthreads();  // s_wsum is the next step's
        }
        if (__any(zacc != 0) && lane == 0) atomicOr(&binary[t], 1u);
    }
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *s_w, uint32_t tid, uint32_t *before)
{
    const uint32_t lane = tid & 63, wave = tid >> 6, incl = wave_incl_scan(v, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t b = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
        if (w < wave) b += s_w[w];
        all += s_w[w];
    }
    __syncthreads();
    *before = b + incl - v;
    return all;
}

// blk_cnt[b] = the matching lines among lines [256 b, 256 b + 256)
__global__ __launch_bounds__(kThreads) void k_grep_count(const Acc *acc, uint32_t nlines, uint32_t nblk, uint32_t *blk_cnt)
{
    __shared__ uint32_t s_w[kThreads / 64];
    for (uint32_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const uint32_t g = b * kThreads + threadIdx.x;
        uint32_t before;
        const uint32_t all = block_sum(g < nlines && acc[g].mask ? 1u : 0u, s_w, threadIdx.x, &before);
        if (threadIdx.x == 0) blk_cnt[b] = all;
    }
}

// base[i] = cnt[0] + ... + cnt[i - 1]; base[n] = all of them
__global__ __launch_bounds__(kThreads) void k_grep_block_scan(const uint32_t *cnt, uint32_t n, uint32_t *base)
{
    __shared__ uint32_t s_w[kThreads / 64];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += kThreads) {
        const uint32_t i = b0 + threadIdx.x;
        uint32_t before;
        const uint32_t all = block_sum(i < n ? cnt[i] : 0u, s_w, threadIdx.x, &before);
        if (i < n) base[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) base[n] = carry;
}

// rank[g] = the matching lines before line g; rank[nlines] = all of them
__global__ __launch_bounds__(kThreads) void k_grep_rank(const Acc *acc, uint32_t nlines, uint32_t nblk, const uint32_t *blk_base,
                                                        uint32_t *rank)
{
    __shared__ uint32_t s_w[kThreads / 64];
    for (uint32_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const uint32_t g = b * kThreads + threadIdx.x;
        uint32_t before;
        (void)block_sum(g < nlines && acc[g].mask ? 1u : 0u, s_w, threadIdx.x, &before);
        if (g < nlines) rank[g] = blk_base[b] + before;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) rank[nlines] = blk_base[nblk];
}

// The table's lines of a text are its newlines + 1: the last one is empty when
// the text is, or ends in a newline, and grep does not count it.
__global__ void k_grep_text(const Text *texts, uint32_t n, const cdc_line_rec *recs, const uint32_t *rank, uint64_t *lines,
                            uint64_t *matched)
{
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const uint32_t l0 = texts[t].line0, l1 = texts[t + 1].line0;
        const cdc_line_rec last = recs[l1 - 1];
        lines[t] = uint64_t(l1 - l0) - (last.hash[0] == last.off ? 1u : 0u);
        matched[t] = rank[l1] - rank[l0];
    }
}

__global__ __launch_bounds__(kThreads) void k_grep_compact(const Text *texts, uint32_t n, const cdc_line_rec *recs, const Acc *acc,
                                                           const uint32_t *rank, const uint64_t *out0, uint64_t limit,
                                                           uint32_t nlines, uint64_t data_len, cdc_grep_hit *hits)
{
    for (uint64_t g64 = uint64_t(blockIdx.x) * kThreads + threadIdx.x; g64 < nlines; g64 += uint64_t(gridDim.x) * kThreads) {
        const uint32_t g = uint32_t(g64);
        const Acc A = acc[g];
        if (!A.mask) continue;
        uint32_t a = 0, b = n;  // the last text whose first line is at or before g
        while (b - a > 1) {
            const uint32_t mid = a + (b - a) / 2;
            if (texts[mid].line0 <= g)
                a = mid;
            else
                b = mid;
        }
        const uint32_t l0 = texts[a].line0;
        const uint64_t r = rank[g] - rank[l0];
        if (limit && r >= limit) continue;
        uint64_t off = recs[g].off, end = recs[g].hash[0];
        // the table wrote both from the bytes its count saw; bytes that changed in between must not lead outside
        if (end > data_len || off > end) off = end = 0;
        cdc_grep_hit H;
        H.text = a;
        H.line = g - l0 + 1;
        H.off = off;
        H.len = uint32_t(end - off);
        H.col = ~A.invcol;
        H.mask = A.mask;
        H.nocc = A.nocc > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(A.nocc);
        hits[out0[a] + r] = H;
    }
}

// ---- host side ------------------------------------------------------------------------
using cdc::Clock;
using cdc::since;

struct Scratch {  // per device, kept across calls and grown on demand
    std::mutex mu;
    cdc::PinBuf h;
    cdc::DevBuf d, recs, lines;
};
static Scratch &scratch(int device)
{
    static Scratch *s = new Scratch[cdc::kMaxDevices];  // never destroyed (DevBuf)
    return s[unsigned(device) % cdc::kMaxDevices];
}
static std::atomic<uint32_t> g_blocks{0};

struct Drain {  // from the first enqueue on, every return drains the stream: the scratch is the next call's
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
};

static uint32_t grid_for(int device, uint64_t blocks, int per_cu)
{
    const uint32_t cap = g_blocks.load(std::memory_order_relaxed);
    const uint64_t most = cap ? cap : uint64_t(cdc::device_cus(device)) * uint64_t(per_cu);
    return uint32_t(std::max<uint64_t>(1, std::min(blocks, most)));
}

static cdc_line_rec *recs_room(void *ctx, uint64_t nlines)
{
    Scratch *S = static_cast<Scratch *>(ctx);
    return S->recs.reserve(sizeof(cdc_line_rec) * size_t(nlines)) ? S->recs.as<cdc_line_rec>() : nullptr;
}

static int run(int device, const uint8_t *d_data, uint64_t data_len, const uint64_t *text_off, const uint64_t *text_len, uint32_t n,
               const gplan::Query &Q, uint64_t limit, cdc::grep_room_fn room, void *room_ctx, uint64_t *lines, uint64_t *matched,
               uint8_t *binary, uint64_t *total, hipStream_t st, double *times)
{
    if (hipSetDevice(device) != hipSuccess) return CDC_E_DEVICE;
    uint64_t ntiles64 = 0;
    for (uint32_t t = 0; t < n; ++t) ntiles64 += std::max<uint64_t>(1, (text_len[t] + kTile - 1) / kTile);
    const uint32_t ntiles = uint32_t(ntiles64);  // at most n + 2^32 / kTile
    Scratch &S = scratch(device);
    std::lock_guard<std::mutex> lk(S.mu);
    auto t0 = Clock::now();
    // ---- the line table
    cdc::Carver hc(16), dc(16);
    const uint32_t qbytes = Q.block[gplan::kBlockBytes];
    const size_t o_texts = hc.take(sizeof(Text) * (size_t(n) + 1)), o_tt = hc.take(4 * size_t(ntiles)), o_q = hc.take(qbytes);
    const size_t up_bytes = hc.bytes();
    const size_t o_out0 = hc.take(8 * size_t(n));
    const size_t o_lines = hc.take(8 * size_t(n)), o_matched = hc.take(8 * size_t(n)), o_bin = hc.take(4 * size_t(n));
    const size_t o_counts = hc.take(8 * size_t(n));
    if (!S.h.reserve(hc.bytes()) || !S.d.reserve(hc.bytes())) return CDC_E_NOMEM;  // one layout on both sides
    uint8_t *const h = S.h.as<uint8_t>(), *const d = S.d.as<uint8_t>();
    uint64_t *counts = reinterpret_cast<uint64_t *>(h + o_counts);
    uint64_t nlines64 = 0;
    Drain drain{st};
    int s = cdc::line_table_raw(device, d_data, data_len, text_off, text_len, n, 0xFFFFFFFEull, recs_room, &S, counts, &nlines64, st);
    if (s != CDC_OK) return s == CDC_E_NOSPACE ? CDC_E_INVALID : s;
    const uint32_t nlines = uint32_t(nlines64);
    const cdc_line_rec *d_recs = S.recs.as<cdc_line_rec>();
    if (times) times[0] += since(t0);
    t0 = Clock::now();
    // ---- the scan
    Text *ht = reinterpret_cast<Text *>(h + o_texts);
    uint32_t *htt = reinterpret_cast<uint32_t *>(h + o_tt);
    uint32_t tile = 0, line = 0;
    for (uint32_t t = 0; t < n; ++t) {
        ht[t] = Text{text_off[t], uint32_t(text_len[t]), tile, line, 0};
        const uint32_t k = uint32_t(std::max<uint64_t>(1, (text_len[t] + kTile - 1) / kTile));
        for (uint32_t j = 0; j < k; ++j) htt[tile + j] = t;
        tile += k;
        line += uint32_t(counts[t]);
    }
    ht[n] = Text{0, 0, ntiles, nlines, 0};
    std::memcpy(h + o_q, Q.block.data(), qbytes);
    const uint32_t nblk = (nlines + kThreads - 1) / kThreads;
    cdc::Carver lc(16);
    const size_t l_acc = lc.take(sizeof(Acc) * size_t(nlines)), l_rank = lc.take(4 * (size_t(nlines) + 1));
    const size_t l_cnt = lc.take(4 * size_t(nblk)), l_base = lc.take(4 * (size_t(nblk) + 1));
    if (!S.lines.reserve(lc.bytes())) return CDC_E_NOMEM;
    uint8_t *const dl = S.lines.as<uint8_t>();
    const Text *dt = reinterpret_cast<const Text *>(d + o_texts);
    const uint32_t *dtt = reinterpret_cast<const uint32_t *>(d + o_tt), *dq = reinterpret_cast<const uint32_t *>(d + o_q);
    uint32_t *dbin = reinterpret_cast<uint32_t *>(d + o_bin);
    uint64_t *dlines = reinterpret_cast<uint64_t *>(d + o_lines), *dmatched = reinterpret_cast<uint64_t *>(d + o_matched);
    uint64_t *dout0 = reinterpret_cast<uint64_t *>(d + o_out0);
    Acc *dacc = reinterpret_cast<Acc *>(dl + l_acc);
    uint32_t *drank = reinterpret_cast<uint32_t *>(dl + l_rank), *dcnt = reinterpret_cast<uint32_t *>(dl + l_cnt);
    uint32_t *dbase = reinterpret_cast<uint32_t *>(dl + l_base);
    if (hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(dacc, 0, sizeof(Acc) * size_t(nlines), st) != hipSuccess ||
        hipMemsetAsync(dbin, 0, 4 * size_t(n), st) != hipSuccess)
        return CDC_E_DEVICE;
    hipLaunchKernelGGL(k_grep_scan, dim3(grid_for(device, ntiles, kScanBlocksPerCU)), dim3(kThreads), 0, st, d_data, dt, dtt, ntiles,
                       dq, d_recs, dacc, dbin);
    if (hipGetLastError() != hipSuccess) return CDC_E_DEVICE;
    if (times) {
        if (hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
        times[1] += since(t0);
        t0 = Clock::now();
    }
    // ---- ranks, the counts of the texts, the records
    const uint32_t lgrid = grid_for(device, nblk, kBlocksPerCU);
    hipLaunchKernelGGL(k_grep_count, dim3(lgrid), dim3(kThreads), 0, st, dacc, nlines, nblk, dcnt);
    hipLaunchKernelGGL(k_grep_block_scan, dim3(1), dim3(kThreads), 0, st, dcnt, nblk, dbase);
    hipLaunchKernelGGL(k_grep_rank, dim3(lgrid), dim3(kThreads), 0, st, dacc, nlines, nblk, dbase, drank);
    hipLaunchKernelGGL(k_grep_text, dim3(grid_for(device, (uint64_t(n) + 255) / 256, kBlocksPerCU)), dim3(256), 0, st, dt, n, d_recs,
                       drank, dlines, dmatched);
    // lines, matched and binary lie one after the other on both sides
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h + o_lines, d + o_lines, o_counts - o_lines, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return CDC_E_DEVICE;
    const uint64_t *hlines = reinterpret_cast<const uint64_t *>(h + o_lines), *hmatched = reinterpret_cast<const uint64_t *>(h + o_matched);
    const uint32_t *hbin = reinterpret_cast<const uint32_t *>(h + o_bin);
    uint64_t *hout0 = reinterpret_cast<uint64_t *>(h + o_out0);
    uint64_t all = 0;
    for (uint32_t t = 0; t < n; ++t) {
        hout0[t] = all;
        all += limit ? std::min(hmatched[t], limit) : hmatched[t];
        if (binary) binary[t] = uint8_t(hbin[t] != 0);
    }
    if (lines) std::memcpy(lines, hlines, 8 * size_t(n));
    if (matched) std::memcpy(matched, hmatched, 8 * size_t(n));
    if (total) *total = all;
    int ret = CDC_OK;
    if (all) {
        cdc_grep_hit *d_hits = room(room_ctx, all);
        if (!d_hits) {
            ret = CDC_E_NOSPACE;
        } else {
            if (hipMemcpyAsync(dout0, hout0, 8 * size_t(n), hipMemcpyHostToDevice, st) != hipSuccess) return CDC_E_DEVICE;
            hipLaunchKernelGGL(k_grep_compact, dim3(lgrid), dim3(kThreads), 0, st, dt, n, d_recs, dacc, drank, dout0, limit, nlines,
                               data_len, d_hits);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return CDC_E_DEVICE;
        }
    }
    if (times) times[2] += since(t0);
    return ret;
}

struct Fixed {
    cdc_grep_hit *d_hits;
    uint64_t cap;
};
static cdc_grep_hit *fixed_room(void *ctx, uint64_t total)
{
    const Fixed *F = static_cast<const Fixed *>(ctx);
    return total <= F->cap ? F->d_hits : nullptr;
}

// the arguments of cdc_grep_device but the patterns and d_hits: CDC_OK or CDC_E_INVALID
static int check_texts(int device, const void *d_data, uint64_t len, const uint64_t *text_off, const uint64_t *text_len, uint32_t n)
{
    if (device < 0 || device >= cdc::kMaxDevices || (n && (!text_off || !text_len)) || (len && !d_data)) return CDC_E_INVALID;
    uint64_t most = n, end = 0;  // most: the lines there can be
    for (uint32_t t = 0; t < n; ++t) {
        if (text_len[t] > len || text_off[t] > len - text_len[t] || text_len[t] >= (1ull << 32) || text_off[t] < end) return CDC_E_INVALID;
        end = text_off[t] + text_len[t];
        most += text_len[t];
        if (most > 0xFFFFFFFEull) return CDC_E_INVALID;
    }
    return CDC_OK;
}

}  // namespace gr

int cdc::grep_texts(int device, const void *d_data, uint64_t len, const uint64_t *text_off, const uint64_t *text_len, uint32_t n,
                    const uint8_t *const *patterns, const uint32_t *pattern_len, uint32_t npatterns, uint32_t flags, uint64_t limit,
                    grep_room_fn room, void *ctx, uint64_t *lines, uint64_t *matched, uint8_t *binary, uint64_t *total, void *stream,
                    double *times)
{
    gplan::Query Q;
    if (gr::check_texts(device, d_data, len, text_off, text_len, n) != CDC_OK ||
        gplan::compile(patterns, pattern_len, npatterns, flags, Q) != CDC_OK || !room)
        return CDC_E_INVALID;
    if (total) *total = 0;
    if (n == 0) return CDC_OK;
    return gr::run(device, static_cast<const uint8_t *>(d_data), len, text_off, text_len, n, Q, limit, room, ctx, lines, matched,
                   binary, total, reinterpret_cast<hipStream_t>(stream), times);
}

extern "C" {

int cdc_debug_set_grep_blocks(uint32_t blocks)
{
    gr::g_blocks.store(blocks, std::memory_order_relaxed);
    return CDC_OK;
}

int cdc_grep_device(int device, const void *d_data, uint64_t len, const uint64_t *text_off, const uint64_t *text_len, uint32_t n,
                    const uint8_t *const *patterns, const uint32_t *pattern_len, uint32_t npatterns, uint32_t flags, uint64_t limit,
                    cdc_grep_hit *d_hits, uint64_t cap, uint64_t *lines, uint64_t *matched, uint8_t *binary, uint64_t *total,
                    void *stream)
{
    if (gr::check_texts(device, d_data, len, text_off, text_len, n) != CDC_OK ||
        gplan::validate(patterns, pattern_len, npatterns, flags) != CDC_OK ||
        (cap && (!d_hits || (reinterpret_cast<uintptr_t>(d_hits) & 15u))))
        return CDC_E_INVALID;
    if (!cdc::device_count_initialised()) return CDC_E_NOT_INIT;
    try {
        gr::Fixed F{d_hits, cap};
        return cdc::grep_texts(device, d_data, len, text_off, text_len, n, patterns, pattern_len, npatterns, flags, limit,
                               gr::fixed_room, &F, lines, matched, binary, total, stream, nullptr);
    } catch (const std::bad_alloc &) {
        return CDC_E_NOMEM;
    }
}

}  // extern "C"
